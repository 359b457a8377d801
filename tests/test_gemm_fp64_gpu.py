"""GPU suite: every kernel launch_gemm can launch, alone, against a float64 product (tests/gemm_fp64_common.py: the cases, the
reference and the bounds; tests/test_gemm_fp64_cpu.py: the same table on the launch plan, and the bounds on emulations).

Each case goes through digat_gemm_launch, the one entry that takes a whole GemmArgs: the kernel the plan chose must be the one the
case names, every segment is held to the reference within the bound of its product set and output format, and nothing else is
written.  Inputs sit as column blocks of wider NaN-filled matrices with NaN rows above and below; outputs are NaN-prefilled
(EPI_ACCUM: prefilled with the values it adds to) with guard columns and guard rows, and after the call every guard element and
every row outside the row list holds its prefill bit for bit.  The split image is made per call in a scratch filled with 0xFF
and forgotten around it.  Launches on the fp16 pieces carry a range flag: it stays 0, and is raised by the cases that hold an
activation of 5000 (whose outputs are not compared).

Bounds: the module docstring of tests/gemm_fp64_common.py — the rule of test_linear_mfma_f32 on the value in front of the epilogue
(x max(|e0|, |e1|) behind the gate: the sigmoid's slope is at most 1/4), the dropped products of x3_segs / x1_segs from the piece
widths, half a bf16 / e4m3 ulp for the reduced outputs, the bounds of tests/test_hip_fp8c.py for the fp16-fp8c kernel.

Worst err / bound per kernel, measured on an MI355X (every figure is to stay below 1; nothing is tuned to them):
    fp32 MFMA         F32_32 0.049, F32_64 0.064, F32_128 0.056, F32_128_PROJ 0.059, one launch per segment 0.054
    skinny fp32       <1> 0.031, <1, KTAIL> 0.034, <2> 0.082, <2, KTAIL> 0.059; weights transposed <1> 0.035, <2> 0.077
    skinny split      bf16x6 <1> 0.037, <2> 0.114; fp16x3 <1> 0.090, <2> 0.244
    strip, all products   fp32 outputs 0.040 - 0.074 over the nine instantiations, the three ragged ones and both tile orders
    strip, x3_segs    bf16x6 0.134; fp16x3 (its full product, held to the full-precision rule) 0.074
    strip, x1_segs    bf16x6 0.344; fp16x3 0.434
    strip, outputs    bf16 0.990, e4m3 elements 0.941 (0.919 under x1_segs), e4m3 block scales 0.363 (0.018 with all products):
                      a rounding to nearest reaches half an ulp, these two cannot be far below 1
    fp16-fp8c         against fp64 <1> 0.268, <3> 0.260; against its quantiser 0.432, 0.340
The first run found one defect: the one-strip fp16x3 kernels at K = 32 (a single K tile) raised the range flag on operands of
ordinary size, from an A buffer in LDS that was split without ever being written (strip_1_f16_k32, strip_1_f16_64_k32; fixed in
gemm_bf16x6s_kernel's prologue).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_fp64_common as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def _report(family, what, cases, **worst):
    print(f"[{family}] {what}: worst err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" over {cases} cases")


class Block:
    """A [rows, cols] operand as the kernels may meet it: a column block of a wider matrix with a row above and a row below, the
    rest filled with `fill` (NaN as floats); keeps the prefill to compare against afterwards."""

    def __init__(self, rows, cols, ld, col, dtype, fill, value=None):
        host = torch.full((rows + 2, ld), fill, dtype=dtype)
        if value is not None:
            host[1:1 + rows, col:col + cols] = torch.from_numpy(np.ascontiguousarray(value))
        self.rows, self.cols, self.col = rows, cols, col
        self.before = host
        self.t = host.to(DEV)
        self.ptr = self.t.data_ptr() + (ld + col) * self.t.element_size()

    def after(self):
        return self.t.cpu()

    def untouched_outside(self, written, what):
        """Every element but [written rows, the block's columns] holds its prefill, bit for bit; returns the block [rows, cols]."""
        now = self.after()
        bits = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[now.element_size()]
        same = now.view(bits) == self.before.view(bits)
        inside = torch.zeros_like(same)
        inside[1:1 + self.rows, self.col:self.col + self.cols] = torch.from_numpy(written)[:, None]
        assert bool(same[~inside].all()), f"{what}: written outside the rows and columns of the launch ({int((~same[~inside]).sum())} elements)"
        return now[1:1 + self.rows, self.col:self.col + self.cols].numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(name, case, image=None):
    """One digat_gemm_launch of the case; image: a ready-made split image to name instead of splitting into a scratch."""
    from digat_amd import _lib
    L = _lib.lib()
    o = G.draw(name, case)
    ld = G.layout(case)
    M, K, nseg, nsegs = case["M"], case["K"], case["nseg"], case["nsegs"]
    k0 = case.get("k0", K)
    nan = float("nan")
    keep, ptr = [], {}

    def block(key, value, ldk, col, dtype=torch.float32, fill=nan):
        b = Block(value.shape[0], value.shape[1], ldk, col, dtype, fill, value)
        keep.append(b)
        ptr[key] = b.ptr

    def flat(key, value):
        t = _dev(value)
        keep.append(t)
        ptr[key] = t.data_ptr()

    block("a0", o["x"][:, :k0], ld["lda0"], 4)
    if k0 < K:
        block("a1", o["x"][:, k0:], ld["lda1"], 8)
    for s in range(nsegs):
        flat(f"w{s}", o["w"][s].T if case.get("transW") else o["w"][s])
        if o["bias"] is not None:
            flat(f"bias{s}", o["bias"][s])
    for k, col in (("e0", 8), ("e1", 4), ("e2", 4)):
        if k in o:
            block(k, o[k], ld["ld" + k], col)
    if "radd" in o:
        flat("radd", o["radd"])
    if "dmask" in o:
        block("dmask", o["dmask"], ld["lddm"], 4, torch.uint8, 255)
    if "rowidx" in o:
        flat("rowidx", o["rowidx"])
        flat("nrows", np.array([o["nrows"]], dtype=np.int32))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr["range_flag"] = flag.data_ptr()
    ys = []
    for s in range(nsegs):
        if G.seg_mask(case, "fp8_segs", s):
            y = Block(M, nseg + 4 * (nseg // 80), ld["ldy8"], 16, torch.uint8, 255)
        elif G.seg_mask(case, "bf16_segs", s):
            y = Block(M, nseg, ld["ldy"], 4, torch.int16, -1)
        else:
            y = Block(M, nseg, ld["ldy"], 4, torch.float32, nan, o["y_before"][s] if "y_before" in o else None)
        ys.append(y)
        ptr[f"y{s}"] = y.ptr
    scratch = None
    fmt = case.get("fmt")
    if image is not None:
        ptr["wsplit"] = image.data_ptr()
    elif fmt is not None:
        scratch = torch.full((L.digat_split_weights_bytes_format(nseg * nsegs, K, fmt),), 255, dtype=torch.uint8, device=DEV)
        L.digat_forget_split_image(scratch.data_ptr())
    g = G.fill_args(case, ptr)
    kernel = C.c_int(-1)
    torch.cuda.synchronize()
    rc = L.digat_gemm_launch(C.addressof(g), C.sizeof(g), G.KIND[case.get("kind")], scratch.data_ptr() if scratch is not None else None,
                             C.byref(kernel), _lib.stream_ptr())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a fault of the device: no later case may launch on it
        pytest.exit(f"{name}: {e}", returncode=3)
    if scratch is not None:
        L.digat_forget_split_image(scratch.data_ptr())
    return dict(rc=rc, kernel=kernel.value, ys=ys, flag=int(flag.item()), o=o, keep=keep)


def _run(name, case):
    """Launch, and hold every segment to the reference; returns the worst err / bound."""
    r = _launch(name, case)
    assert r["rc"] == 0, (name, r["rc"])
    assert r["kernel"] == G.kernel_ids()[case["kernel"]], (name, G.kernel_name(r["kernel"]))
    o = r["o"]
    written = G.written_rows(case, o)
    blocks = [y.untouched_outside(written, f"{name} segment {s}") for s, y in enumerate(r["ys"])]
    worst = {}
    if case.get("big"):
        assert r["flag"] == 1, f"{name}: an activation of 5000 did not raise the range flag"
        return worst
    assert r["flag"] == 0, f"{name}: the range flag was raised by operands of ordinary size"
    ref = G.reference(case, o)
    tol = G.tolerances(case, o, ref)
    for s, (pre, want) in enumerate(ref):
        got = blocks[s]
        if got.dtype == np.int16:
            got = got.view(np.uint16)
        kind = G.output_kind(case, s) if G.products_of(case, s) == "full" else f"{G.output_kind(case, s)} {G.products_of(case, s)}"
        worst[kind] = max(worst.get(kind, 0.0), G.check_segment(case, s, got, want, tol[s], written, f"{name} segment {s}", worst))
    if case["kernel"].startswith("F16F8C"):
        # against the restated quantiser: only the accumulation order is the kernel's (and the rounding of an adding epilogue's store)
        emu = G.reference(case, o, np.float64, lambda s, A, w: G.emulate_f16f8c(A, w))
        rowmax = np.max(np.abs(np.concatenate([pre for pre, _ in emu], axis=1)), axis=1, keepdims=True)
        for s, (pre, want) in enumerate(emu):
            t = 1e-6 * rowmax + (2.0 ** -24 * np.abs(want) if case.get("epi") else 0.0)
            q = G.check_segment(case, s, blocks[s], want, np.broadcast_to(t, want.shape), written, f"{name} segment {s} against its quantiser")
            worst["quantiser"] = max(worst.get("quantiser", 0.0), q)
    return worst


def _family(case):
    k = case["kernel"]
    return ("strip " if k.startswith("STRIP") else "") + k + (f" ragged {case['ragged_plan']}" if case.get("ragged_plan") else "")


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_kernel_alone_against_fp64(name):
    case = G.CASES[name]
    worst = _run(name, case)
    mine = WORST.setdefault(_family(case), {"cases": 0})
    mine["cases"] += 1
    for k, v in worst.items():
        mine[k] = max(mine.get(k, 0.0), v)
    if worst:
        _report(_family(case), name, 1, **worst)


def test_worst_per_kernel():
    """The figures of the module docstring (run the whole file with -s): per kernel, by output format and product set."""
    for key in sorted(WORST):
        _report(key, "all cases", WORST[key]["cases"], **{k: v for k, v in WORST[key].items() if k != "cases"})
    assert all(v <= 1.0 for w in WORST.values() for k, v in w.items() if k != "cases")


@pytest.mark.parametrize("name", sorted(G.REFUSED))
def test_refused_launches_write_nothing(name):
    """The launch returns the plan's error (for an image of another format: the launch's, from the library's record of the images
    it has split) and leaves the NaN-filled outputs as they were."""
    from digat_amd import _lib
    L = _lib.lib()
    case, status = G.REFUSED[name]
    image = None
    if "image_fmt" in case:
        o = G.draw(name, case)
        w = _dev(o["w"][0])
        image = torch.full((L.digat_split_weights_bytes_format(case["nseg"], case["K"], case["image_fmt"]),), 255, dtype=torch.uint8, device=DEV)
        _lib.check(L.digat_split_weights(w.data_ptr(), case["nseg"], case["K"], image.data_ptr(), case["image_fmt"], _lib.stream_ptr()), "split")
    try:
        r = _launch(name, case, image)
    finally:
        if image is not None:
            L.digat_forget_split_image(image.data_ptr())
    assert r["rc"] == status, (name, r["rc"])
    assert r["kernel"] == G.kernel_ids()[case["kernel"]], (name, G.kernel_name(r["kernel"]))
    for s, y in enumerate(r["ys"]):
        y.untouched_outside(np.zeros(case["M"], dtype=bool), f"{name} segment {s}")


def test_entry_refuses_what_it_cannot_launch():
    from digat_amd import _lib
    L = _lib.lib()
    case = G.CASES["f32_32_m40"]
    g = G.fill_args(case, G.fake_pointers(case))
    kernel = C.c_int(-1)
    call = lambda g, size=C.sizeof(G.GemmArgs), kind=1: L.digat_gemm_launch(C.addressof(g), size, kind, None, C.byref(kernel), _lib.stream_ptr())
    assert call(g, C.sizeof(G.GemmArgs) - 4) == 1 and call(g, kind=2) == 1
    assert L.digat_gemm_launch(None, C.sizeof(G.GemmArgs), 1, None, C.byref(kernel), _lib.stream_ptr()) == 1
    for field, value in (("a0", None), ("M", -1), ("K", 0), ("nseg", 0), ("nsegs", 0), ("nsegs", 4), ("k0", case["K"] + 4)):
        bad = G.fill_args(case, G.fake_pointers(case))
        setattr(bad, field, value)
        assert call(bad) == 1, field
    for field in ("w", "y"):
        bad = G.fill_args(case, G.fake_pointers(case))
        getattr(bad, field)[0] = None
        assert call(bad) == 1, field
    g.M = 0          # nothing to do: no launch, no error
    assert call(g) == 0 and kernel.value == G.kernel_ids()["F32_32"]


ROW_LISTS = sorted(n for n, c in G.CASES.items() if c.get("rows") == "all" and (n.endswith("_rows_all") or n.endswith("_m200")))


@pytest.mark.parametrize("name", ROW_LISTS)
def test_sorted_list_of_all_rows_gives_the_bits_of_the_launch_without(name):
    """Strip and fp16-fp8c kernels.  A bf16x6 launch without a list would move to 64-row tiles: it asks for ragged tiles instead,
    which keeps it on the 128-row kernel (three strips or fewer: no ragged tile either)."""
    case = G.CASES[name]
    twin = {k: v for k, v in case.items() if k != "rows"}
    if case["fmt"] == G.BF16X6:
        twin["ragged"] = 1
    a, b = _launch(name, case), _launch(name, twin)
    assert a["rc"] == b["rc"] == 0 and a["kernel"] == b["kernel"] == G.kernel_ids()[case["kernel"]]
    for s in range(case["nsegs"]):
        ya, yb = a["ys"][s].after(), b["ys"][s].after()
        bits = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[ya.element_size()]
        assert torch.equal(ya.view(bits), yb.view(bits)), (name, s)
        if ya.dtype == torch.float32:
            assert bool(torch.isfinite(ya[1:-1, 4:4 + case["nseg"]]).all()), (name, s)
