"""CPU suite behind tests/test_gemm_fp64_gpu.py: the case table of tests/gemm_fp64_common.py on the launch plan, and its bounds on
float64 emulations.

digat_amd/csrc/digat_gemm_plan.h is built with the host compiler into a small shared object: the layout of GemmArgs is held to the
ctypes mirror, gemm_plan is asked about every case — each must get the kernel it names and must not be refused, and together they
must reach every entry of DIGAT_GEMM_KERNELS, the per-segment launch and the three ragged instantiations in both tile orders, so a
table that stops covering a kernel fails here.  A float32 restatement of every case stays within half of the bound the GPU run is
held to, the decoders read back what encoders of the two reduced output formats write, and on the cases with x3_segs / x1_segs
each bound is shown to separate the product sets it is meant to separate.
"""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import gemm_fp64_common as G
from conftest import REPO

SOURCE = r"""
#include <stddef.h>
#include "digat_amd/csrc/digat_gemm_plan.h"
extern "C" {
void plan(const GemmArgs* g, int kind, int* out) {
    const GemmPlan p = gemm_plan(*g, kind);
    out[0] = p.status; out[1] = p.kernel; out[2] = p.mtiles; out[3] = p.ntiles; out[4] = (int)p.grid; out[5] = (int)p.block;
    out[6] = p.image_format; out[7] = p.ragged; out[8] = (int)gemm_takes_row_list(*g);
}
int kernels(void) {
    int n = 0;
#define COUNT(id, ...) ++n;
    DIGAT_GEMM_KERNELS(COUNT)
    return n;
}
long layout(int i) {
    const long at[] = {(long)sizeof(GemmArgs), %s};
    return i < (int)(sizeof(at) / sizeof(at[0])) ? at[i] : -1;
}
}
"""


@pytest.fixture(scope="module")
def planlib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    tmp = tmp_path_factory.mktemp("gemm_plan")
    src = tmp / "plan.cpp"
    src.write_text(SOURCE % ", ".join(f"(long)offsetof(GemmArgs, {f})" for f in G.FIELDS))
    so = tmp / "libplan.so"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", f"-I{REPO}", str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.layout.restype = C.c_long
    lib.plan.argtypes = [C.POINTER(G.GemmArgs), C.c_int, C.POINTER(C.c_int)]
    return lib


def _plan(lib, case):
    g = G.fill_args(case, G.fake_pointers(case))
    out = (C.c_int * 9)()
    lib.plan(C.byref(g), G.KIND[case.get("kind")], out)
    return dict(zip(("status", "kernel", "mtiles", "ntiles", "grid", "block", "image_format", "ragged", "takes_rows"), out))


def test_ctypes_mirror_has_the_layout_of_gemmargs(planlib):
    assert planlib.layout(0) == C.sizeof(G.GemmArgs)
    for i, f in enumerate(G.FIELDS):
        assert planlib.layout(i + 1) == getattr(G.GemmArgs, f).offset, f
    assert planlib.layout(len(G.FIELDS) + 1) == -1
    # every member of the struct is mirrored: the header's declarations name the same fields in the same order
    text = open(G.PLAN_H).read()
    body = text[text.index("struct GemmArgs {"):text.index("enum { DIGAT_GEMM_RAGGED")]
    body = "\n".join(l.split("//")[0] for l in body.splitlines()[1:])
    names = []
    for decl in body.split(";"):
        for part in decl.split(","):
            words = part.replace("*", " ").replace("[3]", " ").split()
            if words and words[-1] != "}":
                names.append(words[-1])
    assert names == G.FIELDS


def test_every_case_gets_the_kernel_it_names(planlib):
    ids = G.kernel_ids()
    assert planlib.kernels() == len(ids) - 2 == 25
    reached = set()
    for name, case in G.CASES.items():
        p = _plan(planlib, case)
        assert p["status"] == 0, (name, "refused", p)
        assert p["kernel"] == ids[case["kernel"]], (name, G.kernel_name(p["kernel"]))
        assert p["ragged"] == case.get("ragged_plan", 0), (name, p)
        if case.get("fmt") is not None and case["kernel"].startswith(("STRIP", "F16F8C", "SKINNY_SPLIT")):
            assert p["image_format"] == case["fmt"], name
        if case.get("rows"):
            assert p["takes_rows"] == 1, name
        reached.add((case["kernel"], p["ragged"]))
    ragged = {(k, order) for k in ("STRIP_3_F16_FULL", "STRIP_3_F16", "STRIP_3_BF16") for order in (1, 2)}
    assert reached == {(k, 0) for k in ids if k != "NONE"} | ragged
    for name, (case, status) in G.REFUSED.items():
        p = _plan(planlib, case)
        assert p["kernel"] == ids[case["kernel"]], (name, G.kernel_name(p["kernel"]))
        # an image split in another format is refused by the launch, from the library's record of its images, not by the plan
        assert p["status"] == (0 if "image_fmt" in case else status), name


def test_table_holds_the_shapes_the_kernels_change_path_at(planlib):
    """Tile counts 1, 7, 8 and 9 on an fp32 and on a strip kernel; the 320- and 480-workgroup thresholds from the smallest shapes."""
    for prefix in ("f32_32_tiles", "strip_3_f16_64_tiles"):
        tiles = {n: _plan(planlib, G.CASES[f"{prefix}{n}"]) for n in (1, 7, 8, 9)}
        assert {n: p["mtiles"] * p["ntiles"] for n, p in tiles.items()} == {1: 1, 7: 7, 8: 8, 9: 9}
        assert {n: p["grid"] for n, p in tiles.items()} == {1: 8, 7: 8, 8: 8, 9: 16}
    for name in ("skinny_split_f16_2_m1", "skinny_split_bf16_2_m40"):
        assert _plan(planlib, G.CASES[name])["grid"] == 320
    for name in ("skinny_2_wide", "skinny_2_ktail_wide", "skinny_tw_2_wide"):
        assert _plan(planlib, G.CASES[name])["grid"] == 480
    assert len(G.CASES) < 700, "the GPU file runs every case: keep the table small"
    for name, case in G.CASES.items():
        assert case["M"] * case["nseg"] * case["nsegs"] * case["K"] <= 1 << 26, (name, "too large for a fraction of a second")


def _restated(name, case, dtype=np.float32, product=None):
    o = G.draw(name, case)
    ref = G.reference(case, o)
    got = G.reference(case, o, dtype, product)
    return o, ref, got


def _store(case, s, v):
    """What the kernel's output formats make of the fp32 value v: fp32, bf16 bits or e4m3 rows."""
    v = np.asarray(v, dtype=np.float32)
    if G.seg_mask(case, "fp8_segs", s):
        return G.encode_e4m3_rows(v, case["nseg"])
    return G.encode_bf16(v) if G.seg_mask(case, "bf16_segs", s) else v


@pytest.mark.parametrize("family", sorted({c["kernel"] for c in G.CASES.values()}))
def test_float32_restatement_meets_half_the_bound(family):
    """numpy in float32, the order of operations of the reference: every case within half of what the GPU run is held to (a case
    that is not has inputs the bound does not fit: change them, not the bound).  Stored through the encoders of the reduced output
    formats, the same values pass the whole check the GPU run goes through — which reads them back with the decoders."""
    worst = 0.0
    for name, case in G.CASES.items():
        if case["kernel"] != family or case.get("big"):
            continue
        o, ref, got = _restated(name, case)
        tol = G.tolerances(case, o, ref, products="full")
        rows = np.ones(case["M"], dtype=bool)
        for s, ((pre, want), (_, v)) in enumerate(zip(ref, got)):
            plain = dict(case, bf16_segs=0, fp8_segs=0)
            worst = max(worst, G.check_segment(plain, s, v, want, 0.5 * tol[s], rows, f"{name} segment {s} in float32"))
            G.check_segment(case, s, _store(case, s, v), want, tol[s], rows, f"{name} segment {s} stored")
    print(f"[{family}] float32 restatement: worst err / (bound / 2) {worst:.3f}")


def test_decoders_invert_the_formats():
    codes = np.arange(256, dtype=np.uint8)
    import torch
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(want), np.isnan(G._E4M3)) and np.array_equal(want[~np.isnan(want)], G._E4M3[~np.isnan(want)])
    v = np.random.default_rng(3).standard_normal((5, 160)).astype(np.float32)
    rows = G.encode_e4m3_rows(v, 160)
    assert rows.shape == (5, 168)
    dec, scales = G.decode_e4m3_rows(rows, 160)
    assert np.array_equal(scales.astype(np.float32), (np.abs(v).reshape(5, 2, 80).max(-1) * np.float32(1 / 448)).astype(np.float32))
    assert (np.abs(dec - v) <= 2.0 ** -4 * np.abs(v) + 2.0 ** -10 * np.repeat(scales, 80, axis=1)).all()
    b = torch.from_numpy(v).to(torch.bfloat16)
    assert np.array_equal(G.encode_bf16(v).view(np.int16), b.view(torch.int16).numpy())
    assert np.array_equal(G.decode_bf16(G.encode_bf16(v)), b.to(torch.float64).numpy())


REDUCED_CASES = sorted(n for n, c in G.CASES.items() if c.get("x3_segs") or c.get("x1_segs"))


def _fails(case, s, got, want, tol, rows):
    try:
        G.check_segment(case, s, got, want, tol, rows, "")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", REDUCED_CASES)
def test_bounds_separate_the_product_sets(name):
    """Per segment with x3_segs / x1_segs: the float64 emulation of the reduced product (the pieces the code makes, only the
    products it keeps) passes its own bound and fails the one of the set above it: x3 fails the full-precision tolerance, x1 fails
    x3's.  fp16x3 forms its three products with x3_segs set or clear: its x3 IS its full product, and is held to that."""
    case = G.CASES[name]
    fmt = case["fmt"]
    plain = dict(case, bf16_segs=0, fp8_segs=0)
    o = G.draw(name, case)
    ref = G.reference(plain, o)
    rows = np.ones(case["M"], dtype=bool)
    emu = {ps: G.reference(plain, o, np.float64, lambda s, A, w, ps=ps: G.emulated_product(fmt, ps, A, w)) for ps in ("full", "x3", "x1")}
    tol = {ps: G.tolerances(plain, o, ref, products=ps) for ps in ("full", "x3", "x1")}
    seen = set()
    for s in range(case["nsegs"]):
        ps = G.products_of(case, s)
        want = ref[s][1]
        r = G.check_segment(plain, s, emu[ps][s][1], want, tol[ps][s], rows, f"{name} segment {s}: the {ps} emulation against its own bound")
        print(f"[{name}] segment {s} {ps}: emulation at {r:.3f} of its bound")
        seen.add(ps)
        if ps == "x3" and fmt == G.BF16X6:
            assert _fails(plain, s, emu["x3"][s][1], want, tol["full"][s], rows), "three products pass for six"
        if ps == "x3" and fmt == G.F16X3:
            assert np.array_equal(emu["x3"][s][1], emu["full"][s][1])
        if ps == "x1":
            assert _fails(plain, s, emu["x1"][s][1], want, tol["x3"][s], rows), "one product passes for three"
            assert _fails(plain, s, emu["x1"][s][1], want, tol["full"][s], rows)
    assert seen - {"full"}


def test_reduced_cases_cover_both_formats_and_both_sets():
    kinds = {(G.CASES[n]["fmt"], ps) for n in REDUCED_CASES for s in range(G.CASES[n]["nsegs"]) for ps in [G.products_of(G.CASES[n], s)]}
    assert {(f, ps) for f in (G.BF16X6, G.F16X3) for ps in ("x3", "x1")} <= kinds
