"""GPU suite: the training primitives of the C ABI and the two context pairs, each ALONE, against float64 references.

The whole-model goldens (test_hip_training.py) hold a training step to the reference at two shapes; they cannot say which kernel is
wrong and they reach little of the shape-dependent dispatch of csrc/digat_train.inc / digat_train_abi.inc.  Here every primitive is
called on its own — through the ctypes table or through the ``torch.autograd.Function`` that wraps it in digat_amd/training.py — and
compared with a float64 CPU computation (numpy, or torch autograd through ``.double()`` copies of the same float32 inputs; the
``oracle.digat_oracle`` functions where one exists).  No reference comes from the library.  Every device output buffer is pre-filled
with NaN (with a known value when the call accumulates): an element the kernel never writes fails the comparison.

Tolerances are the existing ones: ``close()`` below has the form of test_hip_training.close (rtol on max(|want|, 5 % of the tensor's
scale) + atol); GEMM-like sums use test_linear_mfma_f32's rule rtol = 1e-5, atol = 2e-6 sqrt(reduced dimension); composed
forward/backward pairs use test_hip_training's 2e-4 / 2e-6.
"""
import math

import numpy as np
import pytest
import torch

from oracle import digat_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, 1, 2, 3
NAN = float("nan")


def close(got, want, what, rtol=2e-4, atol=2e-6):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite ({int((~np.isfinite(got)).sum())} of {got.size}, first at " \
                                   f"{np.unravel_index(int(np.argmax(~np.isfinite(got))), got.shape)})"
    if got.size == 0:
        return
    scale = max(float(np.abs(want).max()), 1e-12)
    err = np.abs(got - want)
    tol = atol + rtol * np.maximum(np.abs(want), 0.05 * scale)
    if (err > tol).any():
        idx = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int((err > tol).sum())}/{err.size} off, max|diff|={err.max():.3e} (scale {scale:.3e}) at {idx}: "
                             f"got {got[idx]:.7g} want {want[idx]:.7g}")


def _lib():
    from digat_amd import _lib as m
    return m


def _L():
    return _lib().lib()


def _S():
    return _lib().stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan_like(shape):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=DEV)


def poisoned_bytes(nbytes):
    """A scratch buffer of exactly ``nbytes`` (at least one) bytes of 0xFF: every float read before it is written is a NaN."""
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=DEV)


def place(a, layout):
    """Device copy of the [M, C] matrix ``a`` as the kernels may meet it; returns (keep-alive tensor, pointer, row stride).
    dense: contiguous; wide: a column block of a wider matrix (row stride 2 C + 8, as the context backwards pass [B, 2 d] and
    [B, N d] operands; the other columns hold NaN); odd: row stride C + 1; shifted: contiguous, one float past a 16-byte boundary."""
    M, C = a.shape
    if layout == "dense":
        t = nan_like((max(M, 1), C))
        t[:M] = dev(a)
        return t, t.data_ptr(), C
    if layout == "wide":
        ld = 2 * C + 8
        t = nan_like((max(M, 1), ld))
        t[:M, 4:4 + C] = dev(a)
        return t, t.data_ptr() + 16, ld
    if layout == "odd":
        t = nan_like((max(M, 1), C + 1))
        t[:M, :C] = dev(a)
        return t, t.data_ptr(), C + 1
    assert layout == "shifted"
    t = nan_like((max(M, 1) * C + 1,))
    t[1:1 + M * C] = dev(a).reshape(-1)
    return t, t.data_ptr() + 4, C


# ======================================================================================================================
# 1. digat_linear_bwd_weight: dW = dy^T x, db = colsum(dy)
# ======================================================================================================================
def tn_plan(M, No, Ni, vec):
    """csrc/digat_train.inc restated: (kernel, slices, rows per slice) of digat_linear_bwd_weight.  ``tn_slices`` does not know
    ``vec``: from 2 048 rows on it counts 160 x 160 tiles even when the scalar 80 x 80 kernel then runs."""
    cd = lambda a, b: (a + b - 1) // b
    if M >= 2048:
        slices = max(1, min(cd(1024, cd(No, 160) * cd(Ni, 160)), cd(M, 256), 64))
    else:
        slices = min(max(1, min(max(cd(M, 256), cd(512, cd(No, 80) * cd(Ni, 80))), cd(M, 32))), 64)
    kernel = "bf16x6" if (vec and M >= 2048) else ("vector" if vec else "scalar")
    mper = cd(cd(M, slices), 32) * 32 or 32
    return kernel, slices, mper


def is_vec(No, Ni, lay_dy, lay_x):
    def ld_ok(cols, lay):
        return {"dense": cols, "wide": 2 * cols + 8, "odd": cols + 1, "shifted": cols}[lay] % 4 == 0 and lay != "shifted"
    return No % 4 == 0 and Ni % 4 == 0 and ld_ok(No, lay_dy) and ld_ok(Ni, lay_x)


# id -> (M, No, Ni, layout of dy, layout of x, db wanted, accumulate)
TN_CASES = {
    "scalar-No%4-37x17x9": (37, 17, 9, "dense", "dense", True, 0),
    "scalar-ldx%4-strided-view": (70, 16, 12, "dense", "odd", True, 1),
    "scalar-lddy%4-strided-view": (70, 16, 12, "odd", "dense", False, 0),
    "scalar-pointer-one-float-off": (320, 400, 400, "dense", "shifted", True, 0),
    "vector-320x400x800": (320, 400, 800, "dense", "dense", True, 0),
    "vector-ragged80-333x84x164-wide-rows-accumulate": (333, 84, 164, "wide", "wide", True, 1),
    "vector-31x80x80-no-db": (31, 80, 80, "dense", "dense", False, 0),
    "vector-1x4x4": (1, 4, 4, "dense", "dense", True, 0),
    "vector-2047x400x400-empty-trailing-slices": (2047, 400, 400, "dense", "dense", True, 0),
    "bf16x6-2048x400x400": (2048, 400, 400, "dense", "dense", True, 0),
    "bf16x6-ragged160-2049x164x324-wide-rows-accumulate": (2049, 164, 324, "wide", "wide", True, 1),
    "bf16x6-2680x400x400-no-db-accumulate": (2680, 400, 400, "dense", "dense", False, 1),
    "bf16x6-20000x80x400-64-slices": (20000, 80, 400, "dense", "dense", True, 0),
    "scalar-160-tile-slices-2100x18x40": (2100, 18, 40, "dense", "dense", True, 0),
    "scalar-160-tile-slices-2100x80x40-pointer-off-accumulate": (2100, 80, 40, "shifted", "dense", True, 1),
}


def test_weight_gradient_cases_cover_every_kernel_and_slice_count():
    """The parametrisation of the test below, held to the dispatch rule restated in ``tn_plan``: all three kernels (float4-staged
    ``gemm_tn_kernel``, scalar-staged ``gemm_tn_kernel``, ``gemm_tn_bf16x6_kernel``), the scalar kernel on 160-tile slices, slice
    counts of 1, in between and 64, a split whose trailing slices are empty, db present and NULL, accumulate 0 and 1, padded rows.
    (That ``tn_plan`` IS the library's rule is asserted per case through digat_linear_bwd_weight_workspace.)"""
    plans = {k: tn_plan(M, No, Ni, is_vec(No, Ni, ly, lx)) + (M, ly, lx, db, acc) for k, (M, No, Ni, ly, lx, db, acc) in TN_CASES.items()}
    kernels = {p[0] for p in plans.values()}
    assert kernels == {"vector", "scalar", "bf16x6"}, kernels
    for kern in kernels:
        assert {p[7] for p in plans.values() if p[0] == kern} == {0, 1}, f"{kern}: accumulate 0 and 1"
        assert {p[6] for p in plans.values() if p[0] == kern} == {True, False}, f"{kern}: db present and NULL"
    slices = {p[1] for p in plans.values()}
    assert 1 in slices and 64 in slices and any(1 < s_ < 64 for s_ in slices), slices
    assert any(p[0] == "scalar" and p[3] >= 2048 for p in plans.values()), "the scalar kernel on the 160-tile slice rule"
    assert any(p[2] * (p[1] - 1) >= p[3] for p in plans.values()), "a split with empty trailing slices (mper rounded up to 32)"
    assert any("wide" in (p[4], p[5]) for p in plans.values()) and any(p[5] == "odd" for p in plans.values()) \
        and any("shifted" in (p[4], p[5]) for p in plans.values())
    for k, p in plans.items():
        assert k.startswith(p[0]), (k, p[0])          # the ids name the kernel that runs


def _run_bwd_weight(dy, x, lay_dy, lay_x, want_db, accumulate, base_W, base_b, ws_short=0):
    """-> (rc, dW, db or None) of one digat_linear_bwd_weight call on device copies in the given layouts."""
    L = _L()
    M, No = dy.shape
    Ni = x.shape[1]
    keep_y, py, lddy = place(dy, lay_dy)
    keep_x, px, ldx = place(x, lay_x)
    dW = dev(base_W) if accumulate else nan_like((No, Ni))
    db = (dev(base_b) if accumulate else nan_like((No,))) if want_db else None
    nb = L.digat_linear_bwd_weight_workspace(M, No, Ni)
    ws = poisoned_bytes(nb)
    rc = L.digat_linear_bwd_weight(py, lddy, px, ldx, dW.data_ptr(), db.data_ptr() if want_db else None, M, No, Ni, accumulate,
                                   ws.data_ptr(), nb - ws_short, _S())
    torch.cuda.synchronize()
    del keep_y, keep_x
    return rc, dW, db


@pytest.mark.parametrize("case", list(TN_CASES), ids=list(TN_CASES))
def test_linear_bwd_weight_against_fp64(case):
    """digat_linear_bwd_weight alone against dy64^T x64 and dy64.sum(0): every staging path, the M split (ragged last slice, empty
    trailing slices, 1 .. 64 slices), the bias gradient from input-column block 0, ``accumulate`` in the slice reduction, padded
    rows whose padding holds NaN.  Tolerance: test_linear_mfma_f32's rule on the reduced dimension M.  The bf16x6 product must
    also be fp32-grade as test_linear_bf16x6_is_fp32_grade asks: mean error <= 1.5 x that of the fp32 kernel on the same data
    (reached through a pointer one float off alignment)."""
    M, No, Ni, lay_dy, lay_x, want_db, accumulate = TN_CASES[case]
    kernel, slices, _ = tn_plan(M, No, Ni, is_vec(No, Ni, lay_dy, lay_x))
    assert _L().digat_linear_bwd_weight_workspace(M, No, Ni) == slices * (No * Ni + No) * 4, "tn_plan is no longer the library's slice rule"
    rng = np.random.default_rng(M * 7 + No * 3 + Ni)
    dy = rng.standard_normal((M, No)).astype(np.float32)
    x = rng.standard_normal((M, Ni)).astype(np.float32)
    base_W = rng.standard_normal((No, Ni)).astype(np.float32) * 3
    base_b = rng.standard_normal(No).astype(np.float32) * 3
    want_W = dy.astype(np.float64).T @ x.astype(np.float64) + (base_W if accumulate else 0.0)
    want_b = dy.astype(np.float64).sum(0) + (base_b if accumulate else 0.0)
    rc, dW, db = _run_bwd_weight(dy, x, lay_dy, lay_x, want_db, accumulate, base_W, base_b)
    assert rc == OK
    tol = dict(rtol=1e-5, atol=2e-6 * math.sqrt(M))
    close(dW, want_W.astype(np.float32), f"{case}: dW ({kernel}, {slices} slices)", **tol)
    if want_db:
        close(db, want_b.astype(np.float32), f"{case}: db ({kernel}, {slices} slices)", **tol)
    if kernel == "bf16x6":
        rc, dW32, _ = _run_bwd_weight(dy, x, "shifted", lay_x, False, accumulate, base_W, base_b)
        assert rc == OK
        close(dW32, want_W.astype(np.float32), f"{case}: dW (fp32 kernel on the same data)", **tol)
        e6 = np.abs(dW.cpu().numpy().astype(np.float64) - want_W).mean()
        e32 = np.abs(dW32.cpu().numpy().astype(np.float64) - want_W).mean()
        print(f"\n[{case}] mean |err|: bf16x6 {e6:.3e}, fp32 {e32:.3e}")
        assert e6 <= 1.5 * e32 + 1e-9, (e6, e32)


def test_linear_bwd_weight_with_bf16_training_precision():
    """digat_set_train_precision(1): the 2 680-row weight gradient as ONE bf16 product — held to what
    test_bf16_training_precision_at_production_shapes asks of a gradient (norm within 5 %, cosine > 0.98 of the fp64 one); the
    single product must really run, and the default must come back bit for bit."""
    M, No, Ni = 2680, 400, 400
    rng = np.random.default_rng(2680)
    dy = rng.standard_normal((M, No)).astype(np.float32)
    x = rng.standard_normal((M, Ni)).astype(np.float32)
    want = (dy.astype(np.float64).T @ x.astype(np.float64)).reshape(-1)
    _, base, base_b = _run_bwd_weight(dy, x, "dense", "dense", True, 0, None, None)
    prev = _L().digat_set_train_precision(1)
    try:
        rc, dW, db = _run_bwd_weight(dy, x, "dense", "dense", True, 0, None, None)
    finally:
        _L().digat_set_train_precision(prev)
    assert rc == OK and prev == 0
    assert torch.isfinite(dW).all() and not torch.equal(dW, base), "the one-product kernel did not run"
    g = dW.cpu().numpy().astype(np.float64).reshape(-1)
    assert abs(np.linalg.norm(g) - np.linalg.norm(want)) <= 0.05 * np.linalg.norm(want)
    cos = float((g * want).sum() / (np.linalg.norm(g) * np.linalg.norm(want)))
    print(f"\n[bf16 weight gradient] 1 - cos = {1 - cos:.2e}")
    assert cos > 0.98, cos
    close(db, dy.astype(np.float64).sum(0).astype(np.float32), "db under bf16 precision (an fp32 sum of the unsplit values)", rtol=1e-5,
          atol=2e-6 * math.sqrt(M))
    _, again, again_b = _run_bwd_weight(dy, x, "dense", "dense", True, 0, None, None)
    assert torch.equal(again, base) and torch.equal(again_b, base_b)


@pytest.mark.parametrize("want_db", [True, False], ids=["db", "db-NULL"])
def test_linear_bwd_weight_of_no_rows_and_short_workspace(want_db):
    """M = 0 (``mper > 0 ? mper : 32``): zeros with accumulate 0, the destination unchanged with accumulate 1, DIGAT_OK; a workspace
    one byte short is DIGAT_ERR_WORKSPACE and nothing is launched."""
    No, Ni = 20, 36
    rng = np.random.default_rng(0)
    base_W, base_b = rng.standard_normal((No, Ni)).astype(np.float32), rng.standard_normal(No).astype(np.float32)
    empty_y, empty_x = np.zeros((0, No), np.float32), np.zeros((0, Ni), np.float32)
    for lay in ("dense", "odd"):                  # (vector and scalar staging)
        rc, dW, db = _run_bwd_weight(empty_y, empty_x, lay, "dense", want_db, 0, base_W, base_b)
        assert rc == OK and torch.equal(dW.cpu(), torch.zeros(No, Ni)) and (db is None or torch.equal(db.cpu(), torch.zeros(No)))
        rc, dW, db = _run_bwd_weight(empty_y, empty_x, lay, "dense", want_db, 1, base_W, base_b)
        assert rc == OK and torch.equal(dW.cpu(), torch.from_numpy(base_W)) and (db is None or torch.equal(db.cpu(), torch.from_numpy(base_b)))
    for M in (0, 70, 2100):
        dy, x = rng.standard_normal((M, No)).astype(np.float32), rng.standard_normal((M, Ni)).astype(np.float32)
        rc, dW, db = _run_bwd_weight(dy, x, "dense", "dense", want_db, 0, base_W, base_b, ws_short=1)
        assert rc == ERR_WORKSPACE and torch.isnan(dW).all() and (db is None or torch.isnan(db).all())


# ======================================================================================================================
# 2. digat_linear_bwd_input / digat_linear_bwd_input_x3: dx = dy W
# ======================================================================================================================
def _bwd_input_data(M, N, K, seed):
    rng = np.random.default_rng(seed)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / math.sqrt(N)).astype(np.float32)
    base = rng.standard_normal((M, K)).astype(np.float32)
    return dy, w, base, dy.astype(np.float64) @ w.astype(np.float64)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,N,K", [(60, 64, 64), (536, 400, 400), (1024, 400, 400), (4100, 400, 400), (2500, 128, 192), (9000, 36, 80),
                                   (33, 8, 17)])
def test_linear_bwd_input_fp32_against_fp64(M, N, K, accumulate):
    """digat_linear_bwd_input (the fp32 MFMA kernel reading W as [K_red = N, N_out = K]) at test_linear_mfma_f32's ragged shapes
    (reduced and output widths swapped where the reduced one would not be a multiple of 4), ``accumulate`` 0 and 1."""
    dy, w, base, prod = _bwd_input_data(M, N, K, M + N + K)
    dx = dev(base) if accumulate else nan_like((M, K))
    yd, wd = dev(dy), dev(w)
    assert _L().digat_linear_bwd_input(yd.data_ptr(), N, wd.data_ptr(), dx.data_ptr(), K, M, N, K, accumulate, _S()) == OK
    torch.cuda.synchronize()
    close(dx, (prod + (base if accumulate else 0.0)).astype(np.float32), f"dx {M}x{N}x{K} acc={accumulate}", rtol=1e-5, atol=2e-6 * math.sqrt(N))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N,K,x3_from_2048", [(400, 400, True), (40, 80, True), (36, 80, False), (80, 40, False)],
                         ids=["400x400-x3", "40x80-x3", "36x80-N%8-fp32", "80x40-K%80-fp32"])
@pytest.mark.parametrize("M", [2047, 2048, 4100])
def test_linear_bwd_input_through_the_python_dispatch_across_the_x3_boundary(M, N, K, x3_from_2048, accumulate):
    """training._linear_bwd_input: the Python rule (``_x3_ok``) picks digat_linear_bwd_input_x3 (bf16x6) from 2 048 rows on when the
    shape allows it and the C entry accepts exactly those shapes; below, and for the other shapes, the fp32 kernel.  Same data,
    same fp64 product, same tolerance either way."""
    from digat_amd import training
    assert training._x3_ok(M, K, N) == (x3_from_2048 and M >= 2048)
    dy, w, base, prod = _bwd_input_data(M, N, K, M * 3 + N + K)
    dx = dev(base) if accumulate else nan_like((M, K))
    yd, wd = dev(dy), dev(w)
    training._linear_bwd_input(yd.data_ptr(), wd, dx.data_ptr(), M, N, K, accumulate, torch.device(DEV), "dx")
    torch.cuda.synchronize()
    close(dx, (prod + (base if accumulate else 0.0)).astype(np.float32), f"dx {M}x{N}x{K} acc={accumulate}", rtol=1e-5, atol=2e-6 * math.sqrt(N))


def test_linear_bwd_input_rejects_the_documented_shapes():
    """DIGAT_ERR_SHAPE, and nothing written: N % 4 for the fp32 entry; M < 2048, K % 80, N % 8, N < 32 for the bf16x6 entry."""
    L = _L()
    buf = torch.zeros(4100 * 400, device=DEV)
    w = torch.zeros(400 * 400, device=DEV)
    out = nan_like((4100 * 400,))
    ws = poisoned_bytes(L.digat_split_weights_bytes(400, 400))
    assert L.digat_linear_bwd_input(buf.data_ptr(), 8, w.data_ptr(), out.data_ptr(), 16, 40, 6, 16, 0, _S()) == ERR_SHAPE
    for what, (M, N, K) in {"M < 2048": (2047, 400, 400), "K % 80": (2048, 400, 84), "N % 8": (2048, 36, 80), "N < 32": (2048, 24, 80)}.items():
        assert L.digat_linear_bwd_input_x3(buf.data_ptr(), N, w.data_ptr(), out.data_ptr(), K, M, N, K, 0, ws.data_ptr(), _S()) == ERR_SHAPE, what
    assert L.digat_linear_bwd_input_x3(buf.data_ptr(), 400, w.data_ptr(), out.data_ptr(), 400, 2048, 400, 400, 0, None, _S()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ======================================================================================================================
# 3. element-wise and reduction primitives
# ======================================================================================================================
def sum_tol(M, rms=1.0):
    """Tolerance of a plain fp32 sum of M terms of the given rms, whatever its order: rtol = 1e-6 on the result plus
    atol = 2^-23 M rms.  Adding the terms one after the other is the worst order: addition k rounds to half an ulp of a partial sum
    of size ~sqrt(k) rms (an error of rms 2^-23 sqrt(k) rms / sqrt(12)), M of them add up to 2^-23 M rms / sqrt(24) rms — the bound
    is five times that, and still 1 / (2^-23 M) ~ 1 700 times smaller (M = 5 000) than a dropped or doubled row."""
    return dict(rtol=1e-6, atol=2.0 ** -23 * M * rms)


@pytest.mark.parametrize("M", [0, 1, 513, 5000])
def test_colsum_against_fp64(M):
    """digat_colsum, N in {1, 63, 64, 65, 400} (one workgroup per 64 columns: below, at and past the edge), rows of stride > N whose
    padding holds NaN, ``accumulate`` 0 and 1, no rows at all.  Tolerance ``sum_tol``: rtol = 1e-6 and atol = 2^-23 M rms(terms)."""
    L = _L()
    rng = np.random.default_rng(M)
    for N in (1, 63, 64, 65, 400):
        for accumulate, ld in ((0, N), (1, N + 3)):
            x = rng.standard_normal((M, N)).astype(np.float32)
            base = rng.standard_normal(N).astype(np.float32)
            xd = nan_like((max(M, 1), ld))
            xd[:M, :N] = dev(x)
            out = dev(base) if accumulate else nan_like((N,))
            assert L.digat_colsum(xd.data_ptr(), ld, out.data_ptr(), M, N, accumulate, _S()) == OK
            torch.cuda.synchronize()
            want = x.astype(np.float64).sum(0) + (base if accumulate else 0.0)
            close(out, want.astype(np.float32), f"colsum {M}x{N} ld={ld} acc={accumulate}", **sum_tol(M))


@pytest.mark.parametrize("B,n,d", [(3, 10, 400), (5, 67, 36), (1, 1, 4), (7, 128, 37)])
def test_sum_nodes_against_fp64(B, n, d):
    """digat_sum_nodes: dr[b] = sum_j dP[b, j], n terms in node order (``sum_tol``).  B = 0 writes nothing."""
    L = _L()
    rng = np.random.default_rng(B + n + d)
    dP = rng.standard_normal((B, n, d)).astype(np.float32)
    pd, dr = dev(dP), nan_like((B, d))
    assert L.digat_sum_nodes(pd.data_ptr(), dr.data_ptr(), B, n, d, _S()) == OK
    torch.cuda.synchronize()
    untouched = nan_like((B, d))
    assert L.digat_sum_nodes(pd.data_ptr(), untouched.data_ptr(), 0, n, d, _S()) == OK
    torch.cuda.synchronize()
    assert torch.isnan(untouched).all()
    close(dr, dP.astype(np.float64).sum(1).astype(np.float32), f"sum_nodes {B}x{n}x{d}", **sum_tol(n))


GATE_ATOL = 2.0 ** -22


@pytest.mark.parametrize("B,N,d", [(7, 10, 37), (320, 3, 400), (1, 1, 1)])
def test_gate_forward_and_backward_against_fp64(B, N, d):
    """digat_gate_fwd / digat_gate_bwd with l = node 0 of X [B, N, d] (``ldl`` = N d, the way the news context passes it), z holding
    +-40 so that sigmoid saturates (the gradient there must be 0 or tiny, never NaN), B d neither a multiple of 4 nor of 256.
    Tolerance: rtol = 1e-6 on the products, plus an absolute term for the sigmoid: s = 1 / (1 + expf(-z)) carries expf's <= 2 ulp
    (x e / (1 + e)^2 <= 1/4), the rounding of 1 + e and of the division — under 2.5 x 2^-24 absolute — and 1 - s one rounding more:
    atol = 2^-22 x the magnitude of what multiplies s (max |l|, |g| forward; max |dout| for dl, dg; max |dout (l - g)| for dz)."""
    L = _L()
    rng = np.random.default_rng(B * 100 + d)
    X = rng.standard_normal((B, N, d)).astype(np.float32)
    z = (rng.standard_normal((B, d)) * 2).astype(np.float32)
    z.reshape(-1)[::5] = 40.0
    z.reshape(-1)[1::7] = -40.0
    g, dout = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
    Xd, zd, gd, dd = dev(X), dev(z), dev(g), dev(dout)
    out, dz, dl, dg = (nan_like((B, d)) for _ in range(4))
    assert L.digat_gate_fwd(zd.data_ptr(), Xd.data_ptr(), N * d, gd.data_ptr(), out.data_ptr(), B, d, _S()) == OK
    assert L.digat_gate_bwd(dd.data_ptr(), zd.data_ptr(), Xd.data_ptr(), N * d, gd.data_ptr(), dz.data_ptr(), dl.data_ptr(), dg.data_ptr(), B, d, _S()) == OK
    torch.cuda.synchronize()
    l64, z64, g64, do64 = X[:, 0].astype(np.float64), z.astype(np.float64), g.astype(np.float64), dout.astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-z64))
    amp = max(np.abs(l64).max(), np.abs(g64).max())
    close(out, s * l64 + (1 - s) * g64, "gate out", rtol=1e-6, atol=GATE_ATOL * amp)
    close(dl, do64 * s, "gate dl", rtol=1e-6, atol=GATE_ATOL * np.abs(do64).max())
    close(dg, do64 * (1 - s), "gate dg", rtol=1e-6, atol=GATE_ATOL * np.abs(do64).max())
    close(dz, do64 * (l64 - g64) * s * (1 - s), "gate dz", rtol=1e-6, atol=GATE_ATOL * np.abs(do64 * (l64 - g64)).max())
    sat = np.abs(z) == 40.0
    assert sat.any() and float(np.abs(dz.cpu().numpy()[sat]).max()) <= 1e-15 * 40, "a saturated gate passes no gradient to z"
    # B = 0: nothing to do, nothing written
    assert L.digat_gate_fwd(zd.data_ptr(), Xd.data_ptr(), N * d, gd.data_ptr(), out.data_ptr(), 0, d, _S()) == OK
    assert L.digat_gate_bwd(dd.data_ptr(), zd.data_ptr(), Xd.data_ptr(), N * d, gd.data_ptr(), dz.data_ptr(), dl.data_ptr(), dg.data_ptr(), 0, d, _S()) == OK


@pytest.mark.parametrize("n", [0, 1, 1003, 70001])
def test_relu_residual_and_dropout_backward_are_exact(n):
    """digat_relu_res_fwd (relu(y) + t: one rounding), digat_relu_mask (dout [y > 0]: a selection) and digat_dropout_fwd / _bwd
    (x keep x fp32(1 / (1 - p)): one rounding) against float64 at rtol = 1e-6, atol = 0; the selections exactly.  y holds 0.0 and
    -0.0: the gradient at 0 is 0, as torch's.  The keep bytes are the ones ``oracle.hash_dropout_keep`` restates.  Sizes that are
    no multiple of 4 or 256, and n = 0 (nothing written)."""
    L = _L()
    rng = np.random.default_rng(n)
    y, t, dout = (rng.standard_normal(n + 1).astype(np.float32) for _ in range(3))
    y[::3] = 0.0
    y[1::9] = -0.0
    yd, td, dd = dev(y), dev(t), dev(dout)
    out, dy, dropped, dx = (nan_like((n + 1,)) for _ in range(4))
    keep = torch.full((n + 1,), 7, dtype=torch.uint8, device=DEV)
    p, seed = 0.2, 31337 + n
    assert L.digat_relu_res_fwd(yd.data_ptr(), td.data_ptr(), out.data_ptr(), n, _S()) == OK
    assert L.digat_relu_mask(dd.data_ptr(), yd.data_ptr(), dy.data_ptr(), n, _S()) == OK
    assert L.digat_dropout_fwd(yd.data_ptr(), dropped.data_ptr(), keep.data_ptr(), n, p, seed, _S()) == OK
    assert L.digat_dropout_bwd(dd.data_ptr(), keep.data_ptr(), dx.data_ptr(), n, p, _S()) == OK
    torch.cuda.synchronize()
    for buf in (out, dy, dropped, dx):
        assert torch.isnan(buf[n:]).all(), "written past n"
    assert int(keep[n]) == 7
    y64, t64, do64 = (a[:n].astype(np.float64) for a in (y, t, dout))
    close(out[:n], np.maximum(y64, 0.0) + t64, "relu(y) + t", rtol=1e-6, atol=0.0)
    assert np.array_equal(dy[:n].cpu().numpy(), np.where(y[:n] > 0, dout[:n], np.float32(0.0)))
    want_keep = O.hash_dropout_keep(n, p, seed)
    assert np.array_equal(keep[:n].cpu().numpy() != 0, want_keep), "keep bytes differ from oracle.hash_dropout_keep"
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    close(dropped[:n], np.where(want_keep, y64 * scale, 0.0), "dropout forward", rtol=1e-6, atol=0.0)
    close(dx[:n], np.where(want_keep, do64 * scale, 0.0), "dropout backward", rtol=1e-6, atol=0.0)
    if n > 1000:
        assert 0.75 < want_keep.mean() < 0.85


# ======================================================================================================================
# 4. pooling backwards
# ======================================================================================================================
def _pool_rows(n, d, seed):
    """Four rows: a random mask (node 0 live), a row fully masked, a row with only node 0 live, a random mask again (the row whose
    masked nodes get NaN features on the device)."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(4, n, d, generator=g)
    kq = torch.randn(4, d, generator=g) * 2
    dout = torch.randn(4, d, generator=g)
    mask = torch.rand(4, n, generator=g) < 0.6
    mask[:, 0] = True
    mask[1] = False
    mask[2, 1:] = False
    return feat, kq, dout, mask


def _pool_reference(feat, kq, dout, mask):
    """oracle.scaled_dot_attention in float64 with identity key / query projections: the folded query kq IS the query."""
    d = feat.shape[2]
    eye = torch.eye(d, dtype=torch.float64)
    p = {"a.K.weight": eye, "a.Q.weight": eye, "a.Q.bias": torch.zeros(d, dtype=torch.float64)}
    f64, k64 = feat.double().requires_grad_(True), kq.double().requires_grad_(True)
    out = O.scaled_dot_attention(p, "a", f64, k64, mask)
    (out * dout.double()).sum().backward()
    return out.detach(), f64.grad, k64.grad


@pytest.mark.parametrize("n,d", [(1, 4), (10, 400), (67, 64), (68, 512), (82, 800), (128, 32)])
def test_attn_pool_backward_against_oracle_autograd(n, d):
    """training.AttnPool (digat_attn_pool_fwd / digat_attn_pool_bwd): out, dfeat and dkq against float64 autograd through the oracle's
    ScaledDotProductAttention.  digat_attn_pool_fwd always launches attn_pool_kernel, the two-pass kernel, at every size — also at
    those below 68 nodes and 512 channels, where inference's launch_pool takes attn_pool_resident_kernel; the resident kernels are
    held to fp64 alone through digat_pool_fwd in tests/test_hip_ctx_fp64.py.
    Rows: ordinary, fully masked (uniform weights, no gradient to the scores), only node 0 live, and a row whose masked nodes hold
    NaN on the device — a masked node's weight is exactly 0 and its row must not enter any sum (the forward's rule, round 6):
    dfeat there is exactly 0 and nothing turns NaN.  Then ``accumulate_dfeat`` = 1 through the raw entry."""
    from digat_amd import training
    feat, kq, dout, mask = _pool_rows(n, d, n * 1000 + d)
    want_out, want_df, want_dk = _pool_reference(feat, kq, dout, mask)
    poisoned = feat.clone()
    poisoned[3][~mask[3]] = NAN
    fd, kd = poisoned.to(DEV).requires_grad_(True), kq.to(DEV).requires_grad_(True)
    md = mask.to(torch.uint8).to(DEV)
    out = training.AttnPool.apply(fd, kd, md)
    (out * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    close(out, want_out, f"pool n={n} d={d} out", rtol=2e-5, atol=2e-5)
    close(fd.grad, want_df, f"pool n={n} d={d} dfeat")
    close(kd.grad, want_dk, f"pool n={n} d={d} dkq")
    assert float(fd.grad[3][~mask[3]].abs().sum()) == 0.0 and float(fd.grad[2, 1:].abs().sum()) == 0.0, "masked nodes receive exactly no gradient"
    close(fd.grad[1], (dout[1].double() / n).expand(n, d), "fully masked row: dfeat = dout / n")
    assert float(kd.grad[1].abs().max()) == 0.0
    # accumulate_dfeat through the raw entry, dfeat rows of stride > n d
    L = _L()
    alpha = nan_like((4, n))
    o2 = nan_like((4, d))
    f0 = feat.to(DEV)
    assert L.digat_attn_pool_fwd(f0.data_ptr(), n * d, kd.data_ptr(), md.data_ptr(), o2.data_ptr(), alpha.data_ptr(), 4, n, d, _S()) == OK
    base = torch.randn(4, n * d + 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    dfeat, dkq = base.clone(), nan_like((4, d))
    dd = dout.to(DEV)
    assert L.digat_attn_pool_bwd(f0.data_ptr(), n * d, kd.data_ptr(), md.data_ptr(), alpha.data_ptr(), dd.data_ptr(), dfeat.data_ptr(), n * d + 8,
                                 dkq.data_ptr(), 4, n, d, 1, _S()) == OK
    torch.cuda.synchronize()
    close(alpha.sum(1), np.ones(4), "alpha rows sum to one", rtol=1e-6, atol=0)
    close(dfeat[:, :n * d].reshape(4, n, d), base[:, :n * d].reshape(4, n, d).cpu().double() + want_df, f"pool n={n} d={d} dfeat accumulated")
    assert torch.equal(dfeat[:, n * d:], base[:, n * d:])
    close(dkq, want_dk, f"pool n={n} d={d} dkq (raw)")


def _topic_rows(H, C1, d, seed):
    """Four rows of history categories: random with a padded tail; an empty history (every slot on the padding topic C1 - 1); all
    history in topic 0; topic 0 but for ONE slot in another topic."""
    g = torch.Generator().manual_seed(seed)
    C = C1 - 1
    idx = torch.randint(0, C, (4, H), generator=g)
    idx[0, H - H // 3:] = C
    idx[1] = C
    idx[2] = 0
    idx[3] = 0
    idx[3, H - 1] = 1 % C1
    U = H + C
    Xu = torch.randn(4, U, d, generator=g)
    kq = torch.randn(4, d, generator=g) * 2
    dT = torch.randn(4, C1, d, generator=g)
    return Xu, kq, idx, dT


def _topic_reference(Xu, kq, idx, dT, H, C1):
    """oracle.topic_pooling in float64 with identity key / query projections."""
    d = Xu.shape[2]
    eye = torch.eye(d, dtype=torch.float64)
    p = {"user_news_K.weight": eye, "user_news_Q.weight": eye, "user_news_Q.bias": torch.zeros(d, dtype=torch.float64),
         "topic_node_embedding": torch.zeros(C1 - 1, 1)}
    x64, k64 = Xu.double().requires_grad_(True), kq.double().requires_grad_(True)
    T = O.topic_pooling(p, x64, idx, k64, H)
    (T * dT.double()).sum().backward()
    return T.detach(), x64.grad, k64.grad


@pytest.mark.parametrize("H,C1,d", [(1, 2, 4), (50, 18, 400), (64, 18, 36), (65, 18, 36), (256, 33, 36), (65, 18, 516)],
                         ids=["H1-C2", "H50-C18-d400", "H64-register-kernel", "H65-past-register-kernel", "H256-C33-TOPIC_MAX_H", "H65-d516-unsplit-channels"])
def test_topic_pool_backward_against_oracle_autograd(H, C1, d):
    """training.TopicPool (digat_topic_pool_fwd_train / digat_topic_pool_bwd): the H <= 64 register kernel and the one past it, up to
    TOPIC_MAX_H = 256; channels that fit half a workgroup (d <= 512: the halves share the history rows) and that do not.  Rows: an
    empty history, all history in one topic, a topic with exactly one member.  T, dXu (topic rows: zero) and dkq against float64
    autograd through oracle.topic_pooling; the training forward's T equals digat_topic_pool_fwd's bit for bit and alpha sums to 1
    over every non-empty topic."""
    from digat_amd import training
    L = _L()
    Xu, kq, idx, dT = _topic_rows(H, C1, d, H * 100 + C1)
    want_T, want_dX, want_dk = _topic_reference(Xu, kq, idx, dT, H, C1)
    xd, kd = Xu.to(DEV).requires_grad_(True), kq.to(DEV).requires_grad_(True)
    idd = idx.to(DEV)
    T = training.TopicPool.apply(xd, kd, idd, H, C1)
    (T * dT.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    close(T, want_T, f"topics H={H} T", rtol=2e-5, atol=2e-5)
    close(xd.grad, want_dX, f"topics H={H} dXu")
    close(kd.grad, want_dk, f"topics H={H} dkq")
    assert float(xd.grad[:, H:].abs().max()) == 0.0
    U = Xu.shape[1]
    T_inf, T_tr, alpha = nan_like((4, C1, d)), nan_like((4, C1, d)), nan_like((4, H))
    assert L.digat_topic_pool_fwd(xd.data_ptr(), kd.data_ptr(), idd.data_ptr(), T_inf.data_ptr(), 4, U, H, C1, d, _S()) == OK
    assert L.digat_topic_pool_fwd_train(xd.data_ptr(), kd.data_ptr(), idd.data_ptr(), T_tr.data_ptr(), alpha.data_ptr(), 4, U, H, C1, d, _S()) == OK
    torch.cuda.synchronize()
    assert torch.equal(T_inf, T_tr) and torch.equal(T_tr, T.detach())
    sums = torch.zeros(4, C1, dtype=torch.float64).scatter_add(1, idx, alpha.cpu().double())
    members = torch.zeros(4, C1).scatter_add(1, idx, torch.ones(4, H))
    close(sums, (members > 0).double(), "alpha sums to one per non-empty topic", rtol=1e-6, atol=0)
    if (members == 0).any():
        assert float(T_tr.cpu()[members == 0].abs().max()) == 0.0, "an empty topic pools to zero"


def test_topic_pool_rejects_more_than_256_history_slots():
    L = _L()
    H, C1, d = 257, 3, 4
    Xu, kq, T, alpha = torch.zeros(1, H + 2, d, device=DEV), torch.zeros(1, d, device=DEV), nan_like((1, C1, d)), nan_like((1, H))
    idx = torch.zeros(1, H, dtype=torch.int64, device=DEV)
    dX, dk = nan_like((1, H + 2, d)), nan_like((1, d))
    assert L.digat_topic_pool_fwd(Xu.data_ptr(), kq.data_ptr(), idx.data_ptr(), T.data_ptr(), 1, H + 2, H, C1, d, _S()) == ERR_SHAPE
    assert L.digat_topic_pool_fwd_train(Xu.data_ptr(), kq.data_ptr(), idx.data_ptr(), T.data_ptr(), alpha.data_ptr(), 1, H + 2, H, C1, d, _S()) == ERR_SHAPE
    assert L.digat_topic_pool_bwd(Xu.data_ptr(), kq.data_ptr(), idx.data_ptr(), alpha.data_ptr(), T.data_ptr(), dX.data_ptr(), dk.data_ptr(),
                                  1, H + 2, H, C1, d, _S()) == ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(T).all() and torch.isnan(dX).all()


# ======================================================================================================================
# 5. the two context pairs
# ======================================================================================================================
NEWS_W = ("Kc", "Qc", "bQc", "Wg", "bg")
NEWS_NAMES = {"Kc": "candidate_attention.K.weight", "Qc": "candidate_attention.Q.weight", "bQc": "candidate_attention.Q.bias",
              "Wg": "news_graph_W.weight", "bg": "news_graph_W.bias"}


def _news_case(B, N, d):
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + d)
    t = {"X": torch.randn(B, N, d, generator=g), "prev": torch.randn(B, d, generator=g), "dout": torch.randn(B, d, generator=g),
         "Kc": torch.randn(d, d, generator=g) * d ** -0.5, "Qc": torch.randn(d, d, generator=g) * d ** -0.5, "bQc": torch.randn(d, generator=g) * 0.1,
         "Wg": torch.randn(d, 2 * d, generator=g) * (2 * d) ** -0.5, "bg": torch.randn(d, generator=g) * 0.1}
    mask = torch.rand(B, N, generator=g) < 0.7
    mask[:, 0] = True
    if B > 1:
        mask[1] = False                      # a candidate whose whole neighbourhood is masked: uniform pooling
    if B > 2:
        mask[2, 1:] = False                  # ... and one that only sees itself
    t["mask"] = mask
    return t


def _news_reference(t, p, seed, with_prev):
    """oracle.news_graph_context in float64 (the gate's dropout under the library's keep bits), + prev; -> out, {gradients}."""
    w = {k: t[k].double().requires_grad_(True) for k in NEWS_W + ("X", "prev")}
    params = {NEWS_NAMES[k]: w[k] for k in NEWS_W}
    drop = (lambda x, frac: O.hash_dropout(x.contiguous(), p, seed)) if p > 0 else None
    out = O.news_graph_context(params, w["X"], t["mask"], drop)
    if with_prev:
        out = w["prev"] + out
    (out * t["dout"].double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in w.items() if v.grad is not None}


NEWS_SHAPES = [(1, 1, 4), (5, 10, 400), (320, 10, 400), (7, 128, 36), (2100, 3, 80)]
NEWS_IDS = ["1x1x4", "5x10x400", "320x10x400-grouped-products", "7x128x36-most-nodes", "2100x3x80-products-past-2048-rows-go-out-singly"]


@pytest.mark.parametrize("variant", ["plain", "prev", "gate-dropout"])
@pytest.mark.parametrize("B,N,d", NEWS_SHAPES, ids=NEWS_IDS)
def test_news_context_pair_against_oracle_autograd(B, N, d, variant, monkeypatch):
    """training.NewsCtxFused (digat_news_ctx_fwd_train / digat_news_ctx_bwd) alone: out and dX, dKc, dQc, dbQc, dWg, dbg against
    float64 autograd through oracle.news_graph_context — node 0's three paths (pooled value, gate's local term, query; the last two
    added by ``add_node0_kernel``), the three weight gradients of one ``TnGroup`` launch (sent out singly from 2 048 rows on);
    with ``prev`` (out = prev + context, d prev = dout) and with the gate's dropout live (p = 0.2, fixed seed, the same keep
    bits in the oracle), through both bindings."""
    from digat_amd import training
    t = _news_case(B, N, d)
    p, seed = (0.2, 9001) if variant == "gate-dropout" else (0.0, 0)
    want_out, want = _news_reference(t, p, seed, variant == "prev")
    monkeypatch.setattr(training, "_seed", lambda: seed)
    for use_ext in (True, False):
        if not use_ext:
            monkeypatch.setattr(training._lib, "ext", lambda: None)
        v = {k: t[k].to(DEV).requires_grad_(True) for k in NEWS_W + ("X", "prev")}
        out = training.NewsCtxFused.apply(v["X"], t["mask"].to(torch.uint8).to(DEV), v["Kc"], v["Qc"], v["bQc"], v["Wg"], v["bg"], p, None,
                                          v["prev"] if variant == "prev" else None)
        (out * t["dout"].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        close(out, want_out, f"news ctx {variant} out", rtol=2e-5, atol=2e-5)
        for k in NEWS_W + ("X",):
            close(v[k].grad, want[k], f"news ctx {variant} (ext={use_ext}) d{k}")
        if variant == "prev":
            assert torch.equal(v["prev"].grad.cpu(), t["dout"]), "the gradient with respect to prev is the identity"
        else:
            assert v["prev"].grad is None


def _news_raw(t, B, N, d, p, seed, prev, calls, fill):
    """The pair through the ctypes table: forward once, backward ``calls`` times (accumulate_params = 1 from the second on, or from
    the first when ``fill`` is a number: the buffers then start at that value); dX pre-filled with NaN before every call."""
    L = _L()
    v = {k: t[k].to(DEV).contiguous() for k in NEWS_W + ("X", "prev", "dout")}
    md = t["mask"].to(torch.uint8).to(DEV)
    nsave, nws = L.digat_news_ctx_train_save_bytes(B, N, d), L.digat_news_ctx_train_workspace_bytes(B, N, d)
    save, ws = poisoned_bytes(nsave), poisoned_bytes(nws)
    out = nan_like((B, d))
    assert L.digat_news_ctx_fwd_train(v["X"].data_ptr(), md.data_ptr(), v["Kc"].data_ptr(), v["Qc"].data_ptr(), v["bQc"].data_ptr(),
                                      v["Wg"].data_ptr(), v["bg"].data_ptr(), out.data_ptr(), p, seed, B, N, d, save.data_ptr(), nsave, ws.data_ptr(), nws,
                                      v["prev"].data_ptr() if prev else None, _S()) == OK
    grads = {k: (nan_like(t[k].shape) if fill is None else torch.full(t[k].shape, float(fill), device=DEV)) for k in NEWS_W}
    for call in range(calls):
        ws.fill_(255)
        dX = nan_like((B, N, d))
        acc = 1 if (call > 0 or fill is not None) else 0
        assert L.digat_news_ctx_bwd(v["dout"].data_ptr(), v["X"].data_ptr(), md.data_ptr(), v["Kc"].data_ptr(), v["Qc"].data_ptr(), v["Wg"].data_ptr(),
                                    p, save.data_ptr(), nsave, dX.data_ptr(), grads["Kc"].data_ptr(), grads["Qc"].data_ptr(), grads["bQc"].data_ptr(),
                                    grads["Wg"].data_ptr(), grads["bg"].data_ptr(), B, N, d, acc, ws.data_ptr(), nws, _S()) == OK
    torch.cuda.synchronize()
    return out, dX, grads


@pytest.mark.parametrize("B,N,d", [(5, 10, 400), (320, 10, 400), (2100, 3, 80)], ids=["5x10x400", "320x10x400", "2100x3x80-single-products"])
def test_news_context_backward_accumulates_parameters_and_overwrites_dX(B, N, d):
    """digat_news_ctx_bwd through the raw entry with poisoned scratch: called twice with accumulate_params = 1 the second time the
    five parameter gradients are twice autograd's, accumulated onto buffers holding 0.5 they are 0.5 more; dX (pre-filled with NaN)
    is overwritten, not doubled — in the grouped slice reduction (B < 2 048) and in the single launches (B >= 2 048) alike."""
    t = _news_case(B, N, d)
    want_out, want = _news_reference(t, 0.0, 0, True)
    out, dX, g1 = _news_raw(t, B, N, d, 0.0, 0, True, 1, None)
    close(out, want_out, "news ctx raw out", rtol=2e-5, atol=2e-5)
    close(dX, want["X"], "news ctx raw dX")
    for k in NEWS_W:
        close(g1[k], want[k], f"news ctx raw d{k}")
    _, dX2, g2 = _news_raw(t, B, N, d, 0.0, 0, True, 2, None)
    assert torch.equal(dX2, dX)
    for k in NEWS_W:
        close(g2[k], 2 * want[k], f"news ctx raw, two calls: d{k}")
    _, _, g3 = _news_raw(t, B, N, d, 0.0, 0, True, 1, 0.5)
    for k in NEWS_W:
        close(g3[k], 0.5 + want[k], f"news ctx raw, onto 0.5: d{k}")


USER_W = ("Ku", "Qu", "bQu", "Fa", "bFa", "Kua", "Qua", "bQua")
USER_NAMES = {"Ku": "user_news_K.weight", "Qu": "user_news_Q.weight", "bQu": "user_news_Q.bias", "Fa": "featureAffine.weight", "bFa": "featureAffine.bias",
              "Kua": "userAttention.K.weight", "Qua": "userAttention.Q.weight", "bQua": "userAttention.Q.bias"}
RELU_MARGIN = 1e-4


def _user_case(B, H, C, d):
    """Inputs of one user-context call.  Row 1 (when there is one) has an empty history, row 2 a category mask that leaves one
    topic.  featureAffine's bias is nudged, column by column, until no pre-activation of the float64 forward lies within 1e-4 of
    relu's kink: the fp32 kernels' pre-activations differ from float64's by ~1e-6, and an element that lands on the other side of 0
    changes gradients by a whole term — a property of relu at 0, not an error of either side (at B C1 d = 864 000 elements one
    such element is expected otherwise)."""
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + d)
    C1, U = C + 1, H + C
    t = {"Xu": torch.randn(B, U, d, generator=g) * 0.5, "c_n": torch.randn(B, d, generator=g), "prev": torch.randn(B, d, generator=g),
         "dout": torch.randn(B, d, generator=g)}
    for k in ("Ku", "Qu", "Fa", "Kua", "Qua"):
        t[k] = torch.randn(d, d, generator=g) * d ** -0.5
    for k in ("bQu", "bFa", "bQua"):
        t[k] = torch.randn(d, generator=g) * 0.1
    idx = torch.randint(0, C, (B, H), generator=g)
    length = torch.randint(1, H + 1, (B,), generator=g)
    if B > 1:
        length[1] = 0
    idx[torch.arange(H).unsqueeze(0) >= length.unsqueeze(1)] = C
    cat_mask = torch.zeros(B, C1, dtype=torch.bool)
    cat_mask.scatter_(1, idx, torch.ones(B, H, dtype=torch.bool))
    cat_mask[:, C] = False
    if B > 2:
        cat_mask[2] = False
        cat_mask[2, int(idx[2, 0])] = True
    t["idx"], t["cat_mask"] = idx, cat_mask
    with torch.no_grad():
        p = {USER_NAMES[k]: t[k].double() for k in USER_W}
        p["topic_node_embedding"] = torch.zeros(C, 1)
        T = O.topic_pooling(p, t["Xu"].double(), idx, t["c_n"].double(), H).reshape(B * C1, d)
        y0 = T @ t["Fa"].double().T
        for o in range(d):
            while float((y0[:, o] + float(t["bFa"][o])).abs().min()) < RELU_MARGIN:
                t["bFa"][o] += 4 * RELU_MARGIN
    return t


def _user_reference(t, H, p, seed, with_prev):
    w = {k: t[k].double().requires_grad_(True) for k in USER_W + ("Xu", "c_n", "prev")}
    params = {USER_NAMES[k]: w[k] for k in USER_W}
    params["topic_node_embedding"] = torch.zeros(t["cat_mask"].shape[1] - 1, 1)
    drop = (lambda x, frac: O.hash_dropout(x.contiguous(), p, seed)) if p > 0 else None
    out = O.user_graph_context(params, w["Xu"], t["cat_mask"], t["idx"], w["c_n"], H, drop)
    if with_prev:
        out = w["prev"] + out
    (out * t["dout"].double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in w.items() if v.grad is not None}


USER_SHAPES = [(1, 1, 1, 4), (5, 50, 17, 400), (3, 256, 32, 36), (120, 50, 17, 400), (64, 70, 31, 80)]
USER_IDS = ["1x1x1x4", "5x50x17x400-fp32-featureAffine", "3x256x32x36-TOPIC_MAX_H", "120x50x17x400-bf16x6-featureAffine-2160-rows", "64x70x31x80-2048-rows"]


@pytest.mark.parametrize("variant", ["plain", "prev", "topic-dropout"])
@pytest.mark.parametrize("B,H,C,d", USER_SHAPES, ids=USER_IDS)
def test_user_context_pair_against_oracle_autograd(B, H, C, d, variant, monkeypatch):
    """training.UserCtxFused (digat_user_ctx_fwd_train / digat_user_ctx_bwd) alone: out, dXu, dc_n and the eight parameter gradients
    against float64 autograd through oracle.user_graph_context.  featureAffine and its two gradients run fp32 below B C1 = 2 048
    rows and bf16x6 from there on (asserted per shape); the five weight gradients make ``TnGroup`` flush in mid-call.  A row with an
    empty history, a row whose category mask leaves one topic; with ``prev``; with the pooled topics' dropout live (p = 0.2, the
    same keep bits in the oracle); through both bindings."""
    from digat_amd import training
    C1 = C + 1
    assert training._x3_ok(B * C1, d, d) == (B * C1 >= 2048), "the shapes are meant to sit on either side of the bf16x6 switch"
    t = _user_case(B, H, C, d)
    p, seed = (0.2, 7007) if variant == "topic-dropout" else (0.0, 0)
    want_out, want = _user_reference(t, H, p, seed, variant == "prev")
    monkeypatch.setattr(training, "_seed", lambda: seed)
    for use_ext in (True, False):
        if not use_ext:
            monkeypatch.setattr(training._lib, "ext", lambda: None)
        v = {k: t[k].to(DEV).requires_grad_(True) for k in USER_W + ("Xu", "c_n", "prev")}
        out = training.UserCtxFused.apply(v["Xu"], t["cat_mask"].to(torch.uint8).to(DEV), t["idx"].to(DEV), v["c_n"], v["Ku"], v["Qu"], v["bQu"], v["Fa"],
                                          v["bFa"], v["Kua"], v["Qua"], v["bQua"], H, C1, p, None, None, v["prev"] if variant == "prev" else None)
        (out * t["dout"].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        close(out, want_out, f"user ctx {variant} out", rtol=2e-5, atol=2e-5)
        for k in USER_W + ("Xu", "c_n"):
            close(v[k].grad, want[k], f"user ctx {variant} (ext={use_ext}) d{k}")
        assert float(v["Xu"].grad[:, H:].abs().max()) == 0.0, "topic rows of dXu"
        if variant == "prev":
            assert torch.equal(v["prev"].grad.cpu(), t["dout"]), "the gradient with respect to prev is the identity"


def _user_raw(t, B, H, C, d, p, seed, prev, calls, fill, images):
    """As ``_news_raw``; ``images``: featureAffine's forward / backward split images from training.split_images, or None."""
    L = _L()
    C1, U = C + 1, H + C
    v = {k: t[k].to(DEV).contiguous() for k in USER_W + ("Xu", "c_n", "prev", "dout")}
    md, idd = t["cat_mask"].to(torch.uint8).to(DEV), t["idx"].to(DEV)
    nsave, nws = L.digat_user_ctx_train_save_bytes(B, U, H, C1, d), L.digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)
    save, ws = poisoned_bytes(nsave), poisoned_bytes(nws)
    out = nan_like((B, d))
    img_f, img_b = images if images is not None else (None, None)
    assert L.digat_user_ctx_fwd_train(v["Xu"].data_ptr(), md.data_ptr(), idd.data_ptr(), v["c_n"].data_ptr(), v["Ku"].data_ptr(), v["Qu"].data_ptr(),
                                      v["bQu"].data_ptr(), v["Fa"].data_ptr(), v["bFa"].data_ptr(), v["Kua"].data_ptr(), v["Qua"].data_ptr(),
                                      v["bQua"].data_ptr(), out.data_ptr(), p, seed, B, U, H, C1, d, save.data_ptr(), nsave, ws.data_ptr(), nws,
                                      _lib().ptr(img_f), v["prev"].data_ptr() if prev else None, _S()) == OK
    grads = {k: (nan_like(t[k].shape) if fill is None else torch.full(t[k].shape, float(fill), device=DEV)) for k in USER_W}
    for call in range(calls):
        ws.fill_(255)
        dXu, dc = nan_like((B, U, d)), nan_like((B, d))
        acc = 1 if (call > 0 or fill is not None) else 0
        assert L.digat_user_ctx_bwd(v["dout"].data_ptr(), v["Xu"].data_ptr(), md.data_ptr(), idd.data_ptr(), v["c_n"].data_ptr(), v["Ku"].data_ptr(),
                                    v["Qu"].data_ptr(), v["Fa"].data_ptr(), v["Kua"].data_ptr(), v["Qua"].data_ptr(), p, save.data_ptr(), nsave,
                                    dXu.data_ptr(), dc.data_ptr(), grads["Ku"].data_ptr(), grads["Qu"].data_ptr(), grads["bQu"].data_ptr(),
                                    grads["Fa"].data_ptr(), grads["bFa"].data_ptr(), grads["Kua"].data_ptr(), grads["Qua"].data_ptr(),
                                    grads["bQua"].data_ptr(), B, U, H, C1, d, acc, ws.data_ptr(), nws, _lib().ptr(img_b), _S()) == OK
    torch.cuda.synchronize()
    return out, dXu, dc, grads


@pytest.mark.parametrize("B,H,C,d", [(5, 50, 17, 400), (120, 50, 17, 400), (64, 70, 31, 80)], ids=["5x50x17x400-fp32", "120x50x17x400-bf16x6", "64x70x31x80-bf16x6"])
def test_user_context_backward_zero_fills_topic_rows_accumulates_parameters_and_takes_split_images(B, H, C, d):
    """digat_user_ctx_bwd through the raw entry with poisoned scratch and dXu / dc_n pre-filled with NaN: the topic rows of dXu come
    back exactly 0 (``topic_pool_bwd_zero``), its history rows and dc_n equal autograd; a second call with accumulate_params = 1
    doubles the eight parameter gradients and leaves dXu / dc_n as they were; accumulating onto 0.5 adds 0.5.  With featureAffine's
    pre-split images (training.split_images, layouts 0 and 1) handed to the pair every result is bit-identical to the calls that
    split the weight themselves — with the topic dropout live."""
    from digat_amd import training
    t = _user_case(B, H, C, d)
    want_out, want = _user_reference(t, H, 0.0, 0, True)
    out, dXu, dc, g1 = _user_raw(t, B, H, C, d, 0.0, 0, True, 1, None, None)
    close(out, want_out, "user ctx raw out", rtol=2e-5, atol=2e-5)
    assert float(dXu[:, H:].abs().max()) == 0.0, "topic rows of dXu must be zero-filled by the call"
    close(dXu, want["Xu"], "user ctx raw dXu")
    close(dc, want["c_n"], "user ctx raw dc_n")
    for k in USER_W:
        close(g1[k], want[k], f"user ctx raw d{k}")
    _, dXu2, dc2, g2 = _user_raw(t, B, H, C, d, 0.0, 0, True, 2, None, None)
    assert torch.equal(dXu2, dXu) and torch.equal(dc2, dc)
    for k in USER_W:
        close(g2[k], 2 * want[k], f"user ctx raw, two calls: d{k}")
    _, _, _, g3 = _user_raw(t, B, H, C, d, 0.0, 0, True, 1, 0.5, None)
    for k in USER_W:
        close(g3[k], 0.5 + want[k], f"user ctx raw, onto 0.5: d{k}")
    # pre-split images: the same bits
    p, seed = 0.2, 4711
    a = _user_raw(t, B, H, C, d, p, seed, False, 1, None, None)
    Fa = t["Fa"].to(DEV).contiguous()
    images = training.split_images([((Fa,), 0), ((Fa,), 1)], torch.device(DEV))
    b = _user_raw(t, B, H, C, d, p, seed, False, 1, None, (images[0], images[1]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in USER_W:
        assert torch.equal(a[3][k], b[3][k]), k
    want_out, want = _user_reference(t, H, p, seed, False)
    close(b[0], want_out, "user ctx raw out under dropout, with images", rtol=2e-5, atol=2e-5)
    close(b[1], want["Xu"], "user ctx raw dXu under dropout, with images")
    close(b[3]["Fa"], want["Fa"], "user ctx raw dFa under dropout, with images")


# ======================================================================================================================
# 6. the fine-grained Functions of training.py
# ======================================================================================================================
@pytest.mark.parametrize("M", [64, 2100], ids=["64-rows-fp32", "2100-rows-bf16x6"])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_function_against_fp64_autograd(M, bias):
    """training.Linear: y = x W^T + b on [.., K] inputs; forward, dx, dW, db against float64 torch, on either side of ``_x3_ok``
    (N = K = 80)."""
    from digat_amd import training
    N = K = 80
    assert training._x3_ok(M, N, K) == (M >= 2048)
    g = torch.Generator().manual_seed(M)
    x, W, b, dy = torch.randn(M // 4, 4, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn(M // 4, 4, N, generator=g)
    r = [a.double().requires_grad_(True) for a in (x, W, b)]
    y64 = torch.nn.functional.linear(r[0], r[1], r[2] if bias else None)
    (y64 * dy.double()).sum().backward()
    v = [a.to(DEV).requires_grad_(True) for a in (x, W, b)]
    y = training.Linear.apply(v[0], v[1], v[2] if bias else None)
    (y * dy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    close(y, y64.detach(), "Linear y", rtol=1e-5, atol=2e-6 * math.sqrt(K))
    close(v[0].grad, r[0].grad, "Linear dx", rtol=1e-5, atol=2e-6 * math.sqrt(N))
    close(v[1].grad, r[1].grad, "Linear dW", rtol=1e-5, atol=2e-6 * math.sqrt(M))
    if bias:
        close(v[2].grad, r[2].grad, "Linear db", rtol=1e-5, atol=2e-6 * math.sqrt(M))
    else:
        assert v[2].grad is None


@pytest.mark.parametrize("M", [64, 2100], ids=["64-rows-fp32", "2100-rows-bf16x6"])
def test_matmul_w_function_against_fp64_autograd(M):
    """training.MatmulW: y = x @ W (the key projection folded onto the query); forward, dx, dW against float64 torch."""
    from digat_amd import training
    N = K = 80
    g = torch.Generator().manual_seed(M + 1)
    x, W, dy = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g) * N ** -0.5, torch.randn(M, K, generator=g)
    r = [a.double().requires_grad_(True) for a in (x, W)]
    y64 = r[0] @ r[1]
    (y64 * dy.double()).sum().backward()
    v = [a.to(DEV).requires_grad_(True) for a in (x, W)]
    y = training.MatmulW.apply(v[0], v[1])
    (y * dy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    close(y, y64.detach(), "MatmulW y", rtol=1e-5, atol=2e-6 * math.sqrt(N))
    close(v[0].grad, r[0].grad, "MatmulW dx", rtol=1e-5, atol=2e-6 * math.sqrt(K))
    close(v[1].grad, r[1].grad, "MatmulW dW", rtol=1e-5, atol=2e-6 * math.sqrt(M))


@pytest.mark.parametrize("B", [64, 2100])
def test_gate_mix_and_relu_res_functions_against_fp64_autograd(B):
    """training.GateMix and training.ReluRes through torch.autograd against the same expressions in float64 (tolerances of the
    primitives' own tests above)."""
    from digat_amd import training
    d = 80
    g = torch.Generator().manual_seed(B)
    z, l, gl, dout, y = (torch.randn(B, d, generator=g) for _ in range(5))
    z = z * 3
    y[::2, ::3] = 0.0
    r = [a.double().requires_grad_(True) for a in (z, l, gl)]
    s = torch.sigmoid(r[0])
    o64 = s * r[1] + (1 - s) * r[2]
    (o64 * dout.double()).sum().backward()
    v = [a.to(DEV).requires_grad_(True) for a in (z, l, gl)]
    o = training.GateMix.apply(*v)
    (o * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    amp = float(max(l.abs().max(), gl.abs().max()))
    close(o, o64.detach(), "GateMix out", rtol=1e-6, atol=GATE_ATOL * amp)
    close(v[0].grad, r[0].grad, "GateMix dz", rtol=1e-6, atol=GATE_ATOL * float((dout * (l - gl)).abs().max()))
    close(v[1].grad, r[1].grad, "GateMix dl", rtol=1e-6, atol=GATE_ATOL * float(dout.abs().max()))
    close(v[2].grad, r[2].grad, "GateMix dg", rtol=1e-6, atol=GATE_ATOL * float(dout.abs().max()))
    ry, rt = y.double().requires_grad_(True), l.double().requires_grad_(True)
    ((torch.relu(ry) + rt) * dout.double()).sum().backward()
    vy, vt = y.to(DEV).requires_grad_(True), l.to(DEV).requires_grad_(True)
    o = training.ReluRes.apply(vy, vt)
    (o * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    close(o, (torch.relu(y.double()) + l.double()), "ReluRes out", rtol=1e-6, atol=0.0)
    assert torch.equal(vy.grad.cpu().double(), ry.grad) and torch.equal(vt.grad.cpu().double(), rt.grad)


@pytest.mark.parametrize("B,n,d", [(3, 10, 80), (32, 67, 80)], ids=["30-rows-fp32", "2144-rows-bf16x6"])
def test_xattn_layer_function_against_oracle_autograd_and_the_fused_pair(B, n, d):
    """training.XattnLayer (projections, pairwise forward / backward, the three input and weight gradients and K3's node sum as
    separate library calls; K3 = ffn3(ctx) through training.Linear) against float64 autograd through oracle.cross_graph_attention,
    and against training.XattnFused on the same inputs, both at the fused pair's tolerance — on either side of ``_x3_ok``."""
    from digat_amd import training
    assert training._x3_ok(B * n, d, d) == (B * n >= 2048)
    g = torch.Generator().manual_seed(B * n + d)
    X, ctx, dOut = torch.randn(B, n, d, generator=g), torch.randn(B, d, generator=g), torch.randn(B, n, d, generator=g)
    A = (torch.rand(B, n, n, generator=g) < min(1.0, 6.0 / n)) | torch.eye(n, dtype=torch.bool).unsqueeze(0)
    A[1, 0] = False
    shapes = [("W", (d, d), d ** -0.5), ("bW", (d,), 0.1), ("F1", (d, d), d ** -0.5), ("F2", (d, d), d ** -0.5), ("F3", (d, d), d ** -0.5),
              ("b3", (d,), 0.1), ("a", (1, d), d ** -0.5)]
    w = {k: torch.randn(*shape, generator=g) * scale for k, shape, scale in shapes}
    names = {"W": "W.0.weight", "bW": "W.0.bias", "F1": "ffn1.0.weight", "F2": "ffn2.0.weight", "F3": "ffn3.0.weight", "b3": "ffn3.0.bias", "a": "a.0.weight"}
    p = {"user_graph_attention_" + names[k]: v.double().requires_grad_(True) for k, v in w.items()}
    Xo, co = X.double().requires_grad_(True), ctx.double().requires_grad_(True)
    want_out = O.cross_graph_attention(p, "user", 0, Xo, A, co)
    (want_out * dOut.double()).sum().backward()
    want = {"X": Xo.grad, "ctx": co.grad, **{k: p["user_graph_attention_" + names[k]].grad for k in w}}
    Ab = A.to(torch.uint8).to(DEV).contiguous()

    def run(fused):
        dv = {k: v.to(DEV).requires_grad_(True) for k, v in w.items()}
        Xd, cd = X.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
        if fused:
            out = training.XattnFused.apply(Xd, Ab, cd, dv["W"], dv["bW"], dv["F1"], dv["F2"], dv["F3"], dv["b3"], dv["a"], 0.0)
        else:
            r = training.Linear.apply(cd, dv["F3"], dv["b3"])
            out = training.XattnLayer.apply(Xd, Ab, r, dv["W"], dv["bW"], dv["F1"], dv["F2"], dv["a"], 0.0)
        (out * dOut.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), {"X": Xd.grad, "ctx": cd.grad, **{k: dv[k].grad for k in w}}
    out_l, got_l = run(False)
    out_f, got_f = run(True)
    close(out_l, want_out.detach(), "XattnLayer out", rtol=2e-5, atol=2e-5)
    close(out_l, out_f, "XattnLayer out vs XattnFused", rtol=2e-5, atol=2e-5)
    for k in want:
        close(got_l[k], want[k], f"XattnLayer d{k}")
        close(got_l[k], got_f[k], f"XattnLayer d{k} vs XattnFused")
