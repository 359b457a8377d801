"""GPU suite: ragged 240-column tiles of the strip-mined GEMM (GemmArgs::ragged) give the bits of the launch that does not ask.

A launch whose N is more than three strips and no multiple of three runs, when it asks, as ceil(strips / 3) column tiles whose
last has one or two strips (N = 400: 3 + 2, N = 800 in two segments: 3 + 3 + 3 + 1) instead of one-strip tiles.  No output
element's product chain changes, so the results are compared with torch.equal against the same launch with the field clear —
for both tile orders, both operand formats, with a row list (two row tiles: 128 and 72 rows), an empty one and none, a K
tail, relu + residual and the K3 addend on segment 1.  Shapes are the smallest that reach every branch: m_dispatch makes the
384-row launch take the kernel and tiles of a large one.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, LISTED, ROWS_PER_B = 384, 200, 16
BIG = 1 << 30


def _launch(L, _lib, x, w, b, e0, radd, rowidx, nrows, nseg, K, fmt, ragged):
    """y of one launch into NaN-prefilled planes (one per segment)"""
    nsegs = len(w)
    ys = [torch.full((M, nseg), float("nan"), device=DEV) for _ in range(nsegs)]
    ws = torch.empty(L.digat_split_weights_bytes(nsegs * nseg, K), dtype=torch.uint8, device=DEV)
    two = nsegs == 2
    rc = L.digat_linear_rows_f32x3(x.data_ptr(), K, w[0].data_ptr(), w[1].data_ptr() if two else None, b[0].data_ptr(),
                                   b[1].data_ptr() if two else None, ys[0].data_ptr(), ys[1].data_ptr() if two else None, nseg, M, nseg, K,
                                   ws.data_ptr(), fmt, rowidx.data_ptr() if rowidx is not None else None,
                                   nrows.data_ptr() if rowidx is not None else None, e0.data_ptr() if e0 is not None else None, nseg,
                                   radd.data_ptr() if radd is not None and two else None, ROWS_PER_B, BIG, ragged, _lib.stream_ptr())
    _lib.check(rc, "digat_linear_rows_f32x3")
    torch.cuda.synchronize()
    L.digat_forget_split_image(ws.data_ptr())
    return ys


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(20)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    listed = np.sort(rng.choice(M, LISTED, replace=False)).astype(np.int32)
    return {"x": {K: t(rng.standard_normal((M, K))) for K in (400, 48)},
            "w": {(n, K): [t(rng.standard_normal((n, K)) / np.sqrt(K)) for _ in range(2)] for n in (400, 160) for K in (400, 48)},
            "b": {n: [t(rng.standard_normal(n)) for _ in range(2)] for n in (400, 160)},
            "e0": {n: t(rng.standard_normal((M, n))) for n in (400, 160)},
            "radd": t(rng.standard_normal((M // ROWS_PER_B, 400))),
            "listed": listed, "rowidx": torch.from_numpy(listed).to(DEV)}


@pytest.mark.parametrize("fmt", [0, 1], ids=["bf16x6", "fp16x3"])
@pytest.mark.parametrize("K", [400, 48])
@pytest.mark.parametrize("rows", ["list", "empty", "all"])
@pytest.mark.parametrize("shape", ["n400", "n800_two_segments", "n160_ignored"])
def test_ragged_tiles_give_the_bits_of_the_launch_without(operands, shape, rows, K, fmt):
    from digat_amd import _lib
    L = _lib.lib()
    nseg, nsegs = {"n400": (400, 1), "n800_two_segments": (400, 2), "n160_ignored": (160, 1)}[shape]
    o = operands
    rowidx = o["rowidx"] if rows != "all" else None
    nrows = torch.tensor([LISTED if rows == "list" else 0], dtype=torch.int32, device=DEV)
    args = (o["x"][K], o["w"][(nseg, K)][:nsegs], o["b"][nseg][:nsegs], o["e0"][nseg], o["radd"], rowidx, nrows, nseg, K, fmt)
    want = _launch(L, _lib, *args, 0)
    written = np.arange(M) if rows == "all" else (o["listed"] if rows == "list" else np.zeros(0, dtype=np.int32))
    mask = torch.zeros(M, dtype=torch.bool, device=DEV)
    mask[torch.from_numpy(written.astype(np.int64)).to(DEV)] = True
    for ragged in (1, 2):
        got = _launch(L, _lib, *args, ragged)
        for s in range(nsegs):
            assert torch.isfinite(want[s][mask]).all()
            assert torch.equal(got[s][mask], want[s][mask]), (shape, rows, K, fmt, ragged, s)
            assert torch.isnan(got[s][~mask]).all(), "a row outside the list was written"
            assert torch.isnan(want[s][~mask]).all()


@pytest.mark.parametrize("fmt", [0, 1], ids=["bf16x6", "fp16x3"])
def test_ragged_tiles_against_an_fp64_product(operands, fmt):
    """The ragged launch (N = 400, K = 400, all 384 rows, bias only) against an fp64 product, next to the fp32-MFMA kernel on the
    same data, at the bounds the formats are held to elsewhere: fp16x3 mean and largest error at most 1.1x the fp32 chain's
    (tests/test_hip_lowprec.py), bf16x6 mean at most 1.5x and every element within rtol 1e-5 + 2e-6 sqrt(K) (tests/test_hip_parity.py)."""
    from digat_amd import _lib
    L = _lib.lib()
    o, K, N = operands, 400, 400
    x, w, b = o["x"][K], o["w"][(N, K)][:1], o["b"][N][:1]
    nrows = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _launch(L, _lib, x, w, b, None, None, None, nrows, N, K, fmt, 1)[0].cpu().numpy().astype(np.float64)
    # the chain those bounds speak of is the 128-row fp32-MFMA kernel's (one k-ordered fma chain per element), which runs from 2 048
    # rows up — below, digat_linear_f32 keeps two K tiles in flight and sums them pairwise: the 384 rows go through it six times over
    reps = 6
    x6, y32 = x.repeat(reps, 1), torch.full((reps * M, N), float("nan"), device=DEV)
    _lib.check(L.digat_linear_f32(x6.data_ptr(), K, w[0].data_ptr(), b[0].data_ptr(), y32.data_ptr(), N, reps * M, N, K, _lib.stream_ptr()),
               "digat_linear_f32")
    torch.cuda.synchronize()
    y32 = y32[:M]
    want = x.cpu().numpy().astype(np.float64) @ w[0].cpu().numpy().astype(np.float64).T + b[0].cpu().numpy().astype(np.float64)
    e, e32 = np.abs(got - want), np.abs(y32.cpu().numpy().astype(np.float64) - want)
    print(f"\n[ragged fmt {fmt}] mean {e.mean():.3e} (fp32 chain {e32.mean():.3e}), max {e.max():.3e} ({e32.max():.3e})")
    assert np.isfinite(e).all()
    if fmt == 1:
        assert e.mean() <= 1.1 * e32.mean() + 1e-9 and e.max() <= 1.1 * e32.max() + 1e-8
    else:
        assert e.mean() <= 1.5 * e32.mean() + 1e-9
        assert (e <= 2e-6 * np.sqrt(K) + 1e-5 * np.abs(want)).all()
