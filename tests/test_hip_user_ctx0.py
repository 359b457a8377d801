"""GPU suite: the initial user context in one launch (``digat_user_ctx0_fwd``: the GEMM F x = ue Fa^T + ``user_ctx0_kernel``,
csrc/digat_ctx0.inc) through ctypes, without the encoder.

Reference: compute_user_graph_context (graphEncoders.py:123-134) on the input history rows, evaluated here in fp64 with torch on the
CPU from the two folded queries: topic softmax by category, featureAffine, ReLU, residual, masked scaled-dot-product pooling.
Tolerance: rtol = atol = 2e-5, what the suite holds encoder contexts to against the oracle (test_hip_parity.py, fused user context);
and on the same inputs the new path's maximum error may not exceed twice that of the three launches it replaces
(``digat_user_ctx_fwd``: same number of roundings, another order).  The old entry derives the queries from c_n itself, so the
test gives it identity K / Q matrices (and a permutation for the user query): both paths then see bit-identical queries.

Measured on the MI355X (max |error| against fp64, exact fp32 product, worst of the sixteen shapes: H = 53, C + 1 = 6, d = 400):
new path 2.266e-06, three launches 2.266e-06 (equal in every shape: the largest error sits in a one-item category, where both
paths run the same product on the same kernel); the three launches as a 30- / 90-row call, on the K-splitting kernel: 8.4e-07.
d = 64: 2.8e-07 ... 9.5e-07 in both.  On the split images (H = 50, d = 400): bf16x6 1.10e-06, fp16x3 1.01e-06.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu



def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _case(H, C1, d, seed):
    """Five rows over two groups, row_group not in contiguous runs.  Row 0 reads every category it can (min(H, C1) of them) and
    has every bucket unmasked; row 1 has an empty history (every index out of range) and some buckets unmasked (relu(b) buckets);
    row 2 has one item; row 3 reads two categories of which one is masked, and an unread one is unmasked; row 4 has every bucket
    masked (uniform weights)."""
    g = torch.Generator().manual_seed(seed)
    B, G = 5, 2
    ue = torch.randn(G, H, d, generator=g)
    rg = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    idx = torch.empty(B, H, dtype=torch.int64)
    idx[0] = torch.arange(H) % C1
    idx[1] = torch.tensor([C1 + 1, -1] * H)[:H]
    idx[2] = -1
    idx[2, 0] = 2
    idx[3] = torch.where(torch.rand(H, generator=g) < 0.5, 1, 3)
    idx[3, 0], idx[3, H - 1] = 1, 3
    idx[4] = torch.randint(0, C1, (H,), generator=g)
    idx[4, H // 2:] = C1 - 1                                  # a right-padded history: the padding bucket is a category like any other
    mask = torch.zeros(B, C1, dtype=torch.uint8)
    mask[0] = 1
    mask[1, [0, 3]] = 1
    mask[2, 2] = 1
    mask[3, [3, 4]] = 1                                       # category 1 is read and masked, category 4 unread and unmasked
    c_n = torch.randn(B, d, generator=g)
    perm = torch.randperm(d, generator=g)
    Fa = torch.randn(d, d, generator=g) / math.sqrt(d)
    bFa = 0.3 * torch.randn(d, generator=g)                   # both signs: relu(b) has zeros and positive entries
    return dict(ue=ue, rg=rg, idx=idx, mask=mask, c_n=c_n, perm=perm, Fa=Fa, bFa=bFa, kq_t=c_n.clone(), kq_u=c_n[:, perm].contiguous())


def _reference(c, H, C1, d):
    """fp64, row by row."""
    x_all = c["ue"].double().index_select(0, c["rg"].long())
    Fa, b = c["Fa"].double(), c["bFa"].double()
    out = torch.empty(x_all.shape[0], d, dtype=torch.float64)
    for r in range(x_all.shape[0]):
        x, idx = x_all[r], c["idx"][r]
        a = (x @ c["kq_t"][r].double()) / math.sqrt(d)
        T = torch.zeros(C1, d, dtype=torch.float64)
        for cat in range(C1):
            sel = (idx == cat).nonzero().flatten()
            if sel.numel():
                T[cat] = torch.softmax(a[sel], 0) @ x[sel]
        T2 = torch.relu(T @ Fa.T + b) + T
        s = (T2 @ c["kq_u"][r].double()) / math.sqrt(d)
        s = s.masked_fill(c["mask"][r] == 0, -1e9)
        out[r] = torch.softmax(s, 0) @ T2
    return out


def _call(L, _lib, ue, rg, G, c, B, H, C1, d, image=None, fmt=0, addend=None, kq=None, idx=None, mask=None):
    dev = ue.device
    rows = G if rg is not None else B
    nbytes = rows * H * d * 4
    scratch = torch.full((rows * H * d,), float("nan"), device=dev)
    out = torch.full((B, d), float("nan"), device=dev) if addend is None else addend.clone()
    kq_t, kq_u = kq if kq is not None else (c["kq_t"], c["kq_u"])
    idx = c["idx"] if idx is None else idx
    mask = c["mask"] if mask is None else mask
    _lib.check(L.digat_user_ctx0_fwd(ue.data_ptr(), rg.data_ptr() if rg is not None else None, G, kq_t.data_ptr(), kq_u.data_ptr(),
                                     mask.data_ptr(), idx.data_ptr(), c["Fa"].data_ptr(), c["bFa"].data_ptr(),
                                     image.data_ptr() if image is not None else None, fmt, out.data_ptr() if addend is not None else None,
                                     out.data_ptr(), B, H, C1, d, scratch.data_ptr(), nbytes, _lib.stream_ptr()), "digat_user_ctx0_fwd")
    return out


def _three_launches(L, _lib, c, B, H, C1, d, min_gemm_rows=2048):
    """digat_user_ctx_fwd on the same rows.  The entry picks featureAffine's GEMM kernel from its row count B C1: below 2 048 rows a
    K-splitting [B,d] kernel (another summation tree over K, a few times more accurate than any k-ordered chain), from 2 048 rows up
    the tiled kernel family every encoder pass runs it on — the family the new path's F x is pinned to.  "Same number of roundings,
    another order" compares like with like only on that family, so the five rows are repeated until B C1 >= 2 048 (rows are
    independent; the first five are returned)."""
    dev = c["ue"].device
    rep = -(-min_gemm_rows // (B * C1))
    Xu = c["ue"].index_select(0, c["rg"].long()).repeat(rep, 1, 1).contiguous()  # U = H: the pooling reads the history rows only
    mask, idx, c_n = c["mask"].repeat(rep, 1).contiguous(), c["idx"].repeat(rep, 1).contiguous(), c["c_n"].repeat(rep, 1).contiguous()
    Bx = B * rep
    eye = torch.eye(d, device=dev)
    P = torch.zeros(d, d, device=dev)
    P[torch.arange(d, device=dev), c["perm"]] = 1.0                            # (P c)[i] = c[perm[i]]
    zero = torch.zeros(d, device=dev)
    nb = L.digat_user_ctx_workspace_bytes(Bx, H, H, C1, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.full((Bx, d), float("nan"), device=dev)
    _lib.check(L.digat_user_ctx_fwd(Xu.data_ptr(), mask.data_ptr(), idx.data_ptr(), c_n.data_ptr(), eye.data_ptr(), eye.data_ptr(),
                                    zero.data_ptr(), c["Fa"].data_ptr(), c["bFa"].data_ptr(), eye.data_ptr(), P.data_ptr(), zero.data_ptr(),
                                    None, out.data_ptr(), Bx, H, H, C1, d, ws.data_ptr(), nb, _lib.stream_ptr()), "digat_user_ctx_fwd")
    return out[:B]


SHAPES = [(H, C1, d) for d in (64, 400) for H in (5, 50, 52, 53) for C1 in (6, 18)]
_worst = {"new": 0.0, "old": 0.0}


@pytest.mark.parametrize("H,C1,d", SHAPES)
def test_ctx0_against_fp64_and_the_three_launches(H, C1, d):
    """Grouped and per-row calls against the fp64 reference at 2e-5 / 2e-5 and against each other bit for bit; the new path's
    maximum error at most twice the three launches'.  Scratch and output start as NaN.
    Measured (MI355X), worst shape: new 2.266e-06, three launches 2.266e-06 (the module docstring has the rest)."""
    from digat_amd import _lib
    L = _lib.lib()
    dev = _dev()
    c = _case(H, C1, d, seed=1000 * H + 10 * C1 + d)
    want = _reference(c, H, C1, d)
    c = {k: v.to(dev) for k, v in c.items()}
    B, G = 5, 2
    grouped = _call(L, _lib, c["ue"], c["rg"], G, c, B, H, C1, d)
    per_row = _call(L, _lib, c["ue"].index_select(0, c["rg"].long()).contiguous(), None, 0, c, B, H, C1, d)
    old = _three_launches(L, _lib, c, B, H, C1, d)
    old_small = _three_launches(L, _lib, c, B, H, C1, d, min_gemm_rows=1)      # 5 C1 rows: the K-splitting kernel, printed only
    torch.cuda.synchronize()
    assert torch.isfinite(grouped).all() and torch.isfinite(per_row).all()
    assert torch.equal(grouped, per_row), float((grouped - per_row).abs().max())
    err_new = float((grouped.double().cpu() - want).abs().max())
    err_old = float((old.double().cpu() - want).abs().max())
    _worst["new"], _worst["old"] = max(_worst["new"], err_new), max(_worst["old"], err_old)
    err_small = float((old_small.double().cpu() - want).abs().max())
    print(f"ctx0 H={H} C1={C1} d={d}: max|err| new {err_new:.3e}  three launches {err_old:.3e} (as a {B * C1}-row call {err_small:.3e})  "
          f"(worst so far {_worst['new']:.3e} / {_worst['old']:.3e})")
    np.testing.assert_allclose(grouped.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)
    assert err_new <= 2.0 * err_old, (err_new, err_old)
    # an addend joins after the sum
    acc = torch.randn(B, d, device=dev)
    with_acc = _call(L, _lib, c["ue"], c["rg"], G, c, B, H, C1, d, addend=acc)
    torch.cuda.synchronize()
    assert torch.equal(with_acc, acc + grouped)


@pytest.mark.parametrize("H,C1,d,fmt", [(5, 6, 64, None), (50, 18, 400, None), (50, 18, 400, 0), (50, 18, 400, 1)],
                         ids=["d64-fp32", "d400-fp32", "d400-bf16x6", "d400-fp16x3"])      # split images exist for d % 80 == 0 only
def test_ctx0_row_bits_do_not_depend_on_the_call(H, C1, d, fmt):
    """The five rows alone and the same rows inside a 2100-row per-row call give equal rows (the GEMM's row count chooses nothing), in
    the exact fp32 product and on both split images; the image paths hold the 2e-5 bound too."""
    from digat_amd import _lib
    L = _lib.lib()
    dev = _dev()
    c = _case(H, C1, d, seed=7 * H + d)
    want = _reference(c, H, C1, d)
    c = {k: v.to(dev) for k, v in c.items()}
    image = None
    if fmt is not None:
        image = _lib.split_buffer(L.digat_split_weights_bytes(d, d), dev)
        _lib.check(L.digat_split_weights(c["Fa"].data_ptr(), d, d, image.data_ptr(), fmt, _lib.stream_ptr()), "digat_split_weights")
    B, BIG = 5, 2100
    ue5 = c["ue"].index_select(0, c["rg"].long()).contiguous()
    small = _call(L, _lib, ue5, None, 0, c, B, H, C1, d, image=image, fmt=fmt or 0)
    g = torch.Generator(device=dev).manual_seed(5)
    ue = torch.randn(BIG, H, d, device=dev, generator=g)
    kq_t, kq_u = torch.randn(BIG, d, device=dev, generator=g), torch.randn(BIG, d, device=dev, generator=g)
    idx = torch.randint(0, C1, (BIG, H), device=dev, generator=g)
    mask = (torch.rand(BIG, C1, device=dev, generator=g) < 0.6).to(torch.uint8)
    at = torch.tensor([3, 700, 1023, 1024, 2099], device=dev)                  # first / middle / last row tiles of the GEMM
    ue[at], kq_t[at], kq_u[at], idx[at], mask[at] = ue5, c["kq_t"], c["kq_u"], c["idx"], c["mask"]
    big = _call(L, _lib, ue, None, 0, c, BIG, H, C1, d, image=image, fmt=fmt or 0, kq=(kq_t, kq_u), idx=idx, mask=mask)
    torch.cuda.synchronize()
    assert torch.isfinite(big).all()
    assert torch.equal(big[at], small), float((big[at] - small).abs().max())
    print(f"ctx0 bits H={H} d={d} fmt={fmt}: max|err| vs fp64 {float((small.double().cpu() - want).abs().max()):.3e}")
    np.testing.assert_allclose(small.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-5)


def test_ctx0_refuses_what_it_cannot_take():
    from digat_amd import _lib
    L = _lib.lib()
    dev = _dev()
    t = torch.zeros(64, device=dev)
    p = t.data_ptr()
    args = lambda B, H, C1, d, nbytes=1 << 30: (p, None, 0, p, p, p, p, p, p, None, 0, None, p, B, H, C1, d, p, nbytes, None)
    assert L.digat_user_ctx0_fwd(*args(4, 65, 18, 400)) == 2             # DIGAT_ERR_SHAPE: H
    assert L.digat_user_ctx0_fwd(*args(4, 50, 18, 1028)) == 2            # d
    assert L.digat_user_ctx0_fwd(*args(4, 50, 64, 400)) == 2             # the LDS image
    assert L.digat_user_ctx0_fwd(*args(4, 53, 18, 516)) == 2             # the 16-step instantiation's 512 threads
    assert L.digat_user_ctx0_fwd(*args(4, 50, 18, 400, nbytes=16)) == 3  # DIGAT_ERR_WORKSPACE
    assert L.digat_user_ctx0_fwd(*args(0, 50, 18, 400)) == 0             # B == 0: no launch
