"""CPU suite of the quantised first stage: the quantiser's host contract (``evaluate.quantize_rows_host``), the quantised scores within
the derived bound of the real product (``evaluate.qdot_bound``), the two-stage contract on the host twins — where the exact top-k lies
inside the quantised shortlist, the refined list is the exact selection bit for bit —, ``nrms.recommend(index=)`` on CPU tensors, and the
library's symbols."""
import os
import re

import numpy as np
import pytest
import torch

import dot_topk_common as D
import qdot_common as Q
from conftest import REPO


def test_quantiser_contract_on_the_host():
    from digat_amd import evaluate
    for d in (1, 15, 16, 37, 400):
        x = Q.normal(40, 1, d, seed=d)[0]
        q, s = evaluate.quantize_rows_host(x)
        assert q.dtype == np.int8 and s.dtype == np.float32 and q.shape == (40, Q.width(d)) and s.shape == (40,)
        assert not q[:, d:].any(), "zero tail"
        assert (np.abs(q.astype(np.int32)).max(axis=1) == 127).all(), "every non-zero row reaches +-127"
        assert np.array_equal(s, np.abs(x).max(axis=1) / np.float32(127.0))
        # |x - s q| <= s / 2 up to the fp32 rounding of x / s (at most 127 * 2^-24 of a step)
        err = np.abs(x.astype(np.float64) - s.astype(np.float64)[:, None] * q[:, :d])
        assert (err <= s.astype(np.float64)[:, None] * (0.5 + 127 * 2.0 ** -24)).all()
    x = Q.special_rows(37)
    q, s = evaluate.quantize_rows_host(x)
    assert s[1] == 0 and not q[1].any(), "zero row"
    for r in (2, 3, 4):
        assert np.isnan(s[r]) and not q[r].any(), "a row with a NaN or an infinity: codes 0, scale NaN"
    assert q[5, 37 // 3] == -127 and np.count_nonzero(q[5]) == 1 and s[5] == np.float32(2.5) / np.float32(127.0)
    assert s[6] == 0 and not q[6].any(), "amax / 127 underflows: codes 0"
    assert np.isfinite(s[7]) and np.abs(q[7].astype(np.int32)).max() == 127
    assert s[8] == 1.0 and np.array_equal(q[8, :37], np.rint(x[8]).astype(np.int8)) and (q[8, :37] % 2 == 0)[x[8] % 1 != 0].all(), "ties to even"
    with pytest.raises(ValueError, match="QDOT_MAX_D"):
        evaluate.quantize_rows_host(np.zeros((2, 1025), dtype=np.float32))
    # CPU tensors go through the twin
    tq, ts = evaluate.quantize_rows(torch.from_numpy(x))
    assert tq.dtype == torch.int8 and np.array_equal(tq.numpy(), q) and np.array_equal(ts.numpy().view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("G,N,d", [(96, 1000, 64), (96, 8192, 400)])
def test_quantised_scores_stay_within_the_derived_bound(G, N, d):
    """The bound is derived in csrc/digat_qdot.inc, not fitted: the worst ratio seen is about 0.3 at d = 64 and 0.15 at d = 400."""
    from digat_amd import evaluate
    u, v, qu, su, qn, sn = Q.coded(G, N, d)
    S = evaluate.qdot_scores_host(qu, su, qn, sn)
    assert S.dtype == np.float32 and S.shape == (G, N)
    exact = u.astype(np.float64) @ v.astype(np.float64).T
    ratio = np.abs(S.astype(np.float64) - exact) / evaluate.qdot_bound(u, v, su, sn)
    print("worst |quantised - exact| / bound at G=%d N=%d d=%d: %.3f" % (G, N, d, ratio.max()))
    assert ratio.max() <= 1.0
    # the bits: the exact integer product, two fp32 multiplications from left to right
    acc = qu[:7].astype(np.int64) @ qn[:50].astype(np.int64).T
    want = (acc.astype(np.float32) * su[:7, None]) * sn[None, :50]
    assert np.array_equal(S[:7, :50].view(np.uint32), want.view(np.uint32))
    # a pool: positions are ids; an id outside [0, N) holds +0.0
    pool = np.array([5, N - 1, -1, 0, N, 5], dtype=np.int64)
    P = evaluate.qdot_scores_host(qu, su, qn, sn, pool)
    assert np.array_equal(P[:, [0, 1, 3, 5]].view(np.uint32), S[:, [5, N - 1, 0, 5]].view(np.uint32))
    assert not P[:, [2, 4]].view(np.uint32).any()


@pytest.mark.parametrize("G,N,d", [(96, 1000, 64), (96, 8192, 400)])
@pytest.mark.parametrize("M", [32, 64])
def test_two_stage_contract_on_the_host_twins(G, N, d, M):
    from digat_amd import evaluate
    k = 10
    u, v, qu, su, qn, sn = Q.coded(G, N, d)
    rng = np.random.default_rng(1)
    pool = rng.permutation(N)[: N - 7].astype(np.int64)
    skip = pool[rng.integers(0, len(pool), size=(G, 20))]
    tu, tv = torch.from_numpy(u), torch.from_numpy(v)
    with torch.no_grad():                                   # the brute force of the CPU path: one fp32 sum per pair
        rows = tv[pool]
        S = torch.stack([(rows * tu[g]).sum(dim=1) for g in range(G)]).numpy()
    es, ei, ec = evaluate.dot_topk_host(S, k, pool=pool, skip=skip)
    qs, qi, qc = (t.numpy() for t in evaluate.qdot_shortlist(*map(torch.from_numpy, (qu, su, qn, sn)), M, pool=torch.from_numpy(pool),
                                                             skip=torch.from_numpy(skip)))
    want = evaluate.dot_shortlist_host(evaluate.qdot_scores_host(qu, su, qn, sn, pool), M, pool=pool, skip=skip)
    assert np.array_equal(qi, want[1]) and np.array_equal(qc, want[2]) and np.array_equal(qs.view(np.uint32), want[0].view(np.uint32))
    inside = Q.contained(ei, ec, qi, qc)
    print("containment at N=%d d=%d M=%d: %.4f" % (N, d, M, inside.mean()))
    assert inside.mean() >= 0.98, "a condition of the test, not a measurement"
    # the lists in pool order, as nrms.recommend hands them over: exact ties then go by pool position
    where = np.full(N + 1, len(pool), dtype=np.int64)
    where[pool[::-1]] = np.arange(len(pool) - 1, -1, -1)
    order = np.argsort(where[np.where(qi >= 0, qi, N)], axis=1, kind="stable")
    rs, ri, rc = (t.numpy() for t in evaluate.refine_lists(tu, tv, torch.from_numpy(np.take_along_axis(qi, order, axis=1)),
                                                           torch.from_numpy(qc), k))
    assert np.array_equal(rc[inside], ec[inside]) and np.array_equal(ri[inside], ei[inside])
    assert np.array_equal(rs[inside].view(np.uint32), es[inside].view(np.uint32))
    assert (rc == np.minimum(qc, k)).all()


def test_refine_lists_skips_what_is_no_element():
    from digat_amd import evaluate
    u, v = (torch.from_numpy(a) for a in Q.normal(3, 20, 8, seed=2))
    ids = torch.tensor([[4, 7, -1, 20, 9, 4], [1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0]])
    count = torch.tensor([6, 2, 0], dtype=torch.int32)
    s, i, c = evaluate.refine_lists(u, v, ids, count, 4)
    assert c.tolist() == [4, 2, 0] and sorted(i[0].tolist()) == [4, 4, 7, 9] and sorted(i[1, :2].tolist()) == [1, 2]
    assert (i[1, 2:] == -1).all() and torch.isneginf(s[1, 2:]).all() and (i[2] == -1).all()
    want = (v[i[0]] * u[0]).sum(dim=1)
    assert torch.equal(s[0], want) and (s[0, :-1] >= s[0, 1:]).all()
    with pytest.raises(ValueError, match="k must be"):
        evaluate.refine_lists(u, v, ids, count, 129)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_an_index_on_cpu_tensors(pre):
    from digat_amd import nrms
    k = 5
    m, dev, inp = D.model(pre), D.dev_set(), D.inputs()
    users = np.arange(D.USERS)
    S = D.stock_scores(m, dev)
    hist, mask = inp["history_ids"], inp["history_mask"]
    index = nrms.build_index(m, dev)
    assert index.news_num == D.NEWS and index.codes.dtype == torch.int8 and index.codes.shape[1] % 16 == 0
    plain = nrms.recommend(m, dev, users, k=k)
    want = [D.brute_force(S[g], range(1, D.NEWS), D.banned_ids(hist[g], mask[g]), k) for g in users]
    D.check_rows(*plain, want, k)
    for refine in (None, 16, 40):
        M = refine or 64
        qi, qs, qc = nrms.shortlist(m, dev, users, m=M, index=index)
        inside = Q.contained(plain[0].numpy(), plain[2].numpy(), qi.numpy(), qc.numpy())
        assert inside.mean() >= 0.98 if M >= 40 else inside.any(), (M, inside.mean())
        ids, scores, count = nrms.recommend(m, dev, users, k=k, index=index, refine=refine)
        keep = np.flatnonzero(inside)
        D.check_rows(ids[keep], scores[keep], count[keep], [want[g] for g in keep], k)
    # a pool in another order, the history kept in, and the refusals
    pool = np.random.default_rng(4).permutation(np.arange(1, D.NEWS))[:70]
    a = nrms.recommend(m, dev, users, candidates=pool, k=k, exclude_history=False)
    b = nrms.recommend(m, dev, users, candidates=pool, k=k, exclude_history=False, index=index, refine=70)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the whole pool is the shortlist: the exact call"
    csr = (np.tile(pool, D.USERS), np.arange(D.USERS + 1, dtype=np.int64) * len(pool))
    with pytest.raises(ValueError, match="shared by all users"):
        nrms.recommend(m, dev, users, candidates=csr, k=k, index=index)
    with pytest.raises(ValueError, match="refine belongs"):
        nrms.recommend(m, dev, users, k=k, refine=32)
    with pytest.raises(ValueError, match="refine must lie"):
        nrms.recommend(m, dev, users, k=k, index=index, refine=3)
    with pytest.raises(ValueError, match="does not combine with index"):
        nrms.recommend(m, dev, users, k=k, index=index, calibration=0.5)
    div = nrms.recommend(m, dev, users, candidates=pool, k=k, exclude_history=False, diversity=0.3, index=index, refine=70)
    assert all(torch.equal(x, y) for x, y in zip(div, nrms.recommend(m, dev, users, candidates=pool, k=k, exclude_history=False, diversity=0.3)))
    rows = nrms.index_report(m, dev, users, k=k, ms=(8, 64), index=index, replicates=50)
    assert [r["m"] for r in rows] == [8, 64] and rows[0]["containment"] <= rows[1]["containment"] and rows[1]["containment"] >= 0.98
    assert all(0.0 <= r["agreement"] <= 1.0 and r["containment"] <= r["agreement"] + 1e-12 for r in rows)


def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in Q.NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+DIGAT_QDOT_MAX_D\s+(\d+)", header).group(1)) == evaluate.QDOT_MAX_D == 1024
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_shortlist.inc"') < hip.index('#include "digat_qdot.inc"')         # it uses both selections
    assert L.digat_qdot_topk_workspace_bytes(100, 5000, 10) == L.digat_dot_topk_workspace_bytes(100, 5000, 10) > 0
    assert L.digat_qdot_shortlist_workspace_bytes(100, 5000, 300, 64) == L.digat_dot_shortlist_workspace_bytes(100, 5000, 300, 64) > 0
    assert L.digat_qdot_shortlist_workspace_bytes(100, 5000, 1025, 64) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Host memory stands in for the device pointers: every refusal below is decided before a launch, so nothing reads it."""
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    G, N, d = 4, 32, 40
    dq = Q.width(d)
    qu, qn = torch.zeros((G, dq), dtype=torch.int8), torch.zeros((N, dq), dtype=torch.int8)
    su, sn, x = torch.ones(G), torch.ones(N), torch.zeros((G, d))
    out_s, out_i, out_c = torch.zeros((G, 1024)), torch.zeros((G, 1024), dtype=torch.int64), torch.zeros(G, dtype=torch.int32)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)
    assert qu.data_ptr() % 16 == 0 and qn.data_ptr() % 16 == 0
    quant = lambda d_, dq_, x_=x, q_=qu, s_=su: L.digat_quantize_rows_i8(_lib.ptr(x_), G, d_, dq_, _lib.ptr(q_), _lib.ptr(s_), None)
    assert quant(d, dq + 16) == Q.ARG and quant(d, d) == Q.ARG and quant(1025, 1040) == Q.SHAPE and quant(0, 0) == Q.ARG
    assert quant(d, dq, x_=None) == Q.ARG and quant(d, dq, q_=None) == Q.ARG and quant(d, dq, s_=None) == Q.ARG
    head = lambda d_=d, dq_=dq, qu_=qu, sn_=sn: (_lib.ptr(qu_), su.data_ptr(), qn.data_ptr(), _lib.ptr(sn_), None, G, N, N, d_, dq_)
    scores = lambda **kw: L.digat_qdot_scores(*head(**kw), out_s.data_ptr(), None)
    assert scores(d_=1025, dq_=1040) == Q.SHAPE and scores(dq_=dq + 16) == Q.ARG and scores(qu_=None) == Q.ARG and scores(sn_=None) == Q.ARG
    assert L.digat_qdot_scores(*head(), None, None) == Q.ARG
    assert L.digat_qdot_scores(qu.data_ptr() + 1, su.data_ptr(), qn.data_ptr(), sn.data_ptr(), None, G, N, N, d, dq, out_s.data_ptr(), None) == Q.ARG
    outs = (out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())
    topk = lambda k, w=ws, nbytes=None, **kw: L.digat_qdot_topk(*head(**kw), None, 0, k, *outs, _lib.ptr(w),
                                                                 ws.numel() if nbytes is None else nbytes, None)
    assert topk(129) == Q.ARG and topk(0) == Q.ARG and topk(10, d_=1025, dq_=1040) == Q.SHAPE and topk(10, dq_=dq + 16) == Q.ARG
    assert topk(10, w=None) == Q.ARG and topk(10, nbytes=L.digat_qdot_topk_workspace_bytes(G, N, 10) - 1) == Q.WORKSPACE
    short = lambda m, w=ws, nbytes=None, **kw: L.digat_qdot_shortlist(*head(**kw), None, 0, m, 2, *outs, _lib.ptr(w),
                                                                       ws.numel() if nbytes is None else nbytes, None)
    assert short(1025) == Q.ARG and short(0) == Q.ARG and short(200, d_=1025, dq_=1040) == Q.SHAPE and short(200, dq_=dq + 16) == Q.ARG
    assert short(200, w=None) == Q.ARG and short(200, nbytes=L.digat_qdot_shortlist_workspace_bytes(G, N, 200, 2) - 1) == Q.WORKSPACE
    # nothing to do: no launch, no error
    assert L.digat_quantize_rows_i8(x.data_ptr(), 0, d, dq, qu.data_ptr(), su.data_ptr(), None) == Q.OK
    assert L.digat_qdot_scores(qu.data_ptr(), su.data_ptr(), qn.data_ptr(), sn.data_ptr(), None, 0, N, N, d, dq, out_s.data_ptr(), None) == Q.OK
