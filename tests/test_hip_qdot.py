"""GPU suite of the quantised first stage, every comparison exact: the quantiser against its numpy twin byte for byte; the orientation
of the int8 product on asymmetric integer data; ``qdot_scores`` against ``qdot_scores_host`` across the sub-tile, chunk and K-block
boundaries; ``qdot_topk`` / ``qdot_shortlist`` against the host selection on the kernel's own scores; the independence of the bits
from the entry, the pool order and the call; the refusals; ``refine_lists`` and ``nrms.recommend(index=)`` on the device."""
import numpy as np
import pytest
import torch

import dot_topk_common as D
import qdot_common as Q

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    s, i, c = (t.cpu().numpy() for t in got)
    assert np.array_equal(c, want[2]), (what, "count", c.tolist(), np.asarray(want[2]).tolist())
    assert np.array_equal(i, want[1]), (what, "ids", np.argwhere(i != want[1])[:5].tolist())
    assert np.array_equal(_bits(s), _bits(want[0])), (what, "score bits")


def _raw_scores(qu, su, qn, sn, pool, G, N, P):
    """digat_qdot_scores itself: the Python entry refuses pools with ids outside [0, N), the library defines them."""
    from digat_amd import _lib
    out = torch.full((G * P + 64,), 123.0, dtype=torch.float32, device=_dev())
    dq = int(qu.shape[1])
    _lib.check(_lib.lib().digat_qdot_scores(qu.data_ptr(), su.data_ptr(), qn.data_ptr(), sn.data_ptr(), _lib.ptr(pool), G, N, P, dq, dq,
                                            out.data_ptr(), _lib.stream_ptr()), "digat_qdot_scores")
    assert (out[G * P:] == 123.0).all(), "nothing is written beyond [G, P]"
    return out[:G * P].view(G, P)


@pytest.mark.parametrize("d", [1, 15, 16, 37, 64, 65, 400, 1024])
def test_quantiser_matches_the_twin_byte_for_byte(d):
    from digat_amd import evaluate
    for R in (1, 63, 130):
        x = np.concatenate([Q.normal(130, 1, d, seed=d)[0][:R] * np.float32(3.7), Q.special_rows(d)])
        q, s = evaluate.quantize_rows(_t(x))
        wq, ws = evaluate.quantize_rows_host(x)
        assert q.dtype == torch.int8 and tuple(q.shape) == (len(x), Q.width(d)) and s.dtype == torch.float32
        assert np.array_equal(q.cpu().numpy(), wq), (R, np.argwhere(q.cpu().numpy() != wq)[:5].tolist())
        assert np.array_equal(_bits(s), ws.view(np.uint32)), R


def test_orientation_on_asymmetric_integer_data():
    from digat_amd import evaluate
    G, P, d = 70, 130, 100
    users, news, acc = Q.oriented(G, P, d)
    qu, su = evaluate.quantize_rows(_t(users))
    qn, sn = evaluate.quantize_rows(_t(news))
    assert np.array_equal(qn.cpu().numpy()[:, :d], news.astype(np.int8)) and (sn == 1.0).all(), "the news round-trip the quantiser"
    assert np.array_equal(qu.cpu().numpy()[:, :d], (np.sign(users) * 127).astype(np.int8))
    assert np.array_equal(_bits(su), ((np.arange(G) + 1).astype(np.float32) / np.float32(127.0)).view(np.uint32))
    want = (acc.astype(np.float32) * su.cpu().numpy()[:, None]) * np.float32(1.0)
    S = evaluate.qdot_scores(qu, su, qn, sn)
    assert np.array_equal(_bits(S), want.view(np.uint32)), np.argwhere(_bits(S) != want.view(np.uint32))[:5].tolist()
    assert not np.array_equal(acc[:, :G], acc[:, :G].T), "the data tell rows from columns"


@pytest.mark.parametrize("d", [1, 37, 64, 100, 400, 1024])
def test_scores_match_the_twin_across_every_boundary(d):
    from digat_amd import evaluate
    NMAX = 4100 + 37
    u, v, qu, su, qn, sn = Q.coded(130, NMAX, d, seed=d)
    tqu, tsu, tqn, tsn = (_t(a) for a in (qu, su, qn, sn))
    rng = np.random.default_rng(d)
    for P in (1, 63, 64, 65, 2049, 4100):
        for G in (1, 65, 130):
            if P > 65 and G == 65 and d not in (37, 400):
                continue                                    # the middle G at the long pools: two widths are enough
            S = evaluate.qdot_scores(tqu[:G].contiguous(), tsu[:G].contiguous(), tqn[:P].contiguous(), tsn[:P].contiguous())
            want = evaluate.qdot_scores_host(qu[:G], su[:G], qn[:P], sn[:P])
            assert np.array_equal(_bits(S), want.view(np.uint32)), ("no pool", G, P, np.argwhere(_bits(S) != want.view(np.uint32))[:5].tolist())
            N = P + 37
            pool = rng.permutation(N)[:P].astype(np.int64)
            pool[rng.integers(0, P, size=max(1, P // 9))] = rng.choice(np.array([-1, N, N + 5, -(2 ** 40), 2 ** 40]), size=max(1, P // 9))
            S = _raw_scores(tqu[:G].contiguous(), tsu[:G].contiguous(), tqn[:N].contiguous(), tsn[:N].contiguous(), _t(pool), G, N, P)
            want = evaluate.qdot_scores_host(qu[:G], su[:G], qn[:N], sn[:N], pool)
            assert np.array_equal(_bits(S), want.view(np.uint32)), ("pool", G, P, np.argwhere(_bits(S) != want.view(np.uint32))[:5].tolist())


def _select_case(kind, G, N, P, d, seed):
    """``(qu, su, qn, sn, pool, skip)`` as numpy: random or tie-heavy vectors, two users and some news with a NaN (scale NaN), a
    permuted pool with repeats, 50-entry skip rows drawn from the pool."""
    from digat_amd import evaluate
    rng = np.random.default_rng(seed)
    u, v = (Q.tied(G, N, d, seed) if kind == "tied" else tuple(a.copy() for a in Q.normal(G, N, d, seed)))
    u[G // 2, 0] = np.nan
    v[rng.integers(0, N, size=5), d - 1] = np.nan
    v[rng.integers(0, N, size=3)] = 0
    qu, su = evaluate.quantize_rows_host(u)
    qn, sn = evaluate.quantize_rows_host(v)
    pool = rng.integers(0, N, size=P).astype(np.int64)
    skip = pool[rng.integers(0, P, size=(G, 50))]
    return qu, su, qn, sn, pool, skip


@pytest.mark.parametrize("kind", ["normal", "tied"])
def test_selection_is_exact_on_the_kernels_own_scores(kind):
    from digat_amd import evaluate
    G, N, P, d = 70, 4200, 4100, 37                          # two user tiles, three chunks of 2 048, level 1 of the long selection
    qu, su, qn, sn, pool, skip = _select_case(kind, G, N, P, d, 11)
    T = tuple(_t(a) for a in (qu, su, qn, sn))
    S = evaluate.qdot_scores(*T, pool=_t(pool)).cpu().numpy()
    assert np.array_equal(S.view(np.uint32), evaluate.qdot_scores_host(qu, su, qn, sn, pool).view(np.uint32))
    if kind == "tied":
        assert max(len(np.unique(S[g][~np.isnan(S[g])])) for g in range(G)) <= 2 * d + 1, "many equal scores: ties resolve by position"
    assert np.isnan(S[G // 2]).all() and np.isnan(S[0]).any()
    for sk in (None, skip):
        for k in (1, 10, 128):
            _same(evaluate.qdot_topk(*T, k, pool=_t(pool), skip=_t(sk)), evaluate.dot_topk_host(S, k, pool=pool, skip=sk), ("topk", k, sk is None))
        for m in (129, 1024):
            _same(evaluate.qdot_shortlist(*T, m, pool=_t(pool), skip=_t(sk), slab_users=48),
                  evaluate.dot_shortlist_host(S, m, pool=pool, skip=sk), ("shortlist", m, sk is None))
    # without a pool: positions are ids (P = N); a short pool: level 2 of the long selection alone
    S = evaluate.qdot_scores(*T).cpu().numpy()
    _same(evaluate.qdot_topk(*T, 10, skip=_t(skip)), evaluate.dot_topk_host(S, 10, skip=skip), "topk, no pool")
    _same(evaluate.qdot_shortlist(*T, 129, skip=_t(skip), slab_users=64), evaluate.dot_shortlist_host(S, 129, skip=skip), "shortlist, no pool")
    few = pool[:300]
    S = evaluate.qdot_scores(*T, pool=_t(few)).cpu().numpy()
    _same(evaluate.qdot_shortlist(*T, 1024, pool=_t(few), slab_users=33), evaluate.dot_shortlist_host(S, 1024, pool=few), "short pool")
    _same(evaluate.qdot_topk(*T, 128, pool=_t(few)), evaluate.dot_topk_host(S, 128, pool=few), "short pool, topk")


def test_empty_calls():
    from digat_amd import _lib, evaluate
    qu, su, qn, sn, pool, skip = _select_case("normal", 5, 40, 30, 20, 3)
    T = tuple(_t(a) for a in (qu, su, qn, sn))
    none = _t(np.zeros(0, dtype=np.int64))
    for got in (evaluate.qdot_topk(*T, 10, pool=none), evaluate.qdot_shortlist(*T, 200, pool=none)):
        assert got[2].tolist() == [0] * 5 and (got[1] == -1).all() and torch.isneginf(got[0]).all()
    assert tuple(evaluate.qdot_scores(*T, pool=none).shape) == (5, 0)
    E = (T[0][:0], T[1][:0], T[2], T[3])
    assert tuple(evaluate.qdot_topk(*E, 10)[1].shape) == (0, 10) and tuple(evaluate.qdot_shortlist(*E, 200)[1].shape) == (0, 200)
    assert tuple(evaluate.quantize_rows(_t(np.zeros((0, 20), dtype=np.float32)))[0].shape) == (0, 32)
    # the library itself: P == 0 sets every count to 0 and fills the rows, without a workspace
    L, G = _lib.lib(), 5
    out_s, out_i = torch.zeros((G, 10), device=_dev()), torch.zeros((G, 10), dtype=torch.int64, device=_dev())
    out_c = torch.full((G,), 9, dtype=torch.int32, device=_dev())
    one = _t(np.zeros(1, dtype=np.int64))                     # a pool pointer that is not null; P = 0 reads nothing of it
    head = (T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), T[3].data_ptr(), one.data_ptr(), G, 40, 0, 32, 32, None, 0, 10)
    outs = (out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr())
    _lib.check(L.digat_qdot_topk(*head, *outs, None, 0, _lib.stream_ptr()), "digat_qdot_topk")
    assert out_c.tolist() == [0] * G and (out_i == -1).all() and torch.isneginf(out_s).all()
    out_c.fill_(9)
    _lib.check(L.digat_qdot_shortlist(*head, 2, *outs, None, 0, _lib.stream_ptr()), "digat_qdot_shortlist")
    assert out_c.tolist() == [0] * G and (out_i == -1).all() and torch.isneginf(out_s).all()


def test_bits_do_not_depend_on_the_entry_the_pool_order_or_the_call():
    from digat_amd import evaluate
    G, N, d = 70, 2300, 100
    qu, su, qn, sn, _, _ = _select_case("normal", G, N, N, d, 13)
    T = tuple(_t(a) for a in (qu, su, qn, sn))
    rng = np.random.default_rng(2)
    base = evaluate.qdot_scores(*T)
    again = evaluate.qdot_scores(*T)
    assert torch.equal(base.view(torch.int32), again.view(torch.int32)), "two calls"
    perm = rng.permutation(N).astype(np.int64)
    moved = evaluate.qdot_scores(*T, pool=_t(perm))
    assert torch.equal(moved.view(torch.int32), base[:, _t(perm)].view(torch.int32)), "another pool order: other tiles, the same bits"
    alone = evaluate.qdot_scores(T[0][33:34].contiguous(), T[1][33:34].contiguous(), T[2], T[3], pool=_t(perm[:17]))
    assert torch.equal(alone.view(torch.int32), base[33:34, _t(perm[:17])].view(torch.int32)), "one user, a short pool"
    Sb = base.cpu().numpy()
    for pl in (None, perm):
        a = evaluate.qdot_topk(*T, 128, pool=_t(pl))
        b = evaluate.qdot_shortlist(*T, 128, pool=_t(pl), slab_users=40)
        c = evaluate.qdot_shortlist(*T, 128, pool=_t(pl))
        a2 = evaluate.qdot_topk(*T, 128, pool=_t(pl))
        for other in (b, c, a2):
            assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                       for x, y in zip(a, other)), "the fused entry, the slab entry at two slabs, a second call"
        ids, cnt = a[1].cpu().numpy(), a[2].cpu().numpy()
        for g in (0, 34, 69):
            assert np.array_equal(_bits(a[0][g, :cnt[g]]), Sb[g, ids[g, :cnt[g]]].view(np.uint32)), "the bits qdot_scores stores"


def test_python_entries_refuse_bad_arguments():
    from digat_amd import evaluate
    qu, su, qn, sn, pool, skip = _select_case("normal", 5, 40, 30, 20, 3)
    T = tuple(_t(a) for a in (qu, su, qn, sn))
    with pytest.raises(ValueError, match="k must be"):
        evaluate.qdot_topk(*T, 129)
    with pytest.raises(ValueError, match="m must be"):
        evaluate.qdot_shortlist(*T, 1025)
    with pytest.raises(ValueError, match="pool ids"):
        evaluate.qdot_topk(*T, 5, pool=_t(np.array([0, 40], dtype=np.int64)))
    with pytest.raises(ValueError, match="int8 codes of one width"):
        evaluate.qdot_scores(T[0][:, :16].contiguous(), T[1], T[2], T[3])
    with pytest.raises(ValueError, match="multiple of 16"):
        evaluate.qdot_scores(T[0][:, :20].contiguous(), T[1], T[2][:, :20].contiguous(), T[3])
    with pytest.raises(ValueError, match="QDOT_MAX_D"):
        evaluate.quantize_rows(torch.zeros((2, 1025), device=_dev()))
    with pytest.raises(ValueError, match="skip must be"):
        evaluate.qdot_topk(*T, 5, skip=_t(skip[:2]))


def test_refine_lists_is_dot_scores_and_topk_segments():
    from digat_amd import evaluate
    G, N, d, M, k = 70, 900, 100, 150, 10
    u, v, qu, su, qn, sn = Q.coded(G, N, d, seed=21)
    U, V = _t(u), _t(v)
    _, ids, count = evaluate.qdot_shortlist(_t(qu), _t(su), _t(qn), _t(sn), M, pool=_t(np.arange(1, 140, dtype=np.int64)))      # 139 < M: a fill
    assert int(count.max()) == 139
    ids[3, 5] = N + 4                                         # no element
    S = evaluate.dot_scores(U, V)
    elem = evaluate.list_elements(ids, count, N)
    flat = torch.where(elem, ids, torch.full_like(ids, -1))
    picked = torch.gather(S, 1, torch.where(elem, ids, torch.zeros_like(ids)))
    want = evaluate.topk_segments(picked.reshape(-1), torch.arange(G + 1, device=_dev()) * M, k, ids=flat.reshape(-1),
                                  skip=torch.full((G, 1), -1, dtype=torch.int64, device=_dev()))
    got = evaluate.refine_lists(U, V, ids, count, k)
    _same(got, tuple(t.cpu().numpy() for t in want), "refine_lists")
    assert got[2].tolist() == [k] * G and not (got[1][3] == N + 4).any()


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_an_index_on_the_device(pre):
    from digat_amd import nrms
    k = 5
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users = np.arange(D.USERS)
    plain = nrms.recommend(m, dev, users, k=k, batch_size=4)
    index = nrms.build_index(m, dev, batch_size=4)
    assert index.codes.is_cuda and index.codes.dtype == torch.int8 and index.news_num == D.NEWS
    again = nrms.recommend(m, dev, users, k=k, batch_size=4, index=None)
    assert all(torch.equal(x, y) for x, y in zip(plain, again)), "index=None is the call as it was"
    for refine, M in ((None, 64), (40, 40), (129, 129)):
        qi, qs, qc = nrms.shortlist(m, dev, users, m=M, index=index, batch_size=4)
        inside = Q.contained(plain[0].cpu().numpy(), plain[2].cpu().numpy(), qi.cpu().numpy(), qc.cpu().numpy())
        assert inside.mean() >= 0.98, (M, inside.mean())
        ids, scores, count = nrms.recommend(m, dev, users, k=k, batch_size=4, index=index, refine=refine)
        keep = torch.from_numpy(np.flatnonzero(inside)).to(_dev())
        assert torch.equal(ids[keep], plain[0][keep]) and torch.equal(count[keep], plain[2][keep])
        assert torch.equal(scores[keep].view(torch.int32), plain[1][keep].view(torch.int32)), "exact scores: dot_scores' bits"
    # the quantised lists carry quantised scores: qdot_scores' bits of the same users and codes
    user = nrms.user_vectors(m, dev, users, batch_size=4)
    from digat_amd import evaluate
    qu, su = evaluate.quantize_rows(user)
    S = evaluate.qdot_scores(qu, su, index.codes, index.scales)
    assert torch.equal(qs[:, :5].view(torch.int32), torch.gather(S, 1, qi[:, :5]).view(torch.int32))
    rows = nrms.index_report(m, dev, users, k=k, ms=(8, 64), index=index, replicates=50)
    assert rows[1]["containment"] >= 0.98 and rows[0]["agreement"] <= rows[1]["agreement"]
