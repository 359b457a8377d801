"""GPU suite: the fused inner-product + rank-of-target kernel (``digat_dot_rank``) and ``nrms.retrieval_metrics`` on it.  A rank is an
integer count over scores whose bits do not depend on who computes them, so everything here is held exactly: to the host contract
(``evaluate.dot_rank_host``) on the kernel's own scores (``digat_dot_scores``), and to the fused top-k's lists."""
import numpy as np
import pytest
import torch

import dot_rank_common as R
import dot_topk_common as D

pytestmark = pytest.mark.gpu

PER_USER = (0, 1, 5, 70)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def _case(rng, G, P, d, pool, skip, integers):
    N = P + 37 if pool else P
    draw = (lambda shape: rng.integers(-2, 3, size=shape).astype(np.float32)) if integers else \
        (lambda shape: rng.standard_normal(shape).astype(np.float32))
    users, news = draw((G, d)), draw((N, d))
    pl = rng.integers(0, N, size=P).astype(np.int64) if pool else None                   # unsorted, with repeats
    sk = None
    if skip:
        src = pl if pool else np.arange(P, dtype=np.int64)
        sk = np.stack([src[rng.integers(0, P, size=50)] for _ in range(G)])              # 50 wide, with repeats
    return users, news, pl, sk


def _own(users, news, pos, start, pool, skip, what):
    """dot_rank against the host contract on dot_scores of the same arguments: ranks, and the targets' score bits."""
    from digat_amd import evaluate
    rank, score = evaluate.dot_rank(_t(users), _t(news), _t(pos), start, pool=_t(pool), skip=_t(skip))
    assert rank.dtype == torch.int32 and score.dtype == torch.float32 and rank.shape == score.shape == (len(pos),)
    S = evaluate.dot_scores(_t(users), _t(news), pool=_t(pool)).cpu().numpy()
    want = evaluate.dot_rank_host(S, pos, start, pool=pool, skip=skip)
    rank, score = rank.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(rank, want), (what, np.flatnonzero(rank != want)[:5].tolist(), rank[rank != want][:5].tolist(),
                                        want[rank != want][:5].tolist())
    owner = np.repeat(np.arange(len(start) - 1), np.diff(start))
    ok = want >= 0
    assert np.array_equal(_bits(score[ok]), _bits(S[owner[ok], pos[ok]])), (what, "score bits")
    assert np.isnan(score[~ok]).all(), (what, "a target without a rank has a NaN score")
    return rank, S


SWEEP = ((1, 1, 1), (63, 3, 20), (64, 65, 37), (65, 1, 400), (2047, 3, 1), (2048, 65, 20), (2049, 1, 37), (4097, 65, 400))


def test_the_sweep_covers_what_it_should():
    from digat_amd import evaluate
    ch, sub, tile = evaluate.DOT_TOPK_CHUNK, evaluate.DOT_TOPK_SUB, evaluate.DOT_TOPK_USERS
    assert [p for p, _, _ in SWEEP] == [1, sub - 1, sub, sub + 1, ch - 1, ch, ch + 1, 2 * ch + 1]
    assert {g for _, g, _ in SWEEP} == {1, 3, tile + 1} and {d for _, _, d in SWEEP} == {1, 20, 37, 400}
    assert SWEEP[-1][1] > tile and -(-SWEEP[-1][0] // ch) == 3, "the largest case: two user tiles by three chunks"


@pytest.mark.parametrize("P,G,d", SWEEP)
def test_ranks_are_exact_on_the_kernels_own_scores(P, G, d):
    from digat_amd import evaluate
    rng = np.random.default_rng(P)
    n = [p for p, _, _ in SWEEP].index(P)
    for pool in (False, True):
        for skip in (False, True):
            users, news, pl, sk = _case(rng, G, P, d, pool, skip, integers=(n % 2 == 0))
            pos, start = R.make_targets(rng, G, P, PER_USER[n % 4:] + PER_USER[:n % 4], evaluate.DOT_TOPK_CHUNK)
            assert {0, P - 1} <= set(pos.tolist())
            rank, _ = _own(users, news, pos, start, pl, sk, (G, P, d, pool, skip))
            if not skip:
                assert (rank >= 0).all()
            n += 1


@pytest.mark.parametrize("skip", [False, True])
def test_rank_below_k_is_the_slot_in_the_fused_top_k(skip):
    """Integers in [-3, 3], d = 100: every partial sum is exact and ties are everywhere.  Every position is a target."""
    from digat_amd import evaluate
    rng = np.random.default_rng(21)
    G, P, d = 3, evaluate.DOT_TOPK_CHUNK + 1, 100
    u = rng.integers(-3, 4, size=(G, d)).astype(np.float32)
    v = rng.integers(-3, 4, size=(P, d)).astype(np.float32)
    sk = np.stack([rng.integers(0, P, size=50) for _ in range(G)]).astype(np.int64) if skip else None
    pos, start = np.tile(np.arange(P, dtype=np.int64), G), np.arange(G + 1, dtype=np.int64) * P
    rank, S = _own(u, v, pos, start, None, sk, "every position")
    assert np.array_equal(S, u @ v.T) and len(np.unique(S)) < 400
    rank = rank.reshape(G, P)
    for g in range(G):
        elements = P - (len(np.unique(sk[g])) if skip else 0)
        assert sorted(rank[g][rank[g] >= 0].tolist()) == list(range(elements)), "a permutation of the elements"
    for k in (1, 10, 128):
        top_s, top_i, top_c = (t.cpu().numpy() for t in evaluate.dot_topk(_t(u), _t(v), k, skip=_t(sk)))
        assert (top_c == k).all()
        for g in range(G):
            inside = np.flatnonzero((rank[g] >= 0) & (rank[g] < k))
            assert len(inside) == k
            assert np.array_equal(top_i[g, rank[g, inside]], inside), (k, g)             # no pool: the id is the position
            assert np.array_equal(_bits(top_s[g, rank[g, inside]]), _bits(S[g, inside]))


def test_specials_follow_the_host_contract():
    rng = np.random.default_rng(4)
    d, N = 20, 300
    v = rng.standard_normal((N, d)).astype(np.float32)
    v[10], v[20], v[30], v[40] = np.nan, np.inf, -np.inf, 0.0
    v[50, 3] = np.nan
    u = rng.standard_normal((6, d)).astype(np.float32)
    u[0] = -0.0
    u[1] = np.abs(u[1])                                   # +inf and -inf scores; mixed signs give inf - inf = NaN
    u[2] = 0.0
    # user 3: only the last channel counts, and -1e-30 * 1e-30 underflows to -0.0 where -1e-30 * -1e-30 and -1e-30 * 0 + 0 give +0.0
    u[3] = 0.0
    u[3, d - 1] = -1e-30
    v[60, d - 1], v[61, d - 1], v[62, d - 1] = 1e-30, -1e-30, 0.0
    pos, start = np.tile(np.arange(N, dtype=np.int64), 6), np.arange(7, dtype=np.int64) * N
    rank, S = _own(u, v, pos, start, None, None, "specials")
    rank = rank.reshape(6, N)
    assert np.isnan(S[:, 10]).all() and np.isposinf(S[1, 20]) and np.isneginf(S[1, 30]) and np.isnan(S[0, 20])
    # a NaN target ranks behind every number (-inf included) and in position order among NaNs
    assert np.isnan(S[1]).sum() == 2 and rank[1, 20] == 0 and rank[1, 30] == N - 3 and rank[1, 10] == N - 2 and rank[1, 50] == N - 1
    nan0 = np.flatnonzero(np.isnan(S[0]))
    assert set(nan0.tolist()) == {10, 20, 30, 50} and rank[0, nan0].tolist() == [N - 4, N - 3, N - 2, N - 1]
    assert rank[0, ~np.isnan(S[0])].tolist() == list(range(N - 4)), "all zeros: position order"
    # a -0.0 and a +0.0 score tie by position
    assert _bits(S[3, 60:63]).tolist() == [0x80000000, 0, 0], "the product gives a negative zero"
    zeros = np.flatnonzero(S[3] == 0)
    assert {40, 60, 61, 62} <= set(zeros.tolist())
    assert (np.diff(rank[3, zeros]) == 1).all(), "signed zeros are one tie, in position order"
    assert rank[3, zeros[0]] == int((S[3] > 0).sum())
    for g in range(6):
        assert sorted(rank[g].tolist()) == list(range(N))


def test_targets_that_are_no_elements():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(9)
    G, N, d = 3, 500, 20
    u = rng.integers(-2, 3, size=(G, d)).astype(np.float32)
    v = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    few = rng.permutation(N)[:40].astype(np.int64)
    P = len(few)
    skip = rng.integers(0, N, size=(G, 64)).astype(np.int64)
    skip[0], skip[0, 7] = few[4], few[17]                           # user 0: positions 4 and 17 skipped, nothing else (a repeated entry)
    skip[1, :40], skip[1, 40:] = few, few[0]                        # user 1: every id skipped
    pos = np.r_[np.array([3, 4, 5, -1, 16, 17, 18, P, 0, P - 1, -(1 << 40), 1 << 40]), np.arange(P), np.array([4, 17, 2, 9, 5])].astype(np.int64)
    start = np.array([0, 12, 12 + P, 12 + P + 5], dtype=np.int64)
    rank, S = _own(u, v, pos, start, few, skip, "skipped, out of range")
    assert rank[1] == -1 and rank[5] == -1 and rank[3] == -1 and rank[7] == -1 and rank[10] == -1 and rank[11] == -1
    assert (rank[[0, 2, 4, 6, 8, 9]] >= 0).all(), "neighbouring targets keep their ranks"
    assert (rank[[0, 2, 4, 6, 8, 9]] < P - 2).all() and len(set(rank[[0, 2, 4, 6, 8, 9]].tolist())) == 6, "among user 0's 38 elements"
    assert (rank[12:12 + P] == -1).all(), "a user whose every id is skipped"
    banned2 = np.isin(few, skip[2])
    assert ((rank[12 + P:] == -1) == banned2[pos[12 + P:]]).all()
    # pool ids outside [0, N): the Python entry refuses them, the C entry treats them as no element
    pool = few.copy()
    pool[5], pool[9] = N, -3
    with pytest.raises(ValueError, match="pool ids"):
        evaluate.dot_rank(_t(u), _t(v), _t(pos), start, pool=_t(pool))
    L = _lib.lib()
    U, V, PL, SK, TP, ST = _t(u), _t(v), _t(pool), _t(skip), _t(pos), _t(start)
    T = len(pos)
    need = int(L.digat_dot_rank_workspace_bytes(G, P, T))
    ws = _lib.workspace(need, _dev(), "dot_rank")
    out_r = torch.full((T,), 77, dtype=torch.int32, device=_dev())
    out_s = torch.full((T,), 123.0, dtype=torch.float32, device=_dev())
    _lib.check(L.digat_dot_rank(U.data_ptr(), V.data_ptr(), PL.data_ptr(), G, N, P, d, SK.data_ptr(), 64, TP.data_ptr(), ST.data_ptr(), T,
                                out_r.data_ptr(), out_s.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_dot_rank")
    S2 = evaluate.dot_scores(U, V, pool=_t(few)).cpu().numpy()      # the scores of positions 5 and 9 are never read
    want = evaluate.dot_rank_host(S2, pos, start, pool=pool, skip=skip, news_num=N)
    got = out_r.cpu().numpy()
    assert np.array_equal(got, want) and got[2] == -1 and got[12 + P + 3] == -1 and got[12 + P + 4] == -1
    assert (got[[0, 4, 6, 8, 9]] >= 0).sum() >= 3, "their neighbours keep a rank"
    assert np.array_equal(np.isnan(out_s.cpu().numpy()), want < 0)
    # an empty pool: nothing is an element
    none = evaluate.dot_rank(U, V, _t(pos), start, pool=_t(np.zeros(0, dtype=np.int64)))
    assert (none[0] == -1).all() and torch.isnan(none[1]).all()


def test_guards():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(13)
    G, N, P, d = 70, 600, 2300, 20
    u = rng.integers(-2, 3, size=(G, d)).astype(np.float32)
    v = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    pool = rng.integers(0, N, size=P).astype(np.int64)
    skip = rng.integers(0, N, size=(G, 64)).astype(np.int64)
    pos, start = R.make_targets(rng, G, P, PER_USER, evaluate.DOT_TOPK_CHUNK)
    T = len(pos)
    U, V, PL, SK, TP, ST = _t(u), _t(v), _t(pool), _t(skip), _t(pos), _t(start)
    first = evaluate.dot_rank(U, V, TP, start, pool=PL, skip=SK)
    want = evaluate.dot_rank_host(u @ v[pool].T, pos, start, pool=pool, skip=skip)
    assert np.array_equal(first[0].cpu().numpy(), want)

    def same(got, what):
        assert torch.equal(got[0], first[0]), what
        assert np.array_equal(_bits(got[1]), _bits(first[1])), what
    # calling again gives the same counts: the partial sums start from zero every time
    same(evaluate.dot_rank(U, V, TP, start, pool=PL, skip=SK), "second call")
    # a workspace full of 0xFF bytes changes nothing
    L = _lib.lib()
    need = int(L.digat_dot_rank_workspace_bytes(G, P, T))
    ws = _lib.workspace(need, _dev(), "dot_rank")
    ws.fill_(0xFF)
    same(evaluate.dot_rank(U, V, TP, start, pool=PL, skip=SK), "poisoned workspace")
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.dot_rank(U, V, TP, start, pool=PL, skip=SK)
    side.synchronize()
    same(on_side, "side stream")
    # nothing is written beyond [T], twice over the same buffers
    pad = 64
    out_r = torch.full((T + pad,), 77, dtype=torch.int32, device=_dev())
    out_s = torch.full((T + pad,), 123.0, dtype=torch.float32, device=_dev())
    for _ in range(2):
        _lib.check(L.digat_dot_rank(U.data_ptr(), V.data_ptr(), PL.data_ptr(), G, N, P, d, SK.data_ptr(), 64, TP.data_ptr(), ST.data_ptr(), T,
                                    out_r.data_ptr(), out_s.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_dot_rank")
        torch.cuda.synchronize()
        assert (out_r[T:] == 77).all() and (out_s[T:] == 123.0).all()
        same((out_r[:T], out_s[:T]), "raw call")
    # refusals of the Python entry
    with pytest.raises(ValueError, match="target_start"):
        evaluate.dot_rank(U, V, TP, start[:-1], pool=PL)
    with pytest.raises(ValueError, match="target_start"):
        evaluate.dot_rank(U, V, TP, np.r_[start[:-1], T + 1], pool=PL)
    with pytest.raises(ValueError, match="target_start"):
        evaluate.dot_rank(U, V, TP, np.r_[0, start[2], start[1], start[3:]], pool=PL)
    with pytest.raises(ValueError, match="target_pos"):
        evaluate.dot_rank(U, V, TP.float(), start, pool=PL)
    with pytest.raises(ValueError, match="share d"):
        evaluate.dot_rank(U, V[:, :5], TP, start)
    with pytest.raises(ValueError, match="skip must be"):
        evaluate.dot_rank(U, V, TP, start, pool=PL, skip=SK[:2])
    with pytest.raises(_lib.DigatHipError):
        evaluate.dot_rank(U.cpu(), V.cpu(), TP.cpu(), start)
    nobody = evaluate.dot_rank(U, V, TP[:0], np.zeros(G + 1, dtype=np.int64), pool=PL)
    assert nobody[0].shape == (0,) and nobody[1].shape == (0,)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_retrieval_metrics_on_the_device(pre):
    from digat_amd import evaluate, nrms
    ks = (1, 5, 10, 50)
    inp = D.inputs()
    hist, mask = inp["history_ids"], inp["history_mask"]
    m_cpu, dev_cpu = D.model(pre), R.dev_with_rows()                # every candidate clicked: 45 targets
    m, dev = D.model(pre, _dev()), R.dev_with_rows(_dev())
    got = nrms.retrieval_metrics(m, dev, ks=ks, batch_size=4)
    users = np.arange(D.USERS)
    tid, tst = got["target_ids"], got["target_start"]
    assert np.array_equal(tid, inp["candidate_ids"].reshape(-1))
    assert np.array_equal(tst, np.arange(D.USERS + 1) * R.CANDS) and got["rank"].dtype == np.int32
    # exactly the host contract on the device's own user vectors and augmented cache
    with torch.no_grad():
        _, aug = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 16)
    user = nrms.user_vectors(m, dev, users, batch_size=4)
    pool = np.arange(1, D.NEWS, dtype=np.int64)
    S_dev = evaluate.dot_scores(user, aug, pool=_t(pool)).cpu().numpy()
    skip = np.where(mask, hist, 0)
    own = evaluate.dot_rank_host(S_dev, tid - 1, tst, pool=pool, skip=skip)          # id 0 -> position -1: not in the pool
    assert np.array_equal(got["rank"], own)
    # precondition of the comparison with the CPU path, on the CPU path's own scores: every ranked target's gap to every other
    # element of its user exceeds the sum of the two forward tolerances (rtol 1e-5 / atol 2e-6)
    cpu = nrms.retrieval_metrics(m_cpu, dev_cpu, ks=ks)
    S = D.stock_scores(m_cpu, D.dev_set()).astype(np.float64)
    scale = float(np.abs(S).max())
    tol = lambda s: 2e-6 + 1e-5 * np.maximum(np.abs(s), 0.05 * scale)
    worst = np.inf
    for t in np.flatnonzero(cpu["rank"] >= 0):
        g = t // R.CANDS
        banned = D.banned_ids(hist[g], mask[g])
        others = np.array([c for c in range(1, D.NEWS) if c not in banned and c != tid[t]])
        gap = np.abs(S[g, others] - S[g, tid[t]])
        worst = min(worst, float((gap / (tol(S[g, others]) + tol(S[g, tid[t]]))).min()))
    print("smallest gap over the two tolerances:", worst)
    assert worst > 1.0
    assert np.array_equal(got["rank"], cpu["rank"])
    assert int((got["rank"] == -1).sum()) == sum(int(tid[t]) in D.banned_ids(hist[t // R.CANDS], mask[t // R.CANDS]) for t in range(len(tid)))
    assert (got["rank"] == -1).any(), "the fixture has targets without a rank"
    metrics = evaluate.rank_metrics(own, tst, ks)
    assert {k: v for k, v in got.items() if k not in ("rank", "target_start", "target_ids")} == metrics
    # the lists of recommend, scored by list_ranks, say the same about the first five
    ids, _, count = nrms.recommend(m, dev, users, k=5, batch_size=4)
    listed = evaluate.list_ranks(ids, count, _t(tid), tst).cpu().numpy()
    inside = (own >= 0) & (own < 5)
    assert np.array_equal(listed[inside], own[inside]) and (listed[~inside] == -1).all()
    assert evaluate.rank_metrics(listed, tst, (5,))["recall@5"] == metrics["recall@5"]
