"""GPU suite: the fused inner-product + top-k kernel (``digat_dot_topk``) and ``nrms.recommend`` on it.  The selection is held exactly
— ids, score bits, counts — to the host contract (``evaluate.dot_topk_host``) on the kernel's own scores (``digat_dot_scores``, the
same device code with a store epilogue) and on exactly representable products; the values to the classical bound of an fp32 chain of
d terms, ``d 2^-24 sum_c |u_c v_c|``, against an fp64 product."""
import ctypes as C

import numpy as np
import pytest
import torch

import dot_topk_common as D

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
    assert np.array_equal(c, want[2]), (what, "count", c.tolist(), want[2].tolist())
    assert np.array_equal(i, want[1]), (what, "ids", np.argwhere(i != want[1])[:5].tolist())
    assert np.array_equal(_bits(s), _bits(want[0])), (what, "score bits")


def _own(users, news, k, pool, skip, what):
    """dot_topk against the host contract on dot_scores of the same arguments."""
    from digat_amd import evaluate
    got = evaluate.dot_topk(_t(users), _t(news), k, pool=_t(pool), skip=_t(skip))
    S = evaluate.dot_scores(_t(users), _t(news), pool=_t(pool)).cpu().numpy()
    assert S.shape == (users.shape[0], news.shape[0] if pool is None else len(pool))
    _same(got, evaluate.dot_topk_host(S, k, pool=pool, skip=skip), what)
    return got, S


def _case(rng, G, P, d, pool, skip, integers):
    N = P + 37 if pool else P
    draw = (lambda shape: rng.integers(-2, 3, size=shape).astype(np.float32)) if integers else \
        (lambda shape: rng.standard_normal(shape).astype(np.float32))
    users, news = draw((G, d)), draw((max(N, 1), d))
    if not pool:
        news = news[:N]
    pl = rng.integers(0, N, size=P).astype(np.int64) if pool else None                   # unsorted, with repeats
    sk = None
    if skip:
        src = pl if pool else np.arange(P, dtype=np.int64)
        sk = np.stack([src[rng.integers(0, P, size=50)] if P else np.full(50, 5, dtype=np.int64) for _ in range(G)])
    return users, news, pl, sk


def test_selection_is_exact_on_the_kernels_own_scores():
    from digat_amd import evaluate
    ch, sub, tile = evaluate.DOT_TOPK_CHUNK, evaluate.DOT_TOPK_SUB, evaluate.DOT_TOPK_USERS
    rng = np.random.default_rng(1)
    Gs, ds, ks = (1, 3, tile + 1), (1, 20, 100, 400), (1, 10, 128)
    seen, n = set(), 0
    for k in ks:
        for P in (1, k - 1, 255, 257, sub - 1, sub, sub + 1, ch - 1, ch, ch + 1, 2 * ch + 1):
            G, d = Gs[n % 3], ds[(n // 3 + n) % 4]
            if P == 2 * ch + 1:                       # the largest case: more than one user tile by three chunks, once per k
                G, d = tile + 1, (400, 100, 20)[ks.index(k)]
            for pool in (False, True):
                for skip in (False, True):
                    users, news, pl, sk = _case(rng, G, P, d, pool, skip, integers=(n % 2 == 0))
                    (s, i, c), S = _own(users, news, k, pl, sk, (G, P, d, k, pool, skip))
                    if not skip:
                        assert (c.cpu().numpy() == min(k, P)).all()
            seen.add((G, d))
            n += 1
    assert {g for g, _ in seen} == set(Gs) and {d for _, d in seen} == set(ds)


def test_selection_is_exact_against_numpy_on_integer_vectors():
    """Integers in [-3, 3], d = 100: every partial sum is an integer below 2^24, exact in fp32 in any order — thousands of ties."""
    from digat_amd import evaluate
    rng = np.random.default_rng(7)
    G, N, P, d, k = 5, 3000, 5000, 100, 16
    u = rng.integers(-3, 4, size=(G, d)).astype(np.float32)
    v = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    pool = rng.integers(0, N, size=P).astype(np.int64)
    assert len(np.unique(pool)) < P and (np.diff(pool) < 0).any()                         # repeated ids, not sorted
    S = u @ v[pool].T
    assert np.array_equal(S.astype(np.float64), u.astype(np.float64) @ v[pool].astype(np.float64).T)
    assert len(np.unique(S)) < 400
    skip = np.stack([pool[rng.integers(0, P, size=50)] for _ in range(G)])
    for sk in (None, skip):
        got = evaluate.dot_topk(_t(u), _t(v), k, pool=_t(pool), skip=_t(sk))
        _same(got, evaluate.dot_topk_host(S, k, pool=pool, skip=sk), "integers")
    assert np.array_equal(_bits(evaluate.dot_scores(_t(u), _t(v), pool=_t(pool))), _bits(S))


def test_values_are_within_the_fp32_chain_bound_of_an_fp64_product():
    from digat_amd import evaluate
    rng = np.random.default_rng(0)
    G, P, d, k = 24, 3000, 100, 16
    u = rng.standard_normal((G, d)).astype(np.float32)
    v = rng.standard_normal((P, d)).astype(np.float32)
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    S = u64 @ v64.T
    B = d * 2.0 ** -24 * (np.abs(u64) @ np.abs(v64).T)
    order = np.argsort(-S, axis=1, kind="stable")[:, :k + 1]
    top, tb = np.take_along_axis(S, order, 1), np.take_along_axis(B, order, 1)
    assert (top[:, :-1] - top[:, 1:] > tb[:, :-1] + tb[:, 1:]).all(), "every slot's fp64 gap to both neighbours exceeds the two bounds"
    s, i, c = (t.cpu().numpy() for t in evaluate.dot_topk(_t(u), _t(v), k))
    assert (c == k).all()
    assert np.array_equal(i, order[:, :k])
    err = np.abs(s.astype(np.float64) - top[:, :k])
    print("max err / bound", float((err / tb[:, :k]).max()))
    assert (err <= tb[:, :k]).all()
    full = evaluate.dot_scores(_t(u), _t(v)).cpu().numpy().astype(np.float64)
    assert (np.abs(full - S) <= B).all()


@pytest.mark.parametrize("d", [37, 400])
def test_score_bits_do_not_depend_on_the_call(d):
    from digat_amd import evaluate
    rng = np.random.default_rng(3)
    G, N, k = 5, evaluate.DOT_TOPK_CHUNK + 300, 128
    u = rng.standard_normal((G, d)).astype(np.float32)
    v = rng.standard_normal((N, d)).astype(np.float32)
    U, V = _t(u), _t(v)
    full = _bits(evaluate.dot_scores(U, V))
    s, i, c = (t.cpu().numpy() for t in evaluate.dot_topk(U, V, k))
    assert np.array_equal(_bits(s), np.take_along_axis(full, i, 1)), "the fused entry returns dot_scores' bits"
    perm = rng.permutation(N).astype(np.int64)
    assert np.array_equal(_bits(evaluate.dot_scores(U, V, pool=_t(perm))), full[:, perm]), "a permuted pool moves no bit"
    sp, ip, cp = (t.cpu().numpy() for t in evaluate.dot_topk(U, V, k, pool=_t(perm)))
    assert np.array_equal(_bits(sp), np.take_along_axis(full, ip, 1))
    assert np.array_equal(np.sort(ip, axis=1), np.sort(i, axis=1)), "no ties here: the same news in any pool order"
    for g, n in ((0, int(i[0, 0])), (G - 1, int(i[G - 1, k - 1])), (2, N - 1), (3, 0)):
        one = evaluate.dot_scores(U[g:g + 1], V[n:n + 1])
        assert _bits(one)[0, 0] == full[g, n], (g, n)
        s1, i1, c1 = evaluate.dot_topk(U[g:g + 1].clone(), V[n:n + 1].clone(), 1)
        assert _bits(s1)[0, 0] == full[g, n] and int(i1[0, 0]) == 0 and int(c1[0]) == 1


def test_specials_follow_the_host_contract():
    from digat_amd import evaluate
    rng = np.random.default_rng(4)
    d, N = 20, 300
    v = rng.standard_normal((N, d)).astype(np.float32)
    v[10], v[20], v[30], v[40] = np.nan, np.inf, -np.inf, 0.0
    v[50, 3] = np.nan
    u = rng.standard_normal((6, d)).astype(np.float32)
    u[0] = -0.0
    u[1] = np.abs(u[1])                                   # +inf and -inf scores; mixed signs give inf - inf = NaN
    u[2] = 0.0
    for k in (10, 128):
        got, S = _own(u, v, k, None, None, ("specials", k))
        assert np.isnan(S[:, 10]).all() and np.isposinf(S[1, 20]) and np.isneginf(S[1, 30]) and np.isnan(S[0, 20])
    ids = got[1].cpu().numpy()
    assert ids[1, 0] == 20 and 30 not in ids[1].tolist()
    # fewer numbers than k: the NaNs are returned, behind every number (-inf included), in position order
    pool = np.array([10, 7, 30, 50, 20, 3], dtype=np.int64)
    (s, i, c), S = _own(u[1:2], v, 10, pool, None, "nan last")
    assert c.tolist() == [6] and i[0, :6].tolist() == [20] + sorted((7, 3), key=lambda n: -S[0, list(pool).index(n)]) + [30, 10, 50]
    assert torch.isnan(s[0, 4:6]).all() and (i[0, 6:] == -1).all() and torch.isneginf(s[0, 6:]).all()


def test_guards():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(9)
    G, N, P, d, k = 3, 500, 400, 20, 10
    u = rng.integers(-2, 3, size=(G, d)).astype(np.float32)
    v = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    few = rng.permutation(N)[:40].astype(np.int64)
    skip = rng.integers(0, N, size=(G, 64)).astype(np.int64)
    skip[1, :40], skip[1, 40:] = few, few[0]
    (s, i, c), _ = _own(u, v, k, few, skip, "every id of user 1 skipped")
    assert int(c[1]) == 0 and (i[1] == -1).all() and torch.isneginf(s[1]).all() and int(c[0]) == k
    # a workspace full of NaN bytes changes nothing
    pool = rng.integers(0, N, size=P).astype(np.int64)
    U, V, PL, SK = _t(u), _t(v), _t(pool), _t(skip)
    first = evaluate.dot_topk(U, V, k, pool=PL, skip=SK)
    need = int(_lib.lib().digat_dot_topk_workspace_bytes(G, P, k))
    ws = _lib.workspace(need, _dev(), "dot_topk")
    ws.fill_(0xFF)
    again = evaluate.dot_topk(U, V, k, pool=PL, skip=SK)
    _same(again, tuple(t.cpu().numpy() for t in first), "poisoned workspace")
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.dot_topk(U, V, k, pool=PL, skip=SK)
        scores_side = evaluate.dot_scores(U, V, pool=PL)
    side.synchronize()
    _same(on_side, tuple(t.cpu().numpy() for t in first), "side stream")
    assert torch.equal(scores_side, evaluate.dot_scores(U, V, pool=PL))
    # nothing is written beyond [G, k]
    L = _lib.lib()
    pad = 64
    out_s = torch.full((G * k + pad,), 123.0, dtype=torch.float32, device=_dev())
    out_i = torch.full((G * k + pad,), 77, dtype=torch.int64, device=_dev())
    out_c = torch.full((G + pad,), 55, dtype=torch.int32, device=_dev())
    _lib.check(L.digat_dot_topk(U.data_ptr(), V.data_ptr(), PL.data_ptr(), G, N, P, d, SK.data_ptr(), 64, k, out_s.data_ptr(),
                                out_i.data_ptr(), out_c.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_dot_topk")
    torch.cuda.synchronize()
    assert (out_s[G * k:] == 123.0).all() and (out_i[G * k:] == 77).all() and (out_c[G:] == 55).all()
    _same((out_s[:G * k].view(G, k), out_i[:G * k].view(G, k), out_c[:G]), tuple(t.cpu().numpy() for t in first), "raw call")
    out_m = torch.full((G * P + pad,), 123.0, dtype=torch.float32, device=_dev())
    _lib.check(L.digat_dot_scores(U.data_ptr(), V.data_ptr(), PL.data_ptr(), G, N, P, d, out_m.data_ptr(), _lib.stream_ptr()),
               "digat_dot_scores")
    assert (out_m[G * P:] == 123.0).all() and np.array_equal(_bits(out_m[:G * P]), _bits((u @ v[pool].T).ravel()))
    # refusals of the Python entry
    with pytest.raises(ValueError, match="pool ids"):
        evaluate.dot_topk(U, V, k, pool=_t(np.array([0, N], dtype=np.int64)))
    with pytest.raises(ValueError, match="k must be"):
        evaluate.dot_topk(U, V, 129)
    with pytest.raises(ValueError, match="share d"):
        evaluate.dot_scores(U, V[:, :5])
    with pytest.raises(ValueError, match="skip must be"):
        evaluate.dot_topk(U, V, k, skip=SK[:2])
    empty = evaluate.dot_topk(U, V, k, pool=_t(np.zeros(0, dtype=np.int64)))
    assert empty[2].tolist() == [0] * G and (empty[1] == -1).all()


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_on_the_device(pre):
    from digat_amd import nrms, util
    k = 5
    m_cpu, dev_cpu, inp = D.model(pre), D.dev_set(), D.inputs()
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users = np.arange(D.USERS)
    hist, mask = inp["history_ids"], inp["history_mask"]
    # precondition, on the CPU path's own scores: the top-(k + 1) gaps exceed twice the forward tolerance (rtol 1e-5 / atol 2e-6)
    S = D.stock_scores(m_cpu, dev_cpu).astype(np.float64)
    scale = float(np.abs(S).max())
    for g in users:
        banned = D.banned_ids(hist[g], mask[g])
        top = np.sort(S[g, [c for c in range(1, D.NEWS) if c not in banned]])[::-1][:k + 1]
        tol = 2e-6 + 1e-5 * np.maximum(np.abs(top), 0.05 * scale)
        assert (top[:-1] - top[1:] > tol[:-1] + tol[1:]).all(), g
    want = nrms.recommend(m_cpu, dev_cpu, users, k=k)
    ids, scores, count = nrms.recommend(m, dev, users, k=k, batch_size=4)
    assert ids.is_cuda and ids.dtype == torch.int64 and scores.dtype == torch.float32 and count.dtype == torch.int32
    assert torch.equal(ids.cpu(), want[0]) and torch.equal(count.cpu(), want[2])
    # the scores against row_logits on the same caches and user vectors, within d 2^-24 sum |u v|
    with torch.no_grad():
        _, aug = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask)
    user = nrms.user_vectors(m, dev, users, batch_size=4)
    rows_n, rows_u = aug[ids.reshape(-1)], user.repeat_interleave(k, dim=0)
    ref = nrms.row_logits(rows_n, rows_u).view(D.USERS, k)
    hd = int(user.shape[1])
    bound = hd * 2.0 ** -24 * (rows_n.double().abs() * rows_u.double().abs()).sum(dim=1).view(D.USERS, k)
    assert ((scores.double() - ref.double()).abs() <= bound).all()
    assert ((scores.double() - (rows_n.double() * rows_u.double()).sum(dim=1).view(D.USERS, k)).abs() <= bound).all()
    # the shared pool and the same pool as per-user lists
    pool = np.arange(1, D.NEWS, dtype=np.int64)
    csr = (np.tile(pool, D.USERS), np.arange(D.USERS + 1, dtype=np.int64) * len(pool))
    by_list = nrms.recommend(m, dev, users, candidates=csr, k=k)
    assert torch.equal(by_list[0], ids) and torch.equal(by_list[2], count)
    flat, start = nrms.candidates_csr(ids, count)
    got_ids, got_start = util.recommend_candidates((flat, start), users=D.USERS, news_num=D.NEWS)
    assert got_ids.tolist() == ids.reshape(-1).tolist() and got_start.tolist() == (np.arange(D.USERS + 1) * k).tolist()
    # people who are no rows of the corpus, candidates at their word
    other = nrms.recommend(m, dev, (hist[:3], mask[:3]), candidates=np.array([0, 4, 9]), k=3, exclude_history=False)
    assert sorted(other[0][1].tolist()) == [0, 4, 9]
