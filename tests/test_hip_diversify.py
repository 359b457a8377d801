"""GPU suite: the greedy maximal-marginal-relevance kernel (``digat_mmr_select``) and ``recommend(diversity=)`` on it.  The
selection is held exactly — ids, score bits, counts, fills — to the host contract (``evaluate.mmr_select_host``) on the
similarities ``digat_dot_scores`` gives for the same rows, and on integer data to numpy integer arithmetic alone."""
import functools
import types

import numpy as np
import pytest
import torch

import diversify_common as V
import dot_topk_common as D

pytestmark = pytest.mark.gpu

GS, MS, DS, KS, LAMS, QS = (1, 3, 65), (1, 2, 15, 16, 17, 63, 64, 65, 127, 128), (1, 20, 100, 400), (1, 10, "M", 128), (0.0, 0.3, 0.5, 1.0), (0, 1, 2)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def device_gram(ids, vectors):
    """sim [G, M, M] on the device's own product: ``dot_scores(vectors[list_g], vectors, pool=list_g)`` per user (ids outside the
    table stand in as row 0: no elements, their similarities are never used)."""
    from digat_amd import evaluate
    N = int(vectors.shape[0])
    safe = torch.where((ids >= 0) & (ids < N), ids, torch.zeros_like(ids))
    return torch.stack([evaluate.dot_scores(vectors[safe[g]], vectors, pool=safe[g]) for g in range(ids.shape[0])]).cpu().numpy()


def float_case(seed, G, M, N, d):
    rng = np.random.default_rng(seed)
    vec = rng.standard_normal((N, d)).astype(np.float32)
    vec /= np.maximum(np.linalg.norm(vec, axis=1, keepdims=True), 1e-12).astype(np.float32)
    vec[N // 2] = 0.0
    vec[1:N:7] = vec[0:N - 1:7]                                       # near-duplicates are the point: exact copies among the rows
    ids, count = V.make_lists(rng, G, M, N)
    scores = rng.standard_normal((G, M)).astype(np.float32)
    scores[:, ::3] = np.round(scores[:, ::3] * 2) / 2                 # ties among the scores
    category = rng.integers(0, 50, size=N).astype(np.int32)        # a cap of 2 still lets a hundred picks through
    return vec, ids, count, scores, category


def grid_case(n, M):
    """The n-th list length of the grid with the other axes rotating over their values: ``(G, d, N, [(k, lam, q)])``."""
    G, d, N = (GS[n % 3] if M != 128 else 65), DS[(n + n // 4) % 4], (4096 if n % 2 else 300)
    steps = []
    for j, kk in enumerate(KS):
        k = M if kk == "M" else kk
        lam, q = LAMS[(j + n) % 4], QS[(j + n) % 3]
        if G == 65 and k == 128:
            lam, q = 0.3, 2                                           # the largest case meets the cap
        steps.append((k, lam, q))
    return G, d, N, steps


@pytest.mark.parametrize("n,M", list(enumerate(MS)))
def test_selection_is_exact_on_the_devices_own_similarities(n, M):
    from digat_amd import evaluate
    G, d, N, steps = grid_case(n, M)
    vec, ids, count, scores, category = float_case(n, G, M, N, d)
    VEC, IDS, CNT, SC, CAT = _t(vec), _t(ids), _t(count), _t(scores), _t(category)
    sim = device_gram(IDS, VEC)
    assert np.array_equal(sim, sim.transpose(0, 2, 1)), "the product is symmetric, bit for bit"
    for k, lam, q in steps:
        got = evaluate.mmr_select(IDS, SC, CNT, VEC, k, lam, category=CAT if q else None, max_per_category=q)
        want = evaluate.mmr_select_host(ids, scores, count, sim, k, lam, category=category if q else None, max_per_category=q, news_num=N)
        V.same(got, want, (G, M, d, k, lam, q))
    # count=None is M
    got = evaluate.mmr_select(IDS, SC, None, VEC, min(M, 10), 0.3)
    V.same(got, evaluate.mmr_select_host(ids, scores, None, sim, min(M, 10), 0.3, news_num=N), "count None")


def test_every_axis_value_of_the_grid_is_met():
    cases = [grid_case(n, M) for n, M in enumerate(MS)]
    assert {c[0] for c in cases} == set(GS) and {c[1] for c in cases} == set(DS)
    steps = [s for c in cases for s in c[3]]
    assert {s[1] for s in steps} == set(LAMS) and {s[2] for s in steps} == set(QS)
    assert {s[0] for s in steps} >= {1, 10, 128} | set(MS)


@pytest.mark.parametrize("q", [0, 2])
def test_selection_is_exact_against_numpy_on_integer_data(q):
    """Integers in [-2, 2], d = 20, integer scores, lam = 0.5: every similarity, product and difference is exact, hundreds of ties
    per list — no device Gram on the expected side."""
    from digat_amd import evaluate
    rng = np.random.default_rng(7 + q)
    G, M, N, d, k = 5, 128, 700, 20, 100
    vec = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    ids, count = V.make_lists(rng, G, M, N)
    scores = rng.integers(-3, 4, size=(G, M)).astype(np.float32) * 2
    scores[3, ::5] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=np.float32)[rng.integers(0, 5, size=len(scores[3, ::5]))]
    safe = np.where((ids >= 0) & (ids < N), ids, 0)
    rows = vec[safe].astype(np.int64)
    sim = np.einsum("gid,gjd->gij", rows, rows).astype(np.float32)
    assert len(np.unique(scores[0])) <= 7 and len(np.unique(sim[0])) < 200
    category = rng.integers(0, 60, size=N).astype(np.int32)
    got = evaluate.mmr_select(_t(ids), _t(scores), _t(count), _t(vec), k, 0.5, category=_t(category) if q else None, max_per_category=q)
    want = evaluate.mmr_select_host(ids, scores, count, sim, k, 0.5, category=category if q else None, max_per_category=q, news_num=N)
    V.same(got, want, "integers")
    g = 0
    mine = V.brute_force(ids[g], scores[g], count[g], sim[g], k, 0.5, N, category, q)
    assert got[1][g, :len(mine)].tolist() == [e[1] for e in mine] and int(got[2][g]) == len(mine)


def test_a_users_row_does_not_depend_on_the_batch():
    from digat_amd import evaluate
    G, M, N, d, k = 65, 128, 2000, 100, 32
    vec, ids, count, scores, category = float_case(21, G, M, N, d)
    VEC, CAT = _t(vec), _t(category)
    whole = evaluate.mmr_select(_t(ids), _t(scores), _t(count), VEC, k, 0.3, category=CAT, max_per_category=2)
    for g in (0, 1, 2, 31, 64):
        one = evaluate.mmr_select(_t(ids[g:g + 1]), _t(scores[g:g + 1]), _t(count[g:g + 1]), VEC, k, 0.3, category=CAT, max_per_category=2)
        V.same(one, tuple(t[g:g + 1] for t in whole), g)


def test_guards():
    from digat_amd import _lib, evaluate
    G, M, N, d, k, q = 3, 65, 500, 20, 70, 2
    vec, ids, count, scores, category = float_case(9, G, M, N, d)
    VEC, IDS, CNT, SC, CAT = _t(vec), _t(ids), _t(count), _t(scores), _t(category)
    first = evaluate.mmr_select(IDS, SC, CNT, VEC, k, 0.3, category=CAT, max_per_category=q)
    want = tuple(t.cpu().numpy() for t in first)
    assert int(first[2][1]) == 0 and (first[1][1] == -1).all() and torch.isneginf(first[0][1]).all(), "an empty list"
    assert (want[2] < k).all(), "M < k: every row has a fill"
    # a workspace full of NaN bytes changes nothing
    ws = _lib.workspace(0, _dev(), "mmr")
    ws.fill_(0xFF)
    V.same(evaluate.mmr_select(IDS, SC, CNT, VEC, k, 0.3, category=CAT, max_per_category=q), want, "poisoned workspace")
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.mmr_select(IDS, SC, CNT, VEC, k, 0.3, category=CAT, max_per_category=q)
    side.synchronize()
    V.same(on_side, want, "side stream")
    # outputs full of garbage, guard regions on both sides of each: every output byte is written, nothing else is
    L = _lib.lib()
    pad = 64
    out_s = torch.full((pad + G * k + pad,), 123.0, dtype=torch.float32, device=_dev())
    out_i = torch.full((pad + G * k + pad,), 77, dtype=torch.int64, device=_dev())
    out_c = torch.full((pad + G + pad,), 55, dtype=torch.int32, device=_dev())
    inputs = [t.clone() for t in (IDS, SC, CNT, VEC, CAT)]
    lam, mu = evaluate.mmr_weights(0.3)
    _lib.check(L.digat_mmr_select(IDS.data_ptr(), SC.data_ptr(), CNT.data_ptr(), G, M, VEC.data_ptr(), N, d, CAT.data_ptr(), q, float(lam),
                                  float(mu), k, out_i[pad:].data_ptr(), out_s[pad:].data_ptr(), out_c[pad:].data_ptr(), None, 0,
                                  _lib.stream_ptr()), "digat_mmr_select")
    torch.cuda.synchronize()
    assert (out_s[:pad] == 123.0).all() and (out_s[pad + G * k:] == 123.0).all()
    assert (out_i[:pad] == 77).all() and (out_i[pad + G * k:] == 77).all()
    assert (out_c[:pad] == 55).all() and (out_c[pad + G:] == 55).all()
    V.same((out_s[pad:pad + G * k].view(G, k), out_i[pad:pad + G * k].view(G, k), out_c[pad:pad + G]), want, "raw call")
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (IDS, SC, CNT, VEC, CAT))), "inputs are read only"
    # refusals of the Python entry
    with pytest.raises(ValueError, match="k must be"):
        evaluate.mmr_select(IDS, SC, CNT, VEC, 129, 0.3)
    with pytest.raises(ValueError, match="lam must"):
        evaluate.mmr_select(IDS, SC, CNT, VEC, k, 1.2)
    with pytest.raises(ValueError, match="needs category"):
        evaluate.mmr_select(IDS, SC, CNT, VEC, k, 0.3, max_per_category=1)
    with pytest.raises(ValueError, match="one entry per row"):
        evaluate.mmr_select(IDS, SC, CNT, VEC, k, 0.3, category=CAT[:5], max_per_category=1)
    with pytest.raises(ValueError, match=r"\[G, M\]"):
        evaluate.mmr_select(IDS, SC[:, :5], CNT, VEC, k, 0.3)
    nobody = evaluate.mmr_select(IDS[:0], SC[:0], CNT[:0], VEC, k, 0.3)
    assert tuple(nobody[0].shape) == (0, k) and tuple(nobody[2].shape) == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# recommend(diversity=) end to end
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    from digat_amd import synthetic
    kw, depth = synthetic.DEVSET_FIXTURES["devset_tiny"]
    spec = synthetic.SynthSpec(**kw)
    return spec, synthetic.make_corpus(spec), depth


def _model():
    from digat_amd import synthetic
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec, corpus, depth = _corpus()
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return model.to(_dev()).eval()


def test_digat_recommend_with_diversity_end_to_end():
    from digat_amd import evaluate, util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    assert dc.news_category is not None and dc.news_category.dtype == torch.int32
    users, pool, k = np.arange(6), np.arange(1, spec.news_num, dtype=np.int64), 10
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    again = util.recommend(model, dc, users, pool, k, batch_size=256, diversity=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    wide = util.recommend(model, dc, users, pool, 40, batch_size=256)
    # lam = 1: the first k of the un-diversified result, bit for bit
    same = util.recommend(model, dc, users, pool, k, batch_size=256, diversity=0.0)
    V.same((same[1], same[0], same[2]), (wide[1][:, :k], wide[0][:, :k], torch.clamp(wide[2], max=k)), "lam = 1")
    # the plain call at k', then the host restatement on a device Gram
    unit = util.unit_rows(dc.news_embedding)
    got = util.recommend(model, dc, users, pool, k, batch_size=256, diversity=0.3, max_per_category=2)
    assert got[0].is_cuda and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    want = evaluate.mmr_select_host(wide[0].cpu().numpy(), wide[1].cpu().numpy(), wide[2].cpu().numpy(), device_gram(wide[0], unit), k, 0.7,
                                    category=corpus.news_category, max_per_category=2, news_num=spec.news_num)
    V.same((got[1], got[0], got[2]), want, "DIGAT, diversity 0.3, two per category")
    ids = got[0].cpu().numpy()
    assert all(np.bincount(corpus.news_category[ids[g, :int(got[2][g])]]).max() <= 2 for g in range(len(users)))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_diversity_end_to_end(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users, k = np.arange(D.USERS), 5
    wide = nrms.recommend(m, dev, users, k=20, batch_size=4)
    with torch.no_grad():
        cache, _ = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask)
    got = nrms.recommend(m, dev, users, k=k, batch_size=4, diversity=0.3)
    want = evaluate.mmr_select_host(wide[0].cpu().numpy(), wide[1].cpu().numpy(), wide[2].cpu().numpy(), device_gram(wide[0], cache), k, 0.7,
                                    news_num=D.NEWS)
    V.same((got[1], got[0], got[2]), want, (pre, "diversity 0.3"))
    same = nrms.recommend(m, dev, users, k=k, batch_size=4, diversity=0.0)
    V.same((same[1], same[0], same[2]), (wide[1][:, :k], wide[0][:, :k], torch.clamp(wide[2], max=k)), "lam = 1")
