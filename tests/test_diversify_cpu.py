"""CPU suite: diversified top-k without a GPU — ``evaluate.mmr_select_host`` (the yardstick the GPU suite holds the kernel to
exactly) against a brute-force selection in plain Python; its two corollaries (``lam = 1`` is the stable sort by score, a cap
fills ``min(k, sum_c min(q, n_c))`` slots); the library's entry declared, exported and refusing bad arguments before any launch;
``util.recommend`` / ``nrms.recommend`` with ``diversity=`` on CPU tensors; the CLI flags."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import diversify_common as V
import dot_topk_common as D
from conftest import REPO

OK, ARG, SHAPE = 0, 1, 2
NEW = ("digat_mmr_select_workspace_bytes", "digat_mmr_select")


# ---------------------------------------------------------------------------------------------------------------------
# mmr_select_host against plain Python
# ---------------------------------------------------------------------------------------------------------------------
def integer_case(rng, G, M, N, d, specials=False):
    """Integer-valued vectors and scores: with lam = 0.5 every product and difference is exact, and ties are plentiful."""
    vec = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    ids, count = V.make_lists(rng, G, M, N)
    scores = rng.integers(-3, 4, size=(G, M)).astype(np.float32) * 2
    if specials:
        vals = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=np.float32)
        hole = rng.random((G, M)) < 0.25
        scores[hole] = vals[rng.integers(0, len(vals), size=int(hole.sum()))]
    safe = np.where((ids >= 0) & (ids < N), ids, 0)
    rows = vec[safe].astype(np.int64)
    sim = np.einsum("gid,gjd->gij", rows, rows).astype(np.float32)
    category = rng.integers(0, 4, size=N).astype(np.int64)
    return vec, ids, count, scores, sim, category


def check_host_against_brute_force(case, k, q, N):
    from digat_amd import evaluate
    vec, ids, count, scores, sim, category = case
    got = evaluate.mmr_select_host(ids, scores, count, sim, k, 0.5, category=category if q else None, max_per_category=q, news_num=N)
    assert got[0].shape == got[1].shape == (len(ids), k) and got[0].dtype == np.float32 and got[1].dtype == np.int64
    assert got[2].dtype == np.int32
    for g in range(len(ids)):
        want = V.brute_force(ids[g], scores[g], count[g], sim[g], k, 0.5, N, category, q)
        m = len(want)
        assert got[2][g] == m, g
        assert got[1][g, :m].tolist() == [e[1] for e in want], g
        assert V.bits(got[0][g, :m]).tolist() == V.bits(scores[g][[e[0] for e in want]]).tolist(), g       # the input score bits
        assert np.all(got[1][g, m:] == -1) and np.all(np.isneginf(got[0][g, m:])), g


@pytest.mark.parametrize("specials", [False, True])
@pytest.mark.parametrize("k,q", [(1, 0), (5, 0), (5, 1), (12, 2), (40, 0)])
def test_host_selection_matches_plain_python(k, q, specials):
    rng = np.random.default_rng(10 * k + q + 100 * specials)
    G, M, N, d = 9, 23, 60, 6
    case = integer_case(rng, G, M, N, d, specials)
    ids, count, scores = case[1], case[2], case[3]
    assert count[1] == 0 and count[0] == M and ((ids < 0) | (ids >= N)).any()
    assert any(len(set(r.tolist())) < M for r in ids), "a repeated id"
    if specials:
        assert np.isnan(scores).any() and np.isinf(scores).any() and (V.bits(scores) == 0x80000000).any()
    check_host_against_brute_force(case, k, q, N)


def test_lam_one_without_a_cap_is_the_stable_sort_by_score():
    from digat_amd import evaluate
    rng = np.random.default_rng(3)
    G, M, N, d = 6, 31, 50, 5
    vec, ids, count, scores, sim, category = integer_case(rng, G, M, N, d, specials=True)
    ids = np.where((ids >= 0) & (ids < N), ids, 0)                       # every entry inside count an element
    for k in (1, 7, 31, 64):
        got = evaluate.mmr_select_host(ids, scores, count, sim, k, 1.0)
        for g in range(G):
            n = int(count[g])
            ws, wi, wc = evaluate.topk_segments_host(scores[g, :n], np.array([0, n]), k, ids=ids[g, :n])
            assert got[2][g] == wc[0] and got[1][g].tolist() == wi[0].tolist() and V.bits(got[0][g]).tolist() == V.bits(ws[0]).tolist()


@pytest.mark.parametrize("q", [1, 2, 5])
def test_cap_bounds_every_category_and_fills_what_it_can(q):
    from digat_amd import evaluate
    rng = np.random.default_rng(q)
    G, M, N, d, k = 8, 40, 200, 4, 12
    vec, ids, count, scores, sim, category = integer_case(rng, G, M, N, d)
    s, i, c = evaluate.mmr_select_host(ids, scores, count, sim, k, 0.5, category=category, max_per_category=q)
    for g in range(G):
        elem = (np.arange(M) < count[g]) & (ids[g] >= 0) & (ids[g] < N)
        per_cat = np.bincount(category[ids[g][elem]], minlength=4)
        assert c[g] == min(k, int(np.minimum(per_cat, q).sum())), g
        assert np.bincount(category[i[g, :c[g]]], minlength=4).max(initial=0) <= q


def test_host_refuses_bad_arguments():
    from digat_amd import evaluate
    ids = np.zeros((2, 4), dtype=np.int64)
    sc = np.zeros((2, 4), dtype=np.float32)
    sim = np.zeros((2, 4, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="k must be"):
        evaluate.mmr_select_host(ids, sc, None, sim, 0, 0.5)
    with pytest.raises(ValueError, match="k must be"):
        evaluate.mmr_select_host(ids, sc, None, sim, 129, 0.5)
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam must"):
            evaluate.mmr_select_host(ids, sc, None, sim, 2, lam)
    with pytest.raises(ValueError, match="sim must be"):
        evaluate.mmr_select_host(ids, sc, None, sim[:, :3], 2, 0.5)
    with pytest.raises(ValueError, match="needs category"):
        evaluate.mmr_select_host(ids, sc, None, sim, 2, 0.5, max_per_category=1)
    with pytest.raises(ValueError, match="max_per_category"):
        evaluate.mmr_select_host(ids, sc, None, sim, 2, 0.5, category=np.zeros(3), max_per_category=-1)
    with pytest.raises(ValueError, match="count must"):
        evaluate.mmr_select_host(ids, sc, np.zeros(3), sim, 2, 0.5)
    with pytest.raises(ValueError, match=r"\[G, M\]"):
        evaluate.mmr_select_host(np.zeros((2, 129), dtype=np.int64), np.zeros((2, 129)), None, np.zeros((2, 129, 129)), 2, 0.5)
    assert evaluate.mmr_weights(0.3) == (np.float32(0.3), np.float32(1) - np.float32(0.3))


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+DIGAT_ABI_VERSION\s+(\d+)", header).group(1)) == 4
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_dot_topk.inc"') < hip.index('#include "digat_mmr.inc"')          # it uses dot_load4 and topk_key
    assert evaluate.MMR_MAX_LIST == evaluate.TOPK_MAX_K == 128
    assert L.digat_mmr_select_workspace_bytes(4096, 128, 128) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)

    def call(ids=p, scores=p, count=p, G=3, M=16, vectors=p, N=100, d=20, category=p, q=2, lam=0.5, mu=0.5, k=10, out_i=p, out_s=p,
             out_c=p, ws=None, ws_bytes=0):
        return L.digat_mmr_select(ids, scores, count, G, M, vectors, N, d, category, q, lam, mu, k, out_i, out_s, out_c, ws, ws_bytes, None)
    for name in ("ids", "scores", "vectors", "out_i", "out_s", "out_c"):
        assert call(**{name: None}) == ARG, name
    assert call(category=None) == ARG                              # a cap without categories
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(lam=lam) == ARG, lam
    assert call(G=-1) == ARG and call(N=-1) == ARG and call(q=-1) == ARG
    for k in (0, -1, 129):
        assert call(k=k) == SHAPE, k
    for M in (0, -1, 129):
        assert call(M=M) == SHAPE, M
    assert call(d=0) == SHAPE and call(d=-4) == SHAPE
    assert call(G=0) == OK
    assert call(G=0, count=None, category=None, q=0, lam=0.0, mu=1.0, k=128, M=128) == OK
    assert call(G=0, lam=1.0, mu=0.0) == OK


# ---------------------------------------------------------------------------------------------------------------------
# recommend(diversity=) on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def host_corpus(news_num=60, I=5, H=4, C=3, d=8, seed=0):
    from digat_amd import util
    rng = np.random.default_rng(seed)
    emb = torch.from_numpy(rng.integers(-2, 3, size=(news_num, d)).astype(np.float32))
    emb[7] = 0.0                                                    # a zero row stays zero under unit_rows
    return util.DeviceCorpus(
        news_embedding=emb, news_node_ID=torch.zeros(news_num, 2, dtype=torch.int64),
        news_graph=torch.zeros(news_num, 2, 2, dtype=torch.bool), news_graph_mask=torch.zeros(news_num, 2, dtype=torch.bool),
        history=torch.from_numpy(rng.integers(0, news_num, size=(I, H))), user_graph=torch.zeros(I, H + C, H + C, dtype=torch.bool),
        user_category_mask=torch.zeros(I, C + 1, dtype=torch.bool),
        user_category_indices=torch.from_numpy(rng.integers(0, C + 1, size=(I, H))), row_impression=torch.zeros(0, dtype=torch.int64),
        row_candidate=torch.zeros(0, dtype=torch.int64), category_num=C,
        news_category=torch.from_numpy(rng.integers(0, C, size=news_num).astype(np.int32)))


def fake_scoring(monkeypatch):
    """``util.score_rows`` replaced by a fixed function of (user, candidate) with few values, the news-side refresh by nothing: the
    selection stages of ``util.recommend`` run on CPU tensors."""
    from digat_amd import util

    def score_rows(model, view, start, end, batch_size, *a, **kw):
        return ((view.row_impression * 5 + view.row_candidate * 3) % 7).to(torch.float32) * 0.25 - 0.5
    monkeypatch.setattr(util, "score_rows", score_rows)
    monkeypatch.setattr(util, "refresh_news_side", lambda model, dc, batch_size: None)


def test_unit_rows():
    from digat_amd import util
    t = torch.tensor([[3.0, 4.0], [0.0, 0.0], [-2.0, 0.0]])
    u = util.unit_rows(t)
    assert torch.allclose(u, torch.tensor([[0.6, 0.8], [0.0, 0.0], [-1.0, 0.0]])) and u.is_contiguous() and u.dtype == torch.float32
    assert not torch.isnan(u).any()


def test_util_recommend_with_diversity_is_the_plain_call_then_the_host_selection(monkeypatch):
    from digat_amd import evaluate, util
    fake_scoring(monkeypatch)
    dc, model = host_corpus(), types.SimpleNamespace()
    users, pool, k = np.array([0, 3, 4, 1]), np.arange(1, 60), 5
    plain = util.recommend(model, dc, users, pool, k)
    again = util.recommend(model, dc, users, pool, k, diversity=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), "diversity=None is the call without the keyword"
    unit = util.unit_rows(dc.news_embedding)
    for diversity, shortlist, q in ((0.3, None, 0), (0.3, 9, 2), (1.0, 30, 1), (0.0, None, 0)):
        wide = shortlist or min(128, 4 * k)
        i, s, c = util.recommend(model, dc, users, pool, wide)
        sim = evaluate.mmr_gram_stock(i, unit).numpy()
        want = evaluate.mmr_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, 1.0 - diversity,
                                        category=dc.news_category.numpy() if q else None, max_per_category=q, news_num=60)
        got = util.recommend(model, dc, users, pool, k, diversity=diversity, shortlist=shortlist, max_per_category=q)
        V.same((got[1], got[0], got[2]), want, (diversity, shortlist, q))
        if diversity == 0.0:
            V.same((got[1], got[0], got[2]), (plain[1].numpy(), plain[0].numpy(), plain[2].numpy()), "lam = 1: the plain list")
    moved = util.recommend(model, dc, users, pool, k, diversity=1.0)
    assert not torch.equal(moved[0], plain[0]), "full diversity changes some list here"
    none = types.SimpleNamespace(**{f: getattr(dc, f) for f in ("news_embedding", "history", "user_category_indices", "user_graph",
                                                                "user_category_mask")}, news_category=None)
    with pytest.raises(ValueError, match="news_category"):
        util.recommend(model, none, users, pool, k, diversity=0.3, max_per_category=1)
    for bad in (dict(diversity=1.5), dict(diversity=-0.1), dict(diversity=0.3, shortlist=4), dict(diversity=0.3, shortlist=129),
                dict(diversity=0.3, max_per_category=-1), dict(shortlist=20), dict(max_per_category=2)):
        with pytest.raises(ValueError):
            util.recommend(model, dc, users, pool, k, **bad)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_diversity_is_the_plain_call_then_the_host_selection(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), D.dev_set()
    users, k = np.arange(D.USERS), 4
    plain = nrms.recommend(m, dev, users, k=k)
    again = nrms.recommend(m, dev, users, k=k, diversity=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    with torch.no_grad():
        cache, _ = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask)
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    for diversity, shortlist, q in ((0.3, None, 0), (0.6, 12, 1), (0.0, None, 0)):
        wide = shortlist or 4 * k
        i, s, c = nrms.recommend(m, dev, users, k=wide)
        sim = evaluate.mmr_gram_stock(i, cache).numpy()
        want = evaluate.mmr_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, 1.0 - diversity, category=category if q else None,
                                        max_per_category=q, news_num=D.NEWS)
        got = nrms.recommend(m, dev, users, k=k, diversity=diversity, shortlist=shortlist, category=category if q else None,
                             max_per_category=q)
        V.same((got[1], got[0], got[2]), want, (pre, diversity, shortlist, q))
        if q:
            assert all(np.bincount(category[got[0][g, :got[2][g]].numpy()], minlength=5).max(initial=0) <= q for g in users)
        if diversity == 0.0:
            assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2])
    with pytest.raises(ValueError, match="news_category"):
        nrms.recommend(m, dev, users, k=k, diversity=0.3, max_per_category=1)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_config_parses_the_diversity_flags():
    from digat_amd import main
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not any(hasattr(c, f) for f in ("recommend_diversity", "recommend_shortlist", "recommend_max_per_category")), "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_diversity", "0"])
    assert c.recommend_diversity == 0.0 and c.recommend_shortlist == 0 and c.recommend_max_per_category == 0
    c = Config(["--mode", "recommend", "--recommend_diversity", "0.3", "--recommend_shortlist", "50", "--recommend_max_per_category", "2"])
    assert c.recommend_diversity == 0.3 and c.recommend_shortlist == 50 and c.recommend_max_per_category == 2
    for bad in (["--recommend_shortlist", "50"], ["--recommend_max_per_category", "2"], ["--recommend_diversity", "1.5"],
                ["--recommend_diversity", "0.3", "--recommend_shortlist", "-1"]):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend"] + bad)
    with_cat = types.SimpleNamespace(news_category=torch.zeros(4, dtype=torch.int32))
    assert main.recommend_category(with_cat, 2) is with_cat.news_category and main.recommend_category(with_cat, 0) is None
    assert main.recommend_category(types.SimpleNamespace(), 0) is None
    with pytest.raises(ValueError, match="carries none"):
        main.recommend_category(types.SimpleNamespace(news_category=None), 2)
    with pytest.raises(ValueError, match="carries none"):
        main.recommend_category(types.SimpleNamespace(), 1)


def test_lam_one_still_forms_the_diversity_term_where_the_joint_contract_does_not():
    """The two contracts are one greedy pass, but not the same call: ``mmr_select_host`` forms ``rel - fl(mu * pen)`` at every
    ``lam`` (as ``digat_mmr_select`` does), ``rerank_select_host`` forms no term whose weight is zero.  After position 0 is
    picked, position 1's MMR value is ``2 - 0 * inf`` = NaN (key 1), below position 2's."""
    from digat_amd import evaluate
    ids, scores = np.array([[0, 1, 2]]), np.array([[3.0, 2.0, 1.0]], dtype=np.float32)
    sim = np.zeros((1, 3, 3), dtype=np.float32)
    sim[0, 0, 1] = sim[0, 1, 0] = np.inf
    _, got, count = evaluate.mmr_select_host(ids, scores, None, sim, 3, 1.0)
    assert got.tolist() == [[0, 2, 1]] and count.tolist() == [3]
    _, got, count, _ = evaluate.rerank_select_host(ids, scores, None, sim, 3, 1.0, 0.0, 0.0, news_num=3)
    assert got.tolist() == [[0, 1, 2]] and count.tolist() == [3]
