"""CPU suite of the joint re-rank: the numpy contract (``evaluate.rerank_select_host``) against its two reductions
(``mmr_select_host``, ``calibrated_select_host``), a plain-Python brute force and its own robustness certificate on every case the GPU
suite compares exactly (tests/rerank_common.py); the guards, the exports, ``util.rerank`` and both ``recommend(rerank=)`` on CPU
tensors, and the command line."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

import calibrate_common as K
import diversify_common as V
import dot_topk_common as D
import rerank_common as R
from test_calibrate_cpu import fake_scoring, host_corpus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, SHAPE = 0, 1, 2
NEW = ("digat_rerank_select_workspace_bytes", "digat_rerank_select")


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8),
                                                                        np.ascontiguousarray(b).reshape(-1).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", (0.3, 0.7, 1.0))
@pytest.mark.parametrize("q", (0, 2))
def test_without_a_calibration_weight_it_is_mmr_select_host_bit_for_bit(lam, q):
    from digat_amd import evaluate
    for kind, M, k, d in (("unit", 16, 10, 8), ("grid", 128, 128, 16)):
        ids, scores, count, category, target, vec = R.make_case(kind, M, 17, d, groups=12)
        sim = R.host_gram(ids, vec)
        lam32, mu32 = evaluate.mmr_weights(lam)
        want = evaluate.mmr_select_host(ids, scores, count, sim, k, lam, category=category, max_per_category=q)
        got = evaluate.rerank_select_host(ids, scores, count, sim, k, lam32, mu32, 0.0, category=category, max_per_category=q,
                                          return_robust=True)
        assert all(_bits_equal(a, b) for a, b in zip(got[:3], want)), (kind, M, lam, q)
        assert not got[3].any() and got[4].all(), "no target: kl 0; no logarithm: robust"
        if q == 0:                                                    # no category at all
            bare = evaluate.rerank_select_host(ids, scores, count, sim, k, lam32, mu32, 0.0, news_num=len(category))
            assert all(_bits_equal(a, b) for a, b in zip(bare[:3], want))


@pytest.mark.parametrize("M,C,k", [(128, 64, 128), (1024, 17, 128)])
def test_without_a_diversity_weight_it_is_calibrated_select_host_bit_for_bit(M, C, k):
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(0, M, C, groups=R.groups_of(M))
    for lam in (0.3, 0.5):
        lam32, mu32 = evaluate.mmr_weights(lam)
        want = evaluate.calibrated_select_host(ids, scores, count, category, target, k, lam, R.ALPHA, return_robust=True)
        got = evaluate.rerank_select_host(ids, scores, count, None, k, lam32, 0.0, mu32, category=category, target=target, alpha=R.ALPHA,
                                          return_robust=True)
        assert all(_bits_equal(a, b) for a, b in zip(got, want)), (M, lam)


@pytest.mark.parametrize("w", R.WEIGHTS)
@pytest.mark.parametrize("kind,M,C,k,d", R.CASES)
def test_every_case_the_gpu_suite_compares_exactly_is_robust(kind, M, C, k, d, w):
    """Grid vectors: the similarities are exact, so numpy certifies the device's own run.  Unit vectors: the float64 Gram of stock
    PyTorch; the GPU suite certifies again on the device's similarities."""
    from digat_amd import evaluate
    ids, scores, count, category, target, vec = R.make_case(kind, M, C, d)
    if kind == "grid":
        sim = R.host_gram(ids, vec)
        rows = vec[np.where((ids >= 0) & (ids < R.NEWS), ids, 0)][:4]
        assert np.array_equal(sim[:4], np.einsum("gid,gjd->gij", rows, rows[:, ::-1][:, ::-1], dtype=np.float32)), "exact in fp32, in any order"
    else:
        sim = evaluate.mmr_gram_stock(torch.from_numpy(ids), torch.from_numpy(vec).double()).to(torch.float32).numpy()
    s, i, c, kl, robust = evaluate.rerank_select_host(ids, scores, count, sim, k, *w, category=category, target=target, alpha=R.ALPHA,
                                                      return_robust=True)
    assert robust.all(), np.flatnonzero(~robust).tolist()
    assert int(c[1]) == 0 or M == 1, "an empty list is among the cases"
    if M > 1:                                                         # not the plain top-k: the case shows something
        plain = evaluate.rerank_select_host(ids, scores, count, None, k, 1.0, 0.0, 0.0, news_num=len(category))
        live = np.arange(k)[None, :] < c[:, None]
        assert ((i != plain[1]) & live).sum() / max(live.sum(), 1) > 0.2


@pytest.mark.parametrize("w", R.WEIGHTS + ((0.7, 0.3, 0.0), (0.0, 0.5, 0.5)))
@pytest.mark.parametrize("q", (0, 1))
def test_host_selection_matches_the_literal_objective_in_plain_python(w, q):
    from digat_amd import evaluate
    M, C, k, d = 12, 5, 8, 6
    ids, scores, count, category, target, vec = R.make_case("unit", M, C, d, seed=11, groups=20)
    scores[3] = np.random.default_rng(2).standard_normal(M).astype(np.float32)       # the brute force takes finite scores
    sim = R.host_gram(ids, vec)
    wr, wd, wc = (np.float32(x) for x in w)
    s, i, c, kl = evaluate.rerank_select_host(ids, scores, count, sim, k, wr, wd, wc, category=category, target=target, alpha=R.ALPHA,
                                              max_per_category=q)
    for g in range(len(ids)):
        want = R.brute_force(ids[g], scores[g], count[g], sim[g], category, target[g], k, w, R.ALPHA, q)
        assert int(c[g]) == len(want), g
        assert i[g, :len(want)].tolist() == [int(ids[g, p]) for p in want] and _bits_equal(s[g, :len(want)], scores[g, want]), (g, w, q)
        assert (i[g, len(want):] == -1).all() and np.isneginf(s[g, len(want):]).all()


def test_kl_follows_the_calibrated_twin_and_the_cap_holds():
    from digat_amd import evaluate, util
    ids, scores, count, category, target, vec = R.make_case("unit", 65, 17, 33)
    sim = R.host_gram(ids, vec)
    s, i, c, kl = evaluate.rerank_select_host(ids, scores, count, sim, 10, 0.5, 0.3, 0.2, category=category, target=target, max_per_category=2)
    for g in range(len(ids)):
        cats = category[i[g, :c[g]]]
        assert (np.bincount(cats + 1).max(initial=0) <= 2), g
    again = util.calibration_kl(torch.from_numpy(i), torch.from_numpy(c), torch.from_numpy(category), torch.from_numpy(target)).numpy()
    assert _bits_equal(kl, again), "kl is the divergence of the finished list"
    quiet = evaluate.rerank_select_host(ids, scores, count, sim, 10, 0.7, 0.3, 0.0, category=category, target=target)
    bare = evaluate.rerank_select_host(ids, scores, count, sim, 10, 0.7, 0.3, 0.0, category=category)
    assert all(_bits_equal(a, b) for a, b in zip(quiet[:3], bare[:3])) and quiet[3].any() and not bare[3].any()


def test_rerank_weights():
    from digat_amd import evaluate
    w = evaluate.rerank_weights(0.3, 0.2)
    assert all(x.dtype == np.float32 for x in w) and w == (np.float32(1 - 0.3 - 0.2), np.float32(0.3), np.float32(0.2))
    assert evaluate.rerank_weights(0, 0) == (1, 0, 0) and evaluate.rerank_weights(0.3, 0.7)[0] >= 0 and evaluate.rerank_weights(1, 0)[0] == 0
    for bad in ((float("nan"), 0.1), (0.1, float("nan")), (-0.1, 0.2), (0.2, -0.1), (0.6, 0.5), (1.1, 0.0), (0.0, 1.1), (float("inf"), 0)):
        with pytest.raises(ValueError):
            evaluate.rerank_weights(*bad)


def test_host_refuses_bad_arguments():
    from digat_amd import evaluate
    ids, scores, count, category, target, vec = R.make_case("grid", 16, 5, 4, groups=3)
    sim = R.host_gram(ids, vec)
    ok = dict(ids=ids, scores=scores, count=count, sim=sim, k=4, w_rel=0.5, w_div=0.3, w_cal=0.2, category=category, target=target)
    evaluate.rerank_select_host(**ok)
    for bad in (dict(k=0), dict(k=129), dict(scores=scores[:, :5]), dict(ids=ids[0]), dict(count=count[:2]), dict(sim=sim[:, :5]), dict(sim=None),
                dict(w_rel=-0.1), dict(w_div=float("nan")), dict(w_cal=float("inf")), dict(category=None), dict(target=None),
                dict(target=target[:2]), dict(target=np.zeros((3, 65), np.float32)), dict(target=target[0]), dict(alpha=0.0), dict(alpha=1.0),
                dict(max_per_category=-1), dict(category=category[None]),
                dict(ids=np.zeros((1, 1025), np.int64), scores=np.zeros((1, 1025), np.float32), count=None, sim=np.zeros((1, 1025, 1025), np.float32),
                     target=target[:1])):
        with pytest.raises(ValueError):
            evaluate.rerank_select_host(**{**ok, **bad})
    with pytest.raises(ValueError, match="max_per_category needs category"):
        evaluate.rerank_select_host(ids, scores, count, sim, 4, 0.7, 0.3, 0.0, max_per_category=1)


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+DIGAT_ABI_VERSION\s+(\d+)", header).group(1)) == 4
    assert int(re.search(r"#define\s+DIGAT_RERANK_MAX_LIST\s+(\d+)", header).group(1)) == 1024
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    for before in ("digat_topk.inc", "digat_list_softmax.inc", "digat_calibrate.inc"):       # topk_key, the tile sizes, cal_q
        assert hip.index('#include "%s"' % before) < hip.index('#include "digat_rerank.inc"')
    assert L.digat_rerank_select_workspace_bytes(4096, 1024, 128) == 0
    from digat_amd import _ctypes_binding
    ext = open(os.path.join(REPO, "digat_amd", "csrc", "digat_torch_ext.cpp")).read()
    assert len(re.findall(r"\bm\.def\(", ext)) == 12 + 1, "the torch extension stays at 12 functions (and abi_version)"
    assert "rerank" not in ext and not hasattr(_ctypes_binding, "rerank_select")


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)

    def call(ids=p, scores=p, count=p, G=3, M=16, vectors=p, N=100, d=8, category=p, q=0, target=p, Cn=5, w=(0.5, 0.3, 0.2), alpha=0.01, k=10,
             out_i=p, out_s=p, out_c=p, out_kl=p):
        return L.digat_rerank_select(ids, scores, count, G, M, vectors, N, d, category, q, target, Cn, w[0], w[1], w[2], alpha, k, out_i, out_s,
                                     out_c, out_kl, None, 0, None)
    for name in ("ids", "scores", "vectors", "category", "target", "out_i", "out_s", "out_c", "out_kl"):
        assert call(**{name: None}) == ARG, name
    for w in ((-0.1, 0.3, 0.2), (0.5, float("nan"), 0.2), (0.5, 0.3, float("inf")), (0.5, -1.0, 0.0)):
        assert call(w=w) == ARG, w
    for alpha in (0.0, 1.0, -0.5, float("nan")):
        assert call(alpha=alpha) == ARG, alpha
    assert call(G=-1) == ARG and call(N=-1) == ARG and call(q=-1) == ARG
    assert call(q=1, category=None, target=None, w=(0.7, 0.3, 0.0)) == ARG, "a cap needs category"
    for k in (0, -1, 129):
        assert call(k=k) == SHAPE, k
    for M in (0, -1, 1025):
        assert call(M=M) == SHAPE, M
    for d in (0, -1, 513):
        assert call(d=d) == SHAPE, d
    for Cn in (0, -1, 65):
        assert call(Cn=Cn) == SHAPE, Cn
    assert call(G=1 << 31) == SHAPE
    assert call(G=0) == OK
    assert call(G=0, count=None, vectors=None, d=0, w=(0.5, 0.0, 0.5), k=128, M=1024, Cn=64) == OK, "no diversity weight: no vectors, any d"
    assert call(G=0, category=None, target=None, Cn=0, w=(0.7, 0.3, 0.0)) == OK, "no calibration weight, no cap: no category, no target"
    assert call(G=0, target=None, Cn=0, q=2, w=(0.7, 0.3, 0.0)) == OK


# ---------------------------------------------------------------------------------------------------------------------
# util.rerank and recommend(rerank=) on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_util_rerank_on_cpu_tensors_is_the_stock_gram_and_the_twin():
    from digat_amd import evaluate, util
    ids, scores, count, category, target, vec = R.make_case("grid", 65, 17, 33)
    T = torch.from_numpy
    sim = evaluate.mmr_gram_stock(T(ids), T(vec)).numpy()
    for (dv, cl), q in (((0.3, 0.2), 0), ((0.2, 0.4), 2), ((0.3, 0.0), 0), ((0.0, 0.5), 0)):
        w = evaluate.rerank_weights(dv, cl)
        got = util.rerank(T(ids), T(scores), T(count), T(vec), 10, dv, cl, category, target, R.ALPHA, q)
        want = evaluate.rerank_select_host(ids, scores, count, sim, 10, *w, category=category, target=target, alpha=R.ALPHA, max_per_category=q,
                                           news_num=len(vec))
        R.same((got[1], got[0], got[2], got[3]), want, category, target, R.ALPHA, (dv, cl, q))
    bare = util.rerank(T(ids), T(scores), T(count), T(vec), 10, 0.3, 0.0)
    want = evaluate.mmr_select_host(ids, scores, count, sim, 10, np.float32(0.7), news_num=len(vec))
    V.same((bare[1], bare[0], bare[2]), want, "long MMR without categories")
    with pytest.raises(ValueError):
        util.rerank(T(ids), T(scores), T(count), T(vec), 10, 0.3, 0.2)                    # a calibration weight without category / target
    with pytest.raises(ValueError):
        util.rerank(T(ids), T(scores), T(count), T(vec), 10, 0.6, 0.6, category, target)
    with pytest.raises(ValueError):
        util.rerank(T(ids), T(scores), T(count), T(vec), 10, 0.3, 0.2, category[:5], target)


def test_util_recommend_with_rerank_is_the_selection_then_the_twin(monkeypatch):
    from digat_amd import evaluate, util
    fake_scoring(monkeypatch)
    dc, model = host_corpus(), types.SimpleNamespace()
    users, pool, k = np.array([0, 3, 4, 1, 2]), np.arange(1, 300), 5
    plain = util.recommend(model, dc, users, pool, k)
    again = util.recommend(model, dc, users, pool, k, rerank=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), "rerank=None is the call without the keyword"
    category = dc.news_category.numpy()
    target = evaluate.category_share_host(dc.history.numpy()[users], category, 4)
    unit = util.unit_rows(dc.news_embedding)
    for (dv, cl), shortlist, q, alpha in (((0.2, 0.4), None, 0, 0.01), ((0.3, 0.3), 200, 2, 0.1), ((0.3, 0.0), 150, 0, 0.01), ((0.0, 0.0), None, 0, 0.01),
                                          ((0.0, 0.6), 30, 1, 0.01)):
        wide = shortlist or min(1024, 8 * k)
        i, s, c = util.recommend_lists(model, dc, users, pool, wide)
        sim = evaluate.mmr_gram_stock(i, unit).numpy()
        tg = target if cl != 0 else None
        want = evaluate.rerank_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, *evaluate.rerank_weights(dv, cl), category=category, target=tg,
                                           alpha=alpha, max_per_category=q, news_num=300)
        got = util.recommend(model, dc, users, pool, k, rerank=(dv, cl), shortlist=shortlist, max_per_category=q, alpha=alpha)
        V.same((got[1], got[0], got[2]), want[:3], (dv, cl, shortlist, q))
        if (dv, cl) == (0.0, 0.0):
            V.same((got[1], got[0], got[2]), (plain[1].numpy(), plain[0].numpy(), plain[2].numpy()), "weights (1, 0, 0): the plain list")
        else:
            assert not torch.equal(got[0], plain[0])
    given = np.full((5, 4), 0.25, dtype=np.float32)
    mine = (np.arange(300) % 3).astype(np.int64)
    i, s, c = util.recommend_lists(model, dc, users, pool, 40)
    sim = evaluate.mmr_gram_stock(i, unit).numpy()
    got = util.recommend(model, dc, users, pool, k, rerank=(0.2, 0.4), calibration_target=given)
    want = evaluate.rerank_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, *evaluate.rerank_weights(0.2, 0.4), category=category, target=given)
    V.same((got[1], got[0], got[2]), want[:3], "given target")
    got = util.recommend(model, dc, users, pool, k, rerank=(0.2, 0.4), category=mine)
    want = evaluate.rerank_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, *evaluate.rerank_weights(0.2, 0.4), category=mine,
                                       target=evaluate.category_share_host(dc.history.numpy()[users], mine, 3))
    V.same((got[1], got[0], got[2]), want[:3], "given category")
    # refusals
    none = dataclasses.replace(dc, news_category=None)
    with pytest.raises(ValueError, match="news_category"):
        util.recommend(model, none, users, pool, k, rerank=(0.2, 0.4))
    with pytest.raises(ValueError, match="news_category"):
        util.recommend(model, none, users, pool, k, rerank=(0.2, 0.0), max_per_category=1)
    util.recommend(model, none, users, pool, k, rerank=(0.2, 0.0))                          # long MMR needs no category
    for bad in (dict(rerank=(0.2, 0.4), diversity=0.3), dict(rerank=(0.2, 0.4), calibration=0.3), dict(rerank=(0.2, 0.4), sample=1.0)):
        with pytest.raises(ValueError, match="does not combine"):
            util.recommend(model, dc, users, pool, k, **bad)
    for bad in (dict(rerank=(0.6, 0.6)), dict(rerank=(-0.1, 0.2)), dict(rerank=0.3), dict(rerank=(0.1, 0.2, 0.3)), dict(rerank=(0.2, 0.4), shortlist=4),
                dict(rerank=(0.2, 0.4), shortlist=1025), dict(rerank=(0.2, 0.4), alpha=0.0), dict(rerank=(0.2, 0.4), max_per_category=-1),
                dict(rerank=(0.2, 0.4), calibration_target=given[:2]), dict(rerank=(0.2, 0.4), category=np.arange(300))):
        with pytest.raises(ValueError):
            util.recommend(model, dc, users, pool, k, **bad)
    with pytest.raises(ValueError, match="does not combine"):                               # existing behaviour stays
        util.recommend(model, dc, users, pool, k, calibration=0.3, diversity=0.3)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_rerank_is_the_selection_then_the_twin(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), D.dev_set()
    users, k = np.arange(D.USERS), 4
    plain = nrms.recommend(m, dev, users, k=k)
    again = nrms.recommend(m, dev, users, k=k, rerank=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    hist = np.where(dev.history_mask.numpy() != 0, dev.history_ids.numpy(), 0)
    target = evaluate.category_share_host(hist, category, 5)
    vec = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4096)[0]
    for (dv, cl), shortlist, q in (((0.2, 0.4), None, 0), ((0.3, 0.3), 60, 2), ((0.3, 0.0), None, 0)):
        wide = shortlist or 8 * k
        i, s, c = nrms.recommend(m, dev, users, k=wide)
        sim = evaluate.mmr_gram_stock(i, vec.detach().to(torch.float32)).numpy()
        want = evaluate.rerank_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, *evaluate.rerank_weights(dv, cl), category=category,
                                           target=target if cl else None, max_per_category=q, news_num=D.NEWS)
        got = nrms.recommend(m, dev, users, k=k, rerank=(dv, cl), shortlist=shortlist, category=category, max_per_category=q)
        V.same((got[1], got[0], got[2]), want[:3], (pre, dv, cl, shortlist))
    pool = np.tile(np.arange(1, D.NEWS, dtype=np.int64), 3)            # 267 candidates: a shortlist beyond 128
    i, s, c = nrms.shortlist(m, dev, users, candidates=pool, m=200)
    sim = evaluate.mmr_gram_stock(i, vec.detach().to(torch.float32)).numpy()
    got = nrms.recommend(m, dev, users, candidates=pool, k=k, rerank=(0.2, 0.4), shortlist=200, category=category)
    want = evaluate.rerank_select_host(i.numpy(), s.numpy(), c.numpy(), sim, k, *evaluate.rerank_weights(0.2, 0.4), category=category, target=target,
                                       news_num=D.NEWS)
    V.same((got[1], got[0], got[2]), want[:3], "200")
    with pytest.raises(ValueError, match="news_category"):
        nrms.recommend(m, dev, users, k=k, rerank=(0.2, 0.4))
    for bad in (dict(diversity=0.3), dict(calibration=0.3), dict(sample=1.0), dict(index=object())):
        with pytest.raises(ValueError, match="does not combine"):
            nrms.recommend(m, dev, users, k=k, rerank=(0.2, 0.4), category=category, **bad)
    with pytest.raises(ValueError, match="does not combine"):
        nrms.recommend(m, dev, users, k=k, calibration=0.3, diversity=0.3, category=category)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_config_parses_the_rerank_flag_and_keeps_the_old_refusals(capsys):
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not hasattr(c, "recommend_rerank") and not hasattr(c, "recommend_shortlist"), "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_rerank", "0.2,0.4"])
    assert c.recommend_rerank == (0.2, 0.4) and c.recommend_shortlist == 0 and c.recommend_max_per_category == 0
    assert not hasattr(c, "recommend_diversity") and not hasattr(c, "recommend_calibration") and not hasattr(c, "recommend_sample")
    c = Config(["--mode", "recommend", "--recommend_rerank", "0.3,0", "--recommend_shortlist", "1024", "--recommend_max_per_category", "2"])
    assert c.recommend_rerank == (0.3, 0.0) and c.recommend_shortlist == 1024 and c.recommend_max_per_category == 2
    c = Config(["--mode", "recommend", "--recommend_calibration", "0.5"])
    assert not hasattr(c, "recommend_rerank") and not hasattr(c, "recommend_max_per_category")
    old = "--recommend_shortlist and --recommend_max_per_category need --recommend_diversity (0 for the cap alone) or --recommend_report"
    mine = "--recommend_rerank does not combine"
    for bad, text in ((["--recommend_shortlist", "50"], old), (["--recommend_max_per_category", "2"], old),
                      (["--recommend_calibration", "0.5", "--recommend_diversity", "0.3"], "--recommend_calibration does not combine"),
                      (["--recommend_rerank", "0.2,0.4", "--recommend_diversity", "0.3"], mine),
                      (["--recommend_rerank", "0.2,0.4", "--recommend_calibration", "0.3"], mine),
                      (["--recommend_rerank", "0.2,0.4", "--recommend_sample", "1.0"], mine),
                      (["--recommend_rerank", "0.2,0.4", "--recommend_report", "0,0.1"], mine),
                      (["--recommend_rerank", "0.2"], "needs two values"), (["--recommend_rerank", "0.6,0.6"], "needs two values"),
                      (["--recommend_rerank=-0.1,0.2"], "needs two values"), (["--recommend_rerank", "a,b"], "separated by a comma"),
                      (["--recommend_rerank", "0.2,0.4", "--recommend_shortlist", "-1"], "must not be negative")):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend"] + bad)
        assert text in capsys.readouterr().err, bad


def test_recommend_lines_passes_the_pair_through(monkeypatch):
    from digat_amd import main, util
    fake_scoring(monkeypatch)
    dc, model = host_corpus(), types.SimpleNamespace()
    lines = main.recommend_lines(model, dc, 5, 64, shortlist=60, max_per_category=2, rerank=(0.2, 0.4))
    pool, users = torch.arange(1, 300), torch.arange(6)
    ids, _, count = util.recommend(model, dc, users, pool, 5, batch_size=64, rerank=(0.2, 0.4), shortlist=60, category=dc.news_category,
                                   max_per_category=2)
    assert lines == ['%d [%s]' % (g + 1, ','.join(str(int(v)) for v in ids[g, :count[g]])) for g in range(6)]
    assert lines != main.recommend_lines(model, dc, 5, 64)


# ---------------------------------------------------------------------------------------------------------------------
# one contract, one ladder
# ---------------------------------------------------------------------------------------------------------------------
def test_the_three_host_contracts_reach_one_core(monkeypatch):
    from digat_amd import evaluate
    seen = []

    def recorder(idv, sc, count, S, k, wr, wd, wc, form_div, form_cal, **rest):
        seen.append((form_div, form_cal))
        G = idv.shape[0]
        return (np.zeros((G, k), np.float32), np.zeros((G, k), np.int64), np.zeros(G, np.int32), np.zeros(G, np.float32), np.ones(G, bool))
    monkeypatch.setattr(evaluate, "_greedy_select_host", recorder)
    ids, scores = np.arange(6).reshape(2, 3), np.ones((2, 3), dtype=np.float32)
    sim, category, target = np.zeros((2, 3, 3), dtype=np.float32), np.arange(6) % 2, np.full((2, 2), 0.5, dtype=np.float32)
    for lam in (0.3, 1.0):                                       # lam = 1: a zero weight, the term is formed all the same
        assert len(evaluate.mmr_select_host(ids, scores, None, sim, 2, lam)) == 3
        assert seen == [(True, False)]
        seen.clear()
        assert len(evaluate.calibrated_select_host(ids, scores, None, category, target, 2, lam)) == 4
        assert len(evaluate.calibrated_select_host(ids, scores, None, category, target, 2, lam, return_robust=True)) == 5
        assert seen == [(False, True)] * 2
        seen.clear()
    for w_div, w_cal in ((0.3, 0.2), (0.0, 0.2), (0.3, 0.0), (0.0, 0.0)):
        evaluate.rerank_select_host(ids, scores, None, sim, 2, 0.5, w_div, w_cal, category=category, target=target)
        assert seen == [(w_div != 0, w_cal != 0)]
        seen.clear()


RERANK_KNOBS = dict(diversity=0.3, calibration=0.3, sample=1.0, rerank=(0.2, 0.4))


@pytest.mark.parametrize("which", ("util", "nrms"))
def test_the_refusal_table_holds_before_anything_is_scored(which, monkeypatch):
    """Every pair of knobs that does not combine, and every argument given without its knob, is refused — with the text the ladder
    has always used — before the model's selection is called."""
    import itertools
    from digat_amd import nrms, util

    def never(*args, **kwargs):
        raise AssertionError("scored before the refusal")
    if which == "util":
        monkeypatch.setattr(util, "recommend_lists", never)
        dc = host_corpus()
        call = lambda **kw: util.recommend(types.SimpleNamespace(), dc, np.arange(5), np.arange(1, 300), 5, **kw)
        knobs, users, news = dict(RERANK_KNOBS), 5, 300
        alone = {}
    else:
        monkeypatch.setattr(nrms, "_retrieve", never)
        monkeypatch.setattr(nrms, "_retrieve_indexed", never)
        m, dev = D.model("nrms"), D.dev_set()
        call = lambda **kw: nrms.recommend(m, dev, np.arange(D.USERS), k=4, **kw)
        knobs, users, news = dict(RERANK_KNOBS, index=object()), D.USERS, D.NEWS
        alone = {"refine": (64, "belongs to an indexed call")}
    for a, b in itertools.combinations(knobs, 2):
        if {a, b} == {"diversity", "index"}:
            continue                                             # the one pair that composes: checked below
        with pytest.raises(ValueError, match="does not combine"):
            call(**{a: knobs[a], b: knobs[b]})
    alone.update(calibration_target=(np.full((users, 4), 0.25, dtype=np.float32), "belongs to a calibrated call"),
                 shortlist=(20, "belong to a diversified call"), category=(np.zeros(news, dtype=np.int64), "belong to a diversified call"),
                 max_per_category=(1, "belong to a diversified call"))
    for name, (value, text) in alone.items():
        with pytest.raises(ValueError, match=text):
            call(**{name: value})
    with pytest.raises(AssertionError, match="scored"):          # the fake is live: a call that is not refused reaches it
        call(diversity=0.3)
    if which == "nrms":
        with pytest.raises(AssertionError, match="scored"):      # diversity composes with index: its shortlist is the indexed call's
            call(diversity=0.3, index=knobs["index"])
