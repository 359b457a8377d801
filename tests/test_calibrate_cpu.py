"""CPU suite of calibrated top-k: the host contract (``evaluate.calibrated_select_host``) against a plain-Python float64 brute force
of the literal objective and against the plain top-k where the contract says so; ``category_share`` against a loop; the robustness
of EVERY input the GPU suite compares exactly (tests/test_hip_calibrate.py: same generator, same seeds); the library's refusals and
symbols; ``util.recommend`` / ``nrms.recommend`` with ``calibration=`` on CPU tensors; the CLI flag."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import calibrate_common as K
import diversify_common as V
import dot_topk_common as D
from conftest import REPO

OK, ARG, SHAPE = 0, 1, 2
NEW = ("digat_calibrated_select_workspace_bytes", "digat_calibrated_select")
ALPHA = 0.01


# ---------------------------------------------------------------------------------------------------------------------
# calibrated_select_host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
def test_host_selection_matches_the_literal_objective_in_plain_python(lam):
    """Robust lists of finite scores, M <= 12, C <= 4: the step of the twin (two logarithms per category, the common term
    dropped, float32 values) picks what the whole objective ``lam sum(s) - mu KL(p || q)`` in float64 picks."""
    from digat_amd import evaluate
    checked = 0
    for seed in range(24):
        rng = np.random.default_rng(100 + seed)
        M, Cn, k, alpha = int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(1, 13)), (0.01, 0.1, 0.5)[seed % 3]
        ids, scores, count, category, target = K.make_case(seed, M, Cn, groups=6, N=40)
        s, i, c, kl, robust = evaluate.calibrated_select_host(ids, scores, count, category, target, k, lam, alpha, return_robust=True)
        assert s.dtype == np.float32 and i.dtype == np.int64 and c.dtype == np.int32 and kl.dtype == np.float32 and robust.dtype == bool
        assert s.shape == i.shape == (6, k) and c.shape == kl.shape == robust.shape == (6,)
        for g in range(6):
            if not robust[g] or not np.isfinite(scores[g]).all():        # the running sum of the literal objective needs finite scores
                continue
            mine = K.brute_force(ids[g], scores[g], count[g], category, target[g], k, lam, alpha)
            m = len(mine)
            assert c[g] == m and i[g, :m].tolist() == [int(ids[g][p]) for p in mine], (seed, g)
            assert V.bits(s[g, :m]).tolist() == V.bits(scores[g][mine]).tolist(), (seed, g)            # the input score bits
            assert np.all(i[g, m:] == -1) and np.all(np.isneginf(s[g, m:])), (seed, g)
            checked += 1
    assert checked >= 60


def _elements_topk(ids, scores, count, N, k, host):
    """The plain top-k of every list's elements through a segment selection of ``evaluate``."""
    keep = [np.flatnonzero((np.arange(ids.shape[1]) < count[g]) & (ids[g] >= 0) & (ids[g] < N)) for g in range(len(ids))]
    start = np.concatenate([[0], np.cumsum([len(p) for p in keep])]).astype(np.int64)
    flat_s = np.concatenate([scores[g][p] for g, p in enumerate(keep)]).astype(np.float32)
    flat_i = np.concatenate([ids[g][p] for g, p in enumerate(keep)]).astype(np.int64)
    return host(flat_s, start, k, ids=flat_i)


@pytest.mark.parametrize("M,k,host", [(40, 10, "topk_segments_host"), (128, 128, "topk_segments_host"), (300, 100, "shortlist_segments_host")])
def test_lam_one_and_a_zero_target_are_the_plain_topk(M, k, host):
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(7, M, 9, groups=8, grid=True)
    want = _elements_topk(ids, scores, count, K.NEWS, k, getattr(evaluate, host))
    got = evaluate.calibrated_select_host(ids, scores, count, category, target, k, 1.0, ALPHA)
    V.same(got[:3], want, "lam = 1")
    zero = evaluate.calibrated_select_host(ids, scores, count, category, np.zeros_like(target), k, 0.3, ALPHA)
    V.same(zero[:3], want, "zero target")
    assert (zero[3] == 0).all()
    assert np.array_equal(got[1][4], evaluate.calibrated_select_host(ids, scores, count, category, target, k, 0.3, ALPHA)[1][4]), "row 4 is all zero"


def test_one_category_that_holds_every_element_is_the_plain_topk():
    """C = 1, every element categorised: all candidates of a step share one gain.  Scores on a grid of 1/8 and lam = 0.5, so that
    the shared gain neither splits a tie nor merges two scores."""
    from digat_amd import evaluate
    rng = np.random.default_rng(3)
    ids, count = V.make_lists(rng, 6, 50, 200)
    scores = (np.round(rng.standard_normal((6, 50)) * 8) / 8 + 0.0).astype(np.float32)
    category = np.zeros(200, dtype=np.int32)
    target = np.full((6, 1), 0.8, dtype=np.float32)
    got = evaluate.calibrated_select_host(ids, scores, count, category, target, 20, 0.5, ALPHA)
    V.same(got[:3], _elements_topk(ids, scores, count, 200, 20, evaluate.topk_segments_host), "C = 1")
    full = got[2] > 0                                               # q = 0.99 + 0.01 * 0.8 whatever the list: nothing is normalised
    assert np.allclose(got[3][full], 0.8 * np.log(0.8 / 0.998), rtol=1e-6) and (got[3][~full] > 0).all()


def test_kl_is_the_divergence_of_the_finished_list():
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(11, 64, 6, groups=9)
    s, i, c, kl = evaluate.calibrated_select_host(ids, scores, count, category, target, 12, 0.5, 0.05)
    for g in range(9):
        p = [float(x) if np.isfinite(x) and x > 0 else 0.0 for x in target[g]]
        cg = category[i[g, :c[g]]]
        n = [int(np.sum(cg == j)) for j in range(6)]
        want = sum(p[j] * (np.log(p[j]) - np.log(0.95 * n[j] / max(int(c[g]), 1) + 0.05 * p[j])) for j in range(6) if p[j] > 0)
        assert abs(float(kl[g]) - want) <= 1e-6 * max(1.0, abs(want)), g
    assert kl[4] == 0 and c[1] == 0


def test_every_input_the_gpu_suite_compares_exactly_is_robust():
    """The GPU suite holds picks to the twin bit for bit; that is sound on robust lists only (``calibrated_select_host``): every
    case it builds, from the same generator and seeds — no list is left out."""
    from digat_amd import evaluate
    cases = [(K.make_case(K.seed_of(M, Cn, k, lam), M, Cn), k, lam) for M, Cn, k in K.SHAPES for lam in K.LAMS]
    for M, Cn, k in K.SHAPES:                                            # count=None
        ids, scores, _, category, target = K.make_case(K.seed_of(M, Cn, k, K.LAMS[0]), M, Cn)
        cases.append(((ids, scores, None, category, target), min(k, 10), K.LAMS[0]))
    cases += [(K.make_case(seed, M, 16, grid=True, uniform=True), k, 0.5) for M, k, seed in K.GRID_CASES]
    cases += [(K.make_case(3, 16, 17, groups=600), 10, 0.5)]
    for (ids, scores, count, category, target), k, lam in cases:
        robust = evaluate.calibrated_select_host(ids, scores, count, category, target, k, lam, ALPHA, return_robust=True)[4]
        assert robust.all(), (ids.shape, target.shape[1], k, lam, np.flatnonzero(~robust).tolist())
    # and the flag does see a near-tie: two categories whose gains differ in the last bits, equal scores
    ids = np.array([[0, 1]], dtype=np.int64)
    near = evaluate.calibrated_select_host(ids, np.zeros((1, 2), np.float32), None, np.array([0, 1], np.int32),
                                           np.array([[0.5, np.nextafter(np.float32(0.5), np.float32(1))]], np.float32), 1, 0.5, ALPHA,
                                           return_robust=True)
    assert not near[4][0]
    tie = evaluate.calibrated_select_host(ids, np.zeros((1, 2), np.float32), None, np.array([0, 1], np.int32),
                                          np.array([[0.5, 0.5]], np.float32), 1, 0.5, ALPHA, return_robust=True)
    assert tie[4][0] and tie[1][0, 0] == 0, "a true tie goes to the lower position"


def test_host_refuses_bad_arguments():
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(0, 20, 5, groups=4)
    call = lambda **kw: evaluate.calibrated_select_host(**{**dict(ids=ids, scores=scores, count=count, category=category, target=target, k=5,
                                                                  lam=0.5, alpha=ALPHA), **kw})
    call()
    for bad, match in ((dict(k=0), "k must be"), (dict(k=129), "k must be"), (dict(lam=1.5), "lam must"), (dict(lam=float("nan")), "lam must"),
                       (dict(alpha=0.0), "alpha must"), (dict(alpha=1.0), "alpha must"), (dict(alpha=float("nan")), "alpha must"),
                       (dict(scores=scores[:, :5]), r"\[G, M\]"), (dict(count=count[:2]), "count must"), (dict(category=None), "category must"),
                       (dict(category=category.reshape(-1, 1)), "category must"), (dict(target=target[:2]), "target must"),
                       (dict(target=np.zeros((4, 65), np.float32)), "target must"), (dict(target=np.zeros((4, 0), np.float32)), "target must"),
                       (dict(ids=np.zeros((4, 1025), np.int64), scores=np.zeros((4, 1025), np.float32)), r"\[G, M\]")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    assert evaluate.CAL_MAX_LIST == evaluate.SHORTLIST_MAX_K == 1024 and evaluate.CAL_MAX_CATEGORIES == 64


# ---------------------------------------------------------------------------------------------------------------------
# category_share
# ---------------------------------------------------------------------------------------------------------------------
def test_category_share_against_a_loop():
    from digat_amd import evaluate
    rng = np.random.default_rng(2)
    N, Cn, G, H = 50, 6, 12, 9
    category = rng.integers(-1, Cn + 2, size=N).astype(np.int32)
    history = rng.integers(0, N, size=(G, H)).astype(np.int64)
    history[rng.random((G, H)) < 0.3] = 0                              # the pad
    history[2] = 0                                                      # an empty history
    history[3, :2] = (N + 4, -3)                                        # ids outside the table count for nothing
    def loop(pad):
        want = np.zeros((G, Cn), dtype=np.float32)
        for g in range(G):
            counts = [0] * Cn
            for h in history[g]:
                if h != pad and 0 <= h < N and 0 <= category[h] < Cn:
                    counts[category[h]] += 1
            if sum(counts):
                want[g] = np.array(counts, dtype=np.float32) / np.float32(sum(counts))
        return want
    want = loop(0)
    host = evaluate.category_share_host(history, category, Cn)
    dev = evaluate.category_share(torch.from_numpy(history), torch.from_numpy(category), Cn)
    assert host.dtype == np.float32 and dev.dtype == torch.float32 and tuple(dev.shape) == (G, Cn)
    assert np.array_equal(host, want) and np.array_equal(dev.numpy(), want)
    assert not want[2].any() and np.allclose(want[np.r_[0:2, 3:G]].sum(axis=1), 1.0)
    for pad in (-1, int(history[0, 0]), int(history[5, 1])):
        assert np.array_equal(evaluate.category_share_host(history, category, Cn, pad_id=pad), loop(pad)), pad
        assert np.array_equal(evaluate.category_share(torch.from_numpy(history), torch.from_numpy(category), Cn, pad_id=pad).numpy(), loop(pad)), pad
    for bad in (dict(C=0), dict(C=65)):
        with pytest.raises(ValueError, match="C must be"):
            evaluate.category_share_host(history, category, **bad)
    with pytest.raises(ValueError, match="history must be"):
        evaluate.category_share(torch.from_numpy(history[0]), torch.from_numpy(category), Cn)


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
    assert int(re.search(r"#define\s+DIGAT_CALIBRATE_MAX_LIST\s+(\d+)", header).group(1)) == 1024
    assert int(re.search(r"#define\s+DIGAT_CALIBRATE_MAX_CATEGORIES\s+(\d+)", header).group(1)) == 64
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_topk.inc"') < hip.index('#include "digat_calibrate.inc"')          # it uses topk_key
    assert L.digat_calibrated_select_workspace_bytes(4096, 1024, 64, 128) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)

    def call(ids=p, scores=p, count=p, G=3, M=16, category=p, N=100, target=p, Cn=5, lam=0.5, mu=0.5, alpha=0.01, k=10, out_i=p, out_s=p,
             out_c=p, out_kl=p):
        return L.digat_calibrated_select(ids, scores, count, G, M, category, N, target, Cn, lam, mu, alpha, k, out_i, out_s, out_c, out_kl,
                                         None, 0, None)
    for name in ("ids", "scores", "category", "target", "out_i", "out_s", "out_c", "out_kl"):
        assert call(**{name: None}) == ARG, name
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(lam=lam) == ARG, lam
    for alpha in (0.0, 1.0, -0.5, float("nan"), float("inf")):
        assert call(alpha=alpha) == ARG, alpha
    assert call(G=-1) == ARG and call(N=-1) == ARG
    for k in (0, -1, 129):
        assert call(k=k) == SHAPE, k
    for M in (0, -1, 1025):
        assert call(M=M) == SHAPE, M
    for Cn in (0, -1, 65):
        assert call(Cn=Cn) == SHAPE, Cn
    assert call(G=1 << 31) == SHAPE
    assert call(G=0) == OK
    assert call(G=0, count=None, lam=0.0, mu=1.0, k=128, M=1024, Cn=64) == OK


# ---------------------------------------------------------------------------------------------------------------------
# recommend(calibration=) on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def host_corpus(news_num=300, I=6, H=5, Cn=4, d=8, seed=0):
    from digat_amd import util
    rng = np.random.default_rng(seed)
    hist = rng.integers(1, news_num, size=(I, H))
    hist[2] = 0                                                     # a user without a history: the plain top-k
    hist[3, 3:] = 0
    return util.DeviceCorpus(
        news_embedding=torch.from_numpy(rng.standard_normal((news_num, d)).astype(np.float32)),
        news_node_ID=torch.zeros(news_num, 2, dtype=torch.int64), news_graph=torch.zeros(news_num, 2, 2, dtype=torch.bool),
        news_graph_mask=torch.zeros(news_num, 2, dtype=torch.bool), history=torch.from_numpy(hist),
        user_graph=torch.zeros(I, H + Cn, H + Cn, dtype=torch.bool), user_category_mask=torch.zeros(I, Cn + 1, dtype=torch.bool),
        user_category_indices=torch.from_numpy(rng.integers(0, Cn + 1, size=(I, H))), row_impression=torch.zeros(0, dtype=torch.int64),
        row_candidate=torch.zeros(0, dtype=torch.int64), category_num=Cn,
        news_category=torch.from_numpy(rng.integers(0, Cn, size=news_num).astype(np.int32)))


def fake_scoring(monkeypatch):
    """``util.score_rows`` replaced by a fixed function of (user, candidate), the news-side refresh by nothing: the selection stages
    of ``util.recommend`` run on CPU tensors."""
    from digat_amd import util

    def score_rows(model, view, start, end, batch_size, *a, **kw):
        return torch.sin((view.row_impression * 37 + view.row_candidate * 11).to(torch.float32)) * 2
    monkeypatch.setattr(util, "score_rows", score_rows)
    monkeypatch.setattr(util, "refresh_news_side", lambda model, dc, batch_size: None)


def test_util_recommend_with_calibration_is_the_selection_then_the_twin(monkeypatch):
    from digat_amd import evaluate, util
    fake_scoring(monkeypatch)
    dc, model = host_corpus(), types.SimpleNamespace()
    users, pool, k = np.array([0, 3, 4, 1, 2]), np.arange(1, 300), 5
    plain = util.recommend(model, dc, users, pool, k)
    again = util.recommend(model, dc, users, pool, k, calibration=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), "calibration=None is the call without the keyword"
    category = dc.news_category.numpy()
    target = evaluate.category_share_host(dc.history.numpy()[users], category, 4)
    assert not target[4].any() and target[:4].any(axis=1).all()
    for calibration, shortlist, alpha in ((0.5, None, 0.01), (0.8, 200, 0.1), (1.0, 30, 0.01), (0.0, None, 0.01)):
        wide = shortlist or min(1024, 8 * k)
        i, s, c = util.recommend_lists(model, dc, users, pool, wide)
        if wide <= 128:
            assert all(torch.equal(a, b) for a, b in zip((i, s, c), util.recommend(model, dc, users, pool, wide)))
        want = evaluate.calibrated_select_host(i.numpy(), s.numpy(), c.numpy(), category, target, k, 1.0 - calibration, alpha)
        got = util.recommend(model, dc, users, pool, k, calibration=calibration, shortlist=shortlist, alpha=alpha)
        V.same((got[1], got[0], got[2]), want[:3], (calibration, shortlist))
        assert torch.equal(got[0][4], plain[0][4]), "no history: the plain list"
        if calibration == 0.0:
            V.same((got[1], got[0], got[2]), (plain[1].numpy(), plain[0].numpy(), plain[2].numpy()), "lam = 1: the plain list")
        if calibration == 1.0:
            kl_got = util.calibration_kl(got[0], got[2], dc.news_category, torch.from_numpy(target), alpha).numpy()
            kl_plain = util.calibration_kl(plain[0], plain[2], dc.news_category, torch.from_numpy(target), alpha).numpy()
            assert (kl_got <= kl_plain).all() and (kl_got[:4] < kl_plain[:4]).any()
            assert not torch.equal(got[0], plain[0])
    # a target of the caller's, a category array of the caller's
    given = np.full((5, 4), 0.25, dtype=np.float32)
    i, s, c = util.recommend_lists(model, dc, users, pool, 40)
    got = util.recommend(model, dc, users, pool, k, calibration=0.5, calibration_target=given)
    V.same((got[1], got[0], got[2]), evaluate.calibrated_select_host(i.numpy(), s.numpy(), c.numpy(), category, given, k, 0.5)[:3], "given target")
    mine = (np.arange(300) % 3).astype(np.int64)
    got = util.recommend(model, dc, users, pool, k, calibration=0.5, category=mine)
    want = evaluate.calibrated_select_host(i.numpy(), s.numpy(), c.numpy(), mine, evaluate.category_share_host(dc.history.numpy()[users], mine, 3),
                                           k, 0.5)
    V.same((got[1], got[0], got[2]), want[:3], "given category")
    # refusals
    none = types.SimpleNamespace(**{f: getattr(dc, f) for f in ("news_embedding", "history", "user_category_indices", "user_graph",
                                                                "user_category_mask")}, news_category=None)
    with pytest.raises(ValueError, match="news_category"):
        util.recommend(model, none, users, pool, k, calibration=0.3)
    with pytest.raises(ValueError, match="at most 64"):
        util.recommend(model, dc, users, pool, k, calibration=0.3, category=np.arange(300))
    for bad in (dict(calibration=1.5), dict(calibration=-0.1), dict(calibration=0.3, shortlist=4), dict(calibration=0.3, shortlist=1025),
                dict(calibration=0.3, diversity=0.3), dict(calibration=0.3, max_per_category=1), dict(calibration=0.3, alpha=0.0),
                dict(calibration_target=given), dict(calibration=0.3, calibration_target=given[:2]), dict(shortlist=20)):
        with pytest.raises(ValueError):
            util.recommend(model, dc, users, pool, k, **bad)
    with pytest.raises(ValueError, match=r"M <= 128|1 <= M"):
        util.calibration_kl(torch.zeros((2, 129), dtype=torch.int64), None, dc.news_category, torch.from_numpy(given[:2]))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_calibration_is_the_selection_then_the_twin(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), D.dev_set()
    users, k = np.arange(D.USERS), 4
    plain = nrms.recommend(m, dev, users, k=k)
    again = nrms.recommend(m, dev, users, k=k, calibration=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    hist = np.where(dev.history_mask.numpy() != 0, dev.history_ids.numpy(), 0)
    target = evaluate.category_share_host(hist, category, 5)
    for calibration, shortlist in ((0.5, None), (0.7, 60), (0.0, None)):
        wide = shortlist or 8 * k
        i, s, c = nrms.recommend(m, dev, users, k=wide)
        want = evaluate.calibrated_select_host(i.numpy(), s.numpy(), c.numpy(), category, target, k, 1.0 - calibration)
        got = nrms.recommend(m, dev, users, k=k, calibration=calibration, shortlist=shortlist, category=category)
        V.same((got[1], got[0], got[2]), want[:3], (pre, calibration, shortlist))
        if calibration == 0.0:
            assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2])
    pool = np.tile(np.arange(1, D.NEWS, dtype=np.int64), 3)            # 267 candidates: a shortlist beyond 128
    i, s, c = nrms.shortlist(m, dev, users, candidates=pool, m=200)
    got = nrms.recommend(m, dev, users, candidates=pool, k=k, calibration=0.5, shortlist=200, category=category)
    V.same((got[1], got[0], got[2]), evaluate.calibrated_select_host(i.numpy(), s.numpy(), c.numpy(), category, target, k, 0.5)[:3], "200")
    with pytest.raises(ValueError, match="news_category"):
        nrms.recommend(m, dev, users, k=k, calibration=0.3)
    with pytest.raises(ValueError, match="does not combine"):
        nrms.recommend(m, dev, users, k=k, calibration=0.3, diversity=0.3, category=category)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_config_parses_the_calibration_flag_and_keeps_the_old_refusals(capsys):
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not hasattr(c, "recommend_calibration") and not hasattr(c, "recommend_shortlist"), "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_calibration", "0.5"])
    assert c.recommend_calibration == 0.5 and c.recommend_shortlist == 0
    assert not hasattr(c, "recommend_diversity") and not hasattr(c, "recommend_max_per_category")
    c = Config(["--mode", "recommend", "--recommend_calibration", "0", "--recommend_shortlist", "1024"])
    assert c.recommend_calibration == 0.0 and c.recommend_shortlist == 1024
    c = Config(["--mode", "recommend", "--recommend_diversity", "0.3", "--recommend_shortlist", "50"])
    assert c.recommend_diversity == 0.3 and c.recommend_shortlist == 50 and not hasattr(c, "recommend_calibration")
    old = "--recommend_shortlist and --recommend_max_per_category need --recommend_diversity (0 for the cap alone) or --recommend_report"
    for bad, text in ((["--recommend_shortlist", "50"], old), (["--recommend_max_per_category", "2"], old),
                      (["--recommend_calibration", "0.5", "--recommend_max_per_category", "2"], old),
                      (["--recommend_diversity", "1.5"], "--recommend_diversity must lie in [0, 1]"),
                      (["--recommend_diversity", "0.3", "--recommend_shortlist", "-1"], "must not be negative"),
                      (["--recommend_calibration", "1.5"], "--recommend_calibration must lie in [0, 1]"),
                      (["--recommend_calibration", "0.5", "--recommend_diversity", "0.3"], "does not combine"),
                      (["--recommend_calibration", "0.5", "--recommend_report", "0,0.1"], "does not combine"),
                      (["--recommend_calibration", "0.5", "--recommend_shortlist", "-1"], "must not be negative")):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend"] + bad)
        assert text in capsys.readouterr().err, bad
