"""GPU suite: the joint re-rank kernel (``digat_rerank_select``) and ``recommend(rerank=)`` on it.  The selection is held exactly — ids,
score bits, counts, fills — to the host contract (``evaluate.rerank_select_host``) fed the device's OWN similarities
(``evaluate.dot_scores``: the kernel's chain has those bits), on the cases tests/test_rerank_cpu.py holds to be robust (same
generator, same seed: tests/rerank_common.py); the twin is certified again here, on the similarities it is fed."""
import functools

import numpy as np
import pytest
import torch

import calibrate_common as K
import diversify_common as V
import dot_topk_common as D
import rerank_common as R
from test_hip_calibrate import _corpus, _model
from test_hip_diversify import device_gram, float_case

pytestmark = pytest.mark.gpu

ALPHA = R.ALPHA


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(np.uint8)


def _identical(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), what


@functools.lru_cache(maxsize=None)
def _case(kind, M, C, d):
    """The case, its device tensors and the device's own Gram — computed once, shared by both weight triples, never written to."""
    case = R.make_case(kind, M, C, d)
    dev = tuple(_t(x) for x in case)
    sim = device_gram(dev[0], dev[5])
    return case, dev, sim


@pytest.mark.parametrize("w", R.WEIGHTS)
@pytest.mark.parametrize("kind,M,C,k,d", R.CASES)
def test_selection_is_exact_against_the_twin_on_the_devices_own_similarities(kind, M, C, k, d, w):
    from digat_amd import evaluate
    (ids, scores, count, category, target, vec), (IDS, SC, CNT, CAT, TGT, VEC), sim = _case(kind, M, C, d)
    if kind == "grid":
        assert np.array_equal(sim, R.host_gram(ids, vec)), "grid vectors: every product sum is exact"
    got = evaluate.rerank_select(IDS, SC, CNT, VEC, k, *w, category=CAT, target=TGT, alpha=ALPHA)
    assert all(t.is_cuda for t in got)
    want = evaluate.rerank_select_host(ids, scores, count, sim, k, *w, category=category, target=target, alpha=ALPHA, return_robust=True)
    robust = want[4]
    assert (~robust).sum() <= 1, ("the CPU suite predicts every list robust", np.flatnonzero(~robust).tolist())
    R.same(got, want, category, target, ALPHA, (kind, M, C, k, d, w), lists=np.flatnonzero(robust))
    gs, gi, gc = (t.cpu().numpy() for t in got[:3])
    for g in np.flatnonzero(~robust):                                  # left out: still the twin's count, distinct positions of its own elements
        assert gc[g] == want[2][g]
        left = [(int(i), np.float32(s).view(np.uint32)) for i, s in zip(ids[g, :count[g]], scores[g, :count[g]]) if 0 <= i < R.NEWS]
        for i, s in zip(gi[g, :gc[g]], gs[g, :gc[g]]):
            left.remove((int(i), np.float32(s).view(np.uint32)))
    if w == R.WEIGHTS[0] and M in (65, 1024):                          # count=None is M; a cap
        got = evaluate.rerank_select(IDS, SC, None, VEC, min(k, 10), *w, category=CAT, target=TGT, alpha=ALPHA, max_per_category=2)
        want = evaluate.rerank_select_host(ids, scores, None, sim, min(k, 10), *w, category=category, target=target, alpha=ALPHA,
                                           max_per_category=2, return_robust=True)
        R.same(got, want, category, target, ALPHA, "count None, cap 2", lists=np.flatnonzero(want[4]))
        assert want[4].sum() >= len(want[4]) - 1


@pytest.mark.parametrize("M", (16, 128))
@pytest.mark.parametrize("q", (0, 2))
def test_without_a_calibration_weight_it_is_mmr_select(M, q):
    from digat_amd import evaluate
    vec, ids, count, scores, category = float_case(7, 37, M, 900, 100)
    k = min(M, 100)
    for lam in (0.3, 0.7):
        lam32, mu32 = evaluate.mmr_weights(lam)
        want = evaluate.mmr_select(_t(ids), _t(scores), _t(count), _t(vec), k, lam, category=_t(category), max_per_category=q)
        got = evaluate.rerank_select(_t(ids), _t(scores), _t(count), _t(vec), k, lam32, mu32, 0.0, category=_t(category), max_per_category=q)
        _identical(got[:3], want, (M, q, lam))
        assert not got[3].any()
        if q == 0:
            bare = evaluate.rerank_select(_t(ids), _t(scores), _t(count), _t(vec), k, lam32, mu32, 0.0)
            _identical(bare[:3], want, "no category at all")


@pytest.mark.parametrize("M,C,k", [(128, 64, 128), (1024, 17, 128)])
def test_without_a_diversity_weight_it_is_calibrated_select(M, C, k):
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(0, M, C, groups=R.groups_of(M))
    for lam in (0.3, 0.5):
        lam32, mu32 = evaluate.mmr_weights(lam)
        want = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(target), k, lam, ALPHA)
        got = evaluate.rerank_select(_t(ids), _t(scores), _t(count), None, k, lam32, 0.0, mu32, category=_t(category), target=_t(target),
                                     alpha=ALPHA)
        _identical(got, want, (M, lam))


def test_a_padded_list_two_calls_and_a_list_alone_give_the_same_bits():
    from digat_amd import evaluate
    (ids, scores, count, category, target, vec), (IDS, SC, CNT, CAT, TGT, VEC), _ = _case("grid", 128, 64, 32)
    k, w = 20, R.WEIGHTS[0]
    whole = evaluate.rerank_select(IDS, SC, CNT, VEC, k, *w, category=CAT, target=TGT, alpha=ALPHA, max_per_category=3)
    again = evaluate.rerank_select(IDS, SC, CNT, VEC, k, *w, category=CAT, target=TGT, alpha=ALPHA, max_per_category=3)
    _identical(whole, again, "two calls")
    pad_i = np.concatenate([ids, np.full((len(ids), 1), 5, np.int64)], axis=1)                     # M = 129: a slot beyond every count
    pad_s = np.concatenate([scores, np.full((len(ids), 1), 9.0, np.float32)], axis=1)
    padded = evaluate.rerank_select(_t(pad_i), _t(pad_s), CNT, VEC, k, *w, category=CAT, target=TGT, alpha=ALPHA, max_per_category=3)
    _identical(whole, padded, "M = 128 and the same lists inside M = 129")
    for g in (0, 1, 3, 4, 17, 36):
        one = evaluate.rerank_select(IDS[g:g + 1], SC[g:g + 1], CNT[g:g + 1], VEC, k, *w, category=CAT, target=TGT[g:g + 1], alpha=ALPHA,
                                     max_per_category=3)
        _identical(one, tuple(t[g:g + 1] for t in whole), g)


def test_more_workgroups_than_compute_units_and_nobody():
    from digat_amd import evaluate
    M, C, k, d, groups = 16, 17, 10, 20, 1500
    ids, scores, count, category, target, vec = R.make_case("grid", M, C, d, seed=3, groups=groups)
    sim = R.host_gram(ids, vec)                                        # grid vectors: the device's bits
    w = R.WEIGHTS[1]
    got = evaluate.rerank_select(_t(ids), _t(scores), _t(count), _t(vec), k, *w, category=_t(category), target=_t(target), alpha=ALPHA)
    want = evaluate.rerank_select_host(ids, scores, count, sim, k, *w, category=category, target=target, alpha=ALPHA, return_robust=True)
    assert want[4].all(), "grid vectors: numpy certifies these lists alone, and every one is robust"
    R.same(got, want, category, target, ALPHA, "G = 1500")
    nobody = evaluate.rerank_select(_t(ids[:0]), _t(scores[:0]), _t(count[:0]), _t(vec), k, *w, category=_t(category), target=_t(target[:0]))
    assert [tuple(t.shape) for t in nobody] == [(0, k), (0, k), (0,), (0,)] and all(t.is_cuda for t in nobody)


def test_guards():
    from digat_amd import _lib, evaluate
    (ids, scores, count, category, target, vec), (IDS, SC, CNT, CAT, TGT, VEC), _ = _case("grid", 64, 17, 3)
    ok = dict(ids=IDS, scores=SC, count=CNT, vectors=VEC, k=5, w_rel=0.5, w_div=0.3, w_cal=0.2, category=CAT, target=TGT)
    evaluate.rerank_select(**ok)
    wide = torch.zeros((R.NEWS, 513), device=_dev())
    for bad in (dict(k=0), dict(k=129), dict(scores=SC[:, :5]), dict(count=CNT[:2]), dict(w_rel=-0.1), dict(w_div=float("nan")),
                dict(category=None), dict(target=None), dict(target=TGT[:2]), dict(vectors=None), dict(vectors=wide), dict(vectors=VEC[:5]),
                dict(alpha=0.0), dict(max_per_category=-1), dict(ids=IDS.repeat(1, 17), scores=SC.repeat(1, 17))):
        with pytest.raises(ValueError):
            evaluate.rerank_select(**{**ok, **bad})
    evaluate.rerank_select(**{**ok, "vectors": wide, "w_div": 0.0})      # no diversity weight: the vectors only name N
    with pytest.raises(_lib.DigatHipError):
        evaluate.rerank_select(**{**ok, "ids": IDS.cpu()})


# ---------------------------------------------------------------------------------------------------------------------
# recommend(rerank=) end to end
# ---------------------------------------------------------------------------------------------------------------------
def _twin_on(short, vectors, category, target, k, rerank, q=0):
    """The twin on a device shortlist ``(ids, scores, count)`` and the device's own similarities — robust, or the exact comparison
    behind it would prove nothing."""
    from digat_amd import evaluate
    sim = device_gram(short[0], vectors)
    out = evaluate.rerank_select_host(short[0].cpu().numpy(), short[1].cpu().numpy(), short[2].cpu().numpy(), sim, k,
                                      *evaluate.rerank_weights(*rerank), category=category, target=target, alpha=ALPHA, max_per_category=q,
                                      news_num=int(vectors.shape[0]), return_robust=True)
    assert out[4].all(), ("the model's scores meet a near-tie for users", np.flatnonzero(~out[4]).tolist())
    return out[:4]


def test_digat_recommend_with_rerank_end_to_end():
    from digat_amd import evaluate, util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k = np.arange(8), np.arange(1, spec.news_num, dtype=np.int64), 10
    C = int(corpus.news_category.max()) + 1
    target = evaluate.category_share_host(corpus.history[users], corpus.news_category, C)
    unit = util.unit_rows(dc.news_embedding)
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    again = util.recommend(model, dc, users, pool, k, batch_size=256, rerank=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), "rerank=None is the plain call"
    for shortlist, wide, q in ((None, 80, 0), (300, 300, 2)):          # the second: shortlist_segments' long lists
        short = (util.recommend(model, dc, users, pool, wide, batch_size=256) if wide <= 128 else
                 util.recommend_lists(model, dc, users, pool, wide, batch_size=256))
        got = util.recommend(model, dc, users, pool, k, batch_size=256, rerank=(0.2, 0.4), shortlist=shortlist, max_per_category=q)
        assert got[0].is_cuda and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        want = _twin_on(short, unit, corpus.news_category, target, k, (0.2, 0.4), q)
        V.same((got[1], got[0], got[2]), want[:3], ("DIGAT, rerank (0.2, 0.4)", wide))
        assert not torch.equal(got[0], plain[0])
    # long MMR: no calibration weight, a shortlist beyond what diversity= takes
    long = util.recommend_lists(model, dc, users, pool, 300, batch_size=256)
    sim = device_gram(long[0], unit)
    assert evaluate.rerank_weights(0.3, 0.0)[:2] == evaluate.mmr_weights(np.float32(0.7)), "the weights diversity=0.3 hands digat_mmr_select"
    for dv in (0.3, 0.9):
        got = util.recommend(model, dc, users, pool, k, batch_size=256, rerank=(dv, 0.0), shortlist=300)
        want = evaluate.rerank_select_host(long[0].cpu().numpy(), long[1].cpu().numpy(), long[2].cpu().numpy(), sim, k,
                                           *evaluate.rerank_weights(dv, 0.0), news_num=spec.news_num)
        V.same((got[1], got[0], got[2]), want[:3], ("long MMR: 300 entries, where mmr_select stops at 128", dv))
    same = util.recommend(model, dc, users, pool, k, batch_size=256, rerank=(0.0, 0.0))
    V.same((same[1], same[0], same[2]), (plain[1], plain[0], plain[2]), "weights (1, 0, 0): the plain list")


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_rerank_end_to_end(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users, k = np.arange(D.USERS), 5
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    hist = np.where(dev.history_mask.cpu().numpy() != 0, dev.history_ids.cpu().numpy(), 0)
    target = evaluate.category_share_host(hist, category, 5)
    vec = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 16)[0]
    plain = nrms.recommend(m, dev, users, k=k, batch_size=4)
    again = nrms.recommend(m, dev, users, k=k, batch_size=4, rerank=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    wide = nrms.recommend(m, dev, users, k=40, batch_size=4)
    got = nrms.recommend(m, dev, users, k=k, batch_size=4, rerank=(0.2, 0.4), category=category, max_per_category=2)
    V.same((got[1], got[0], got[2]), _twin_on(wide, vec, category, target, k, (0.2, 0.4), 2)[:3], (pre, "rerank (0.2, 0.4)"))
    # a pool of 267 entries (every news three times: equal scores and similarity 1, true ties) and a shortlist of 200
    pool = np.tile(np.arange(1, D.NEWS, dtype=np.int64), 3)
    long = nrms.shortlist(m, dev, users, candidates=pool, m=200, batch_size=4)
    got = nrms.recommend(m, dev, users, candidates=pool, k=k, batch_size=4, rerank=(0.2, 0.4), shortlist=200, category=category)
    V.same((got[1], got[0], got[2]), _twin_on(long, vec, category, target, k, (0.2, 0.4))[:3], (pre, "shortlist 200"))
