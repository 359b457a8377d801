"""GPU suite: the calibrated re-rank kernel (``digat_calibrated_select``) and ``recommend(calibration=)`` on it.  The selection is
held exactly — ids, score bits, counts, fills — to the host contract (``evaluate.calibrated_select_host``) on inputs that
tests/test_calibrate_cpu.py holds to be robust (same generator, same seeds: tests/calibrate_common.py), the ``kl`` output inside the
rounding of one float32 conversion and a float64 sum in any order."""
import functools
import types

import numpy as np
import pytest
import torch

import calibrate_common as K
import diversify_common as V
import dot_topk_common as D

pytestmark = pytest.mark.gpu

ALPHA = 0.01


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


@pytest.mark.parametrize("lam", K.LAMS)
@pytest.mark.parametrize("M,C,k", K.SHAPES)
def test_selection_is_exact_against_the_twin(M, C, k, lam):
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(K.seed_of(M, C, k, lam), M, C)
    got = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(target), k, lam, ALPHA)
    assert all(t.is_cuda for t in got)
    want = evaluate.calibrated_select_host(ids, scores, count, category, target, k, lam, ALPHA)
    K.same(got, want, category, target, ALPHA, (M, C, k, lam))
    assert int(want[2][1]) == 0, "an empty list is among the cases"
    if lam == K.LAMS[0]:                                                  # count=None is M
        got = evaluate.calibrated_select(_t(ids), _t(scores), None, _t(category), _t(target), min(k, 10), lam, ALPHA)
        K.same(got, evaluate.calibrated_select_host(ids, scores, None, category, target, min(k, 10), lam, ALPHA), category, target, ALPHA,
               "count None")


@pytest.mark.parametrize("M,k,seed", K.GRID_CASES)
def test_uniform_target_with_scores_on_a_grid(M, k, seed):
    """Target 1/16 everywhere, scores multiples of 1/16: dozens of exact ties per step, every one of them a true tie."""
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(seed, M, 16, grid=True, uniform=True)
    assert len(np.unique(scores[np.isfinite(scores)])) < 200
    got = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(target), k, 0.5, ALPHA)
    K.same(got, evaluate.calibrated_select_host(ids, scores, count, category, target, k, 0.5, ALPHA), category, target, ALPHA, (M, k))


@pytest.mark.parametrize("M,k", [(100, 100), (1000, 128)])
def test_lam_one_is_the_shortlist_of_the_same_lists(M, k):
    """``lam = 1``: ``value = s`` exactly — ``evaluate.shortlist_segments`` over the lists' elements, on the device, bit for bit;
    scores on a grid, so ties by position are met."""
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    ids, count = V.make_lists(rng, K.G, M, K.NEWS, invalid=False)
    scores = (np.round(rng.standard_normal((K.G, M)) * 4) / 4).astype(np.float32)
    category = rng.integers(0, 17, size=K.NEWS).astype(np.int32)
    target = rng.dirichlet(np.ones(17), size=K.G).astype(np.float32)
    got = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(target), k, 1.0, ALPHA)
    flat_s = np.concatenate([scores[g, :count[g]] for g in range(K.G)])
    flat_i = np.concatenate([ids[g, :count[g]] for g in range(K.G)])
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    want = evaluate.shortlist_segments(_t(flat_s), _t(start), k, ids=_t(flat_i))
    V.same(got[:3], want, (M, k))
    zero = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(np.zeros_like(target)), k, 0.3, ALPHA)
    V.same(zero[:3], want, "an all-zero target is the plain top-k")
    assert (zero[3] == 0).all()


@pytest.mark.parametrize("M,C,k", [(128, 64, 128), (1024, 17, 128)])
def test_two_calls_agree_and_a_list_does_not_depend_on_its_batch(M, C, k):
    from digat_amd import evaluate
    ids, scores, count, category, target = K.make_case(K.seed_of(M, C, k, 0.5), M, C)
    CAT = _t(category)
    whole = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), CAT, _t(target), k, 0.5, ALPHA)
    again = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), CAT, _t(target), k, 0.5, ALPHA)
    _identical(whole, again, "two calls")
    for g in (0, 1, 3, 4, 17, 36):
        one = evaluate.calibrated_select(_t(ids[g:g + 1]), _t(scores[g:g + 1]), _t(count[g:g + 1]), CAT, _t(target[g:g + 1]), k, 0.5, ALPHA)
        _identical(one, tuple(t[g:g + 1] for t in whole), g)


def test_more_workgroups_than_compute_units_and_nobody():
    from digat_amd import evaluate
    M, C, k, groups = 16, 17, 10, 600
    ids, scores, count, category, target = K.make_case(3, M, C, groups=groups)
    got = evaluate.calibrated_select(_t(ids), _t(scores), _t(count), _t(category), _t(target), k, 0.5, ALPHA)
    K.same(got, evaluate.calibrated_select_host(ids, scores, count, category, target, k, 0.5, ALPHA), category, target, ALPHA, "G = 600")
    nobody = evaluate.calibrated_select(_t(ids[:0]), _t(scores[:0]), _t(count[:0]), _t(category), _t(target[:0]), k, 0.5, ALPHA)
    assert [tuple(t.shape) for t in nobody] == [(0, k), (0, k), (0,), (0,)] and all(t.is_cuda for t in nobody)


def test_guards():
    from digat_amd import _lib, evaluate
    M, C, k, groups = 129, 17, 16, 5
    ids, scores, count, category, target = K.make_case(K.seed_of(M, C, k, 0.3), M, C)
    ids, scores, count, target = ids[:groups], scores[:groups], count[:groups], target[:groups]
    IDS, SC, CNT, CAT, TGT = _t(ids), _t(scores), _t(count), _t(category), _t(target)
    want = evaluate.calibrated_select_host(ids, scores, count, category, target, k, 0.3, ALPHA)
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.calibrated_select(IDS, SC, CNT, CAT, TGT, k, 0.3, ALPHA)
    side.synchronize()
    K.same(on_side, want, category, target, ALPHA, "side stream")
    # outputs full of garbage, guard regions on both sides of each: every output byte is written, nothing else is
    L = _lib.lib()
    assert L.digat_calibrated_select_workspace_bytes(groups, M, C, k) == 0
    pad = 64
    out_s = torch.full((pad + groups * k + pad,), 123.0, dtype=torch.float32, device=_dev())
    out_i = torch.full((pad + groups * k + pad,), 77, dtype=torch.int64, device=_dev())
    out_c = torch.full((pad + groups + pad,), 55, dtype=torch.int32, device=_dev())
    out_kl = torch.full((pad + groups + pad,), 9.0, dtype=torch.float32, device=_dev())
    inputs = [t.clone() for t in (IDS, SC, CNT, CAT, TGT)]
    lam, mu = evaluate.mmr_weights(0.3)
    _lib.check(L.digat_calibrated_select(IDS.data_ptr(), SC.data_ptr(), CNT.data_ptr(), groups, M, CAT.data_ptr(), K.NEWS, TGT.data_ptr(), C,
                                         float(lam), float(mu), ALPHA, k, out_i[pad:].data_ptr(), out_s[pad:].data_ptr(),
                                         out_c[pad:].data_ptr(), out_kl[pad:].data_ptr(), None, 0, _lib.stream_ptr()),
               "digat_calibrated_select")
    torch.cuda.synchronize()
    assert (out_s[:pad] == 123.0).all() and (out_s[pad + groups * k:] == 123.0).all()
    assert (out_i[:pad] == 77).all() and (out_i[pad + groups * k:] == 77).all()
    assert (out_c[:pad] == 55).all() and (out_c[pad + groups:] == 55).all()
    assert (out_kl[:pad] == 9.0).all() and (out_kl[pad + groups:] == 9.0).all()
    raw = (out_s[pad:pad + groups * k].view(groups, k), out_i[pad:pad + groups * k].view(groups, k), out_c[pad:pad + groups],
           out_kl[pad:pad + groups])
    K.same(raw, want, category, target, ALPHA, "raw call")
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (IDS, SC, CNT, CAT, TGT))), "inputs are read only"
    # refusals of the Python entry
    with pytest.raises(ValueError, match="k must be"):
        evaluate.calibrated_select(IDS, SC, CNT, CAT, TGT, 129, 0.3)
    with pytest.raises(ValueError, match="lam must"):
        evaluate.calibrated_select(IDS, SC, CNT, CAT, TGT, k, 1.2)
    with pytest.raises(ValueError, match="alpha must"):
        evaluate.calibrated_select(IDS, SC, CNT, CAT, TGT, k, 0.3, alpha=1.0)
    with pytest.raises(ValueError, match=r"\[G, M\]"):
        evaluate.calibrated_select(IDS, SC[:, :5], CNT, CAT, TGT, k, 0.3)
    with pytest.raises(ValueError, match="target must be"):
        evaluate.calibrated_select(IDS, SC, CNT, CAT, TGT[:2], k, 0.3)
    with pytest.raises(_lib.DigatHipError):
        evaluate.calibrated_select(IDS.cpu(), SC.cpu(), CNT.cpu(), CAT.cpu(), TGT.cpu(), k, 0.3)


# ---------------------------------------------------------------------------------------------------------------------
# recommend(calibration=) end to end
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


def _twin_on(short, category, target, k, lam):
    """The twin on a device shortlist ``(ids, scores, count)`` — robust, or the exact comparison behind it would prove nothing."""
    from digat_amd import evaluate
    s, i, c, kl, robust = evaluate.calibrated_select_host(short[0].cpu().numpy(), short[1].cpu().numpy(), short[2].cpu().numpy(), category,
                                                          target, k, lam, ALPHA, return_robust=True)
    assert robust.all(), ("the model's scores meet a near-tie for users", np.flatnonzero(~robust).tolist())
    return s, i, c, kl


def test_digat_recommend_with_calibration_end_to_end():
    from digat_amd import evaluate, util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k = np.arange(8), np.arange(1, spec.news_num, dtype=np.int64), 10
    C = int(corpus.news_category.max()) + 1
    target = evaluate.category_share_host(corpus.history[users], corpus.news_category, C)
    assert np.array_equal(evaluate.category_share(dc.history[:8], dc.news_category, C).cpu().numpy(), target)
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    again = util.recommend(model, dc, users, pool, k, batch_size=256, calibration=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    for shortlist, wide in ((None, 80), (200, 200)):                   # the second: shortlist_segments' long lists
        short = (util.recommend(model, dc, users, pool, wide, batch_size=256) if wide <= 128 else
                 util.recommend_lists(model, dc, users, pool, wide, batch_size=256))
        got = util.recommend(model, dc, users, pool, k, batch_size=256, calibration=0.5, shortlist=shortlist)
        assert got[0].is_cuda and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        want = _twin_on(short, corpus.news_category, target, k, 0.5)
        V.same((got[1], got[0], got[2]), want[:3], ("DIGAT, calibration 0.5", wide))
        same = util.recommend(model, dc, users, pool, k, batch_size=256, calibration=0.0, shortlist=shortlist)
        V.same((same[1], same[0], same[2]), (plain[1], plain[0], plain[2]), "lam = 1: the plain list")
    # a given target in place of the histories'
    given = np.full((len(users), C), 1.0 / C, dtype=np.float32)
    got = util.recommend(model, dc, users, pool, k, batch_size=256, calibration=0.5, calibration_target=given)
    short = util.recommend(model, dc, users, pool, 80, batch_size=256)
    V.same((got[1], got[0], got[2]), _twin_on(short, corpus.news_category, given, k, 0.5)[:3], "calibration_target")


def test_full_calibration_does_not_raise_the_divergence():
    """``calibration = 1``: every pick is the one that lowers the divergence most; the list's ``calibration_kl`` is not above the
    plain top-k's for any user with a full shortlist and a target that names a category."""
    from digat_amd import evaluate, util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k = np.arange(24), np.arange(1, spec.news_num, dtype=np.int64), 10
    C = int(corpus.news_category.max()) + 1
    target = evaluate.category_share(dc.history[:24], dc.news_category, C)
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    full = util.recommend(model, dc, users, pool, k, batch_size=256, calibration=1.0)
    kl_plain = util.calibration_kl(plain[0], plain[2], dc.news_category, target, ALPHA).cpu().numpy()
    kl_full = util.calibration_kl(full[0], full[2], dc.news_category, target, ALPHA).cpu().numpy()
    matter = (plain[2].cpu().numpy() == k) & (target.sum(dim=1).cpu().numpy() > 0)
    assert matter.sum() >= 12
    assert (kl_full[matter] <= kl_plain[matter]).all(), (kl_full[matter].tolist(), kl_plain[matter].tolist())
    assert (kl_full[matter] < kl_plain[matter]).any(), "and lowers it for somebody"
    # calibration_kl of a list is the kl its own re-rank reports
    short = util.recommend(model, dc, users, pool, 80, batch_size=256)
    _, _, _, kl = util.calibrate(*short, dc.news_category, target, k, 0.0, ALPHA)
    assert np.array_equal(kl.cpu().numpy().view(np.uint32), kl_full.view(np.uint32))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_calibration_end_to_end(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users, k = np.arange(D.USERS), 5
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    hist = np.where(dev.history_mask.cpu().numpy() != 0, dev.history_ids.cpu().numpy(), 0)
    target = evaluate.category_share_host(hist, category, 5)
    plain = nrms.recommend(m, dev, users, k=k, batch_size=4)
    wide = nrms.recommend(m, dev, users, k=40, batch_size=4)
    got = nrms.recommend(m, dev, users, k=k, batch_size=4, calibration=0.5, category=category)
    V.same((got[1], got[0], got[2]), _twin_on(wide, category, target, k, 0.5)[:3], (pre, "calibration 0.5"))
    same = nrms.recommend(m, dev, users, k=k, batch_size=4, calibration=0.0, category=category)
    V.same((same[1], same[0], same[2]), (plain[1], plain[0], plain[2]), "lam = 1")
    # a pool of 267 entries (every news three times: equal scores, true ties) and a shortlist of 200: the long-list kernels
    pool = np.tile(np.arange(1, D.NEWS, dtype=np.int64), 3)
    long = nrms.shortlist(m, dev, users, candidates=pool, m=200, batch_size=4)
    got = nrms.recommend(m, dev, users, candidates=pool, k=k, batch_size=4, calibration=0.5, shortlist=200, category=category)
    V.same((got[1], got[0], got[2]), _twin_on(long, category, target, k, 0.5)[:3], (pre, "shortlist 200"))
