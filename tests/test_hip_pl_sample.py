"""GPU suite: the Plackett-Luce slate kernels (``digat_pl_sample``, ``digat_pl_log_prob``) and what stands on them —
``util.sample_lists``, ``util.slate_log_prob``, ``recommend(sample=)`` of both models, ``util.recommend_slates``.  Picks, lengths and
the gathered ids and score bits are held exactly to the host contract (``evaluate.pl_sample_host``) on inputs that
tests/test_pl_sample_cpu.py holds to be robust (same generator, same seeds: tests/pl_sample_common.py); ``logp`` and ``step_logp``
inside ``evaluate.pl_bound``, the worst error-to-bound ratio printed."""
import functools
import types

import numpy as np
import pytest
import torch

import dot_topk_common as D
import pl_sample_common as P

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(-1).view(np.uint8)


def _identical(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and np.array_equal(_bits(x), _bits(y)), what


@functools.lru_cache(maxsize=None)
def _case(M, T):
    """``(seed, scores, count, streams)`` of (M, T), generated once for all the tests that use them."""
    seed = P.seed_of(M, T)
    return (seed,) + P.make_case(seed, M)


@pytest.mark.parametrize("T", P.TS)
@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("M", P.MS)
def test_slates_are_exact_and_probabilities_within_the_bound(M, k, T):
    from digat_amd import evaluate, util
    seed, scores, count, streams = _case(M, T)
    SC, CNT, ST = _t(scores), _t(count), _t(streams)
    rng = np.random.default_rng(M)
    ids = np.stack([rng.permutation(100000)[:M] for _ in range(P.G)]).astype(np.int64)
    for S in P.SS:
        got = evaluate.pl_sample(SC, CNT, k, T, seed=seed, samples=S, streams=ST)
        assert all(t.is_cuda for t in got) and tuple(got[0].shape) == (P.G, S, k)
        want = evaluate.pl_sample_host(scores, count, k, T, seed=seed, samples=S, streams=streams, parts=True)
        ratio = P.same(got, want, want[4], (M, k, S, T))
        print(f"pl_sample M={M} k={k} S={S} T={T}: worst |logp - twin| / bound = {ratio:.4f}")
        assert int(want[1][1]) == 0 and int(want[1][4]) == min(M, 3, k), "an empty list and a short one are among the cases"
        # the ids and the input score bits, gathered through the picks
        out_ids, out_scores, n_out, logp, step = util.sample_lists(_t(ids), SC, CNT, k, T, seed=seed, samples=S, streams=ST)
        hit, g = want[0] >= 0, np.arange(P.G)[:, None, None]
        assert np.array_equal(out_ids.cpu().numpy(), np.where(hit, ids[g, np.maximum(want[0], 0)], -1))
        want_scores = np.where(hit, scores[g, np.maximum(want[0], 0)], -np.inf).astype(np.float32)
        assert np.array_equal(out_scores.cpu().numpy().view(np.uint32), want_scores.view(np.uint32))
        _identical((n_out, logp, step), got[1:], "sample_lists is pl_sample")
    if k == 10 and T == 1.0:                                              # count=None is M, streams=None is the list's index
        got = evaluate.pl_sample(SC, None, k, T, seed=seed)
        want = evaluate.pl_sample_host(scores, None, k, T, seed=seed, parts=True)
        P.same(got, want, want[4], (M, "count None"))


def test_a_spread_above_700_temperatures_sits_on_the_clamp():
    from digat_amd import evaluate
    scores, count, streams, k, T, seed = P.extra_cases()["clamp"]
    got = evaluate.pl_sample(_t(scores), _t(count), k, T, seed=seed, samples=3, streams=_t(streams))
    want = evaluate.pl_sample_host(scores, count, k, T, seed=seed, samples=3, streams=streams, parts=True)
    ratio = P.same(got, want, want[4], "clamp")
    print(f"pl_sample clamp: worst ratio {ratio:.4f}")
    assert (scores.max(axis=1) - scores.min(axis=1) > 700.0 * T).all(), "every list has entries on the clamp"
    assert np.isfinite(got[2].cpu().numpy()).all()


@pytest.mark.parametrize("M,k", [(65, 10), (1024, 128)])
def test_two_calls_a_list_alone_and_a_call_split_by_first_sample_agree_bit_for_bit(M, k):
    from digat_amd import evaluate
    seed, scores, count, streams = _case(M, 1.0)
    SC, CNT, ST = _t(scores), _t(count), _t(streams)
    whole = evaluate.pl_sample(SC, CNT, k, 1.0, seed=seed, samples=3, streams=ST)
    again = evaluate.pl_sample(SC, CNT, k, 1.0, seed=seed, samples=3, streams=ST)
    _identical(whole, again, "two calls")
    for g in (0, 1, 3, 4, 9, 15):
        one = evaluate.pl_sample(SC[g:g + 1], CNT[g:g + 1], k, 1.0, seed=seed, samples=3, streams=ST[g:g + 1])
        _identical(one, tuple(t[g:g + 1] for t in whole), ("alone", g))
    for s in range(3):
        part = evaluate.pl_sample(SC, CNT, k, 1.0, seed=seed, samples=1, first_sample=s, streams=ST)
        _identical((part[0][:, 0], part[1], part[2][:, 0], part[3][:, 0]), (whole[0][:, s], whole[1], whole[2][:, s], whole[3][:, s]),
                   ("first_sample", s))
    other = evaluate.pl_sample(SC, CNT, k, 1.0, seed=seed + 1, samples=3, streams=ST)
    assert not torch.equal(other[0], whole[0]), "another seed: other slates"


@pytest.mark.parametrize("M,k,T", [(65, 10, 1.0), (257, 128, 0.05), (1024, 128, 8.0)])
def test_log_prob_of_the_samplers_picks_is_the_samplers_and_of_a_permuted_slate_the_twins(M, k, T):
    from digat_amd import evaluate
    seed, scores, count, streams = _case(M, T)
    SC, CNT = _t(scores), _t(count)
    picks, n_out, logp, step = evaluate.pl_sample(SC, CNT, k, T, seed=seed, samples=3, streams=_t(streams))
    got = evaluate.pl_log_prob(SC, CNT, picks, T)
    _identical(got, (logp, step), "pl_log_prob on pl_sample's picks")
    _identical(evaluate.pl_log_prob(SC, CNT, picks.to(torch.int64), T), (logp, step), "int64 picks")
    # permuted slates, some cut short by a repeat, a dead position, an entry out of range: the twin
    rng = np.random.default_rng(M + k)
    pk = picks.cpu().numpy().copy()
    for g in range(P.G):
        for s in range(3):
            n = int(n_out[g])
            pk[g, s, :n] = pk[g, s, :n][rng.permutation(n)]
    if k >= 10:
        pk[0, 0, 5] = pk[0, 0, 2]                                          # a repeat
        pk[2, 1, 3] = M                                                    # out of range
        pk[3, 2, 4] = 1 if M >= 8 else -1                                  # list 3, position 1: a NaN
        pk[6, 0, 0] = -1
    got = evaluate.pl_log_prob(SC, CNT, _t(pk), T)
    want = evaluate.pl_log_prob_host(scores, count, pk, T, parts=True)
    ratio = P.within_bound(got[0], got[1], want[0], want[1], want[2], (M, k, T, "permuted"))
    print(f"pl_log_prob M={M} k={k} T={T}: worst ratio {ratio:.4f}")
    if k >= 10:
        assert want[2]["length"][0, 0] == 5 and want[2]["length"][2, 1] == 3 and want[2]["length"][6, 0] == 0
        assert float(got[0][6, 0]) == 0.0 and (got[1][6, 0] == 0).all()


def test_more_workgroups_than_compute_units_and_nobody():
    from digat_amd import evaluate
    scores, count, streams, k, T, seed = P.extra_cases()["many"]
    assert len(scores) == 1100
    got = evaluate.pl_sample(_t(scores), _t(count), k, T, seed=seed, samples=3, streams=_t(streams))
    want = evaluate.pl_sample_host(scores, count, k, T, seed=seed, samples=3, streams=streams, parts=True)
    P.same(got, want, want[4], "G = 1100")
    SC = _t(scores)
    nobody = evaluate.pl_sample(SC[:0], None, k, T, samples=3)
    assert [tuple(t.shape) for t in nobody] == [(0, 3, k), (0,), (0, 3), (0, 3, k)] and all(t.is_cuda for t in nobody)
    nobody = evaluate.pl_log_prob(SC[:0], None, torch.zeros((0, 2, k), dtype=torch.int32, device=_dev()), T)
    assert [tuple(t.shape) for t in nobody] == [(0, 2), (0, 2, k)]


def test_guards_and_every_output_byte():
    from digat_amd import _lib, evaluate
    M, k, T, S, groups = 129, 16, 1.0, 2, 5
    seed, scores, count, streams = _case(M, T)
    scores, count, streams = scores[:groups], count[:groups], streams[:groups]
    SC, CNT, ST = _t(scores), _t(count), _t(streams)
    want = evaluate.pl_sample_host(scores, count, k, T, seed=seed, samples=S, streams=streams, parts=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.pl_sample(SC, CNT, k, T, seed=seed, samples=S, streams=ST)
    side.synchronize()
    P.same(on_side, want, want[4], "side stream")
    # outputs full of garbage with guard regions on both sides: every output byte is written, nothing else is
    L, pad = _lib.lib(), 64
    picks = torch.full((pad + groups * S * k + pad,), 77, dtype=torch.int32, device=_dev())
    n_out = torch.full((pad + groups + pad,), 55, dtype=torch.int32, device=_dev())
    logp = torch.full((pad + groups * S + pad,), 9.0, dtype=torch.float64, device=_dev())
    step = torch.full((pad + groups * S * k + pad,), 123.0, dtype=torch.float32, device=_dev())
    inputs = [t.clone() for t in (SC, CNT, ST)]
    inv_t = 1.0 / T
    _lib.check(L.digat_pl_sample(SC.data_ptr(), CNT.data_ptr(), groups, M, k, inv_t, seed, S, 0, ST.data_ptr(), picks[pad:].data_ptr(),
                                 n_out[pad:].data_ptr(), logp[pad:].data_ptr(), step[pad:].data_ptr(), None, 0, _lib.stream_ptr()),
               "digat_pl_sample")
    torch.cuda.synchronize()
    for buf, fill, n in ((picks, 77, groups * S * k), (n_out, 55, groups), (logp, 9.0, groups * S), (step, 123.0, groups * S * k)):
        assert (buf[:pad] == fill).all() and (buf[pad + n:] == fill).all()
    raw = (picks[pad:pad + groups * S * k].view(groups, S, k), n_out[pad:pad + groups], logp[pad:pad + groups * S].view(groups, S),
           step[pad:pad + groups * S * k].view(groups, S, k))
    P.same(raw, want, want[4], "raw call")
    logp2 = torch.full((pad + groups * S + pad,), 9.0, dtype=torch.float64, device=_dev())
    step2 = torch.full((pad + groups * S * k + pad,), 123.0, dtype=torch.float32, device=_dev())
    _lib.check(L.digat_pl_log_prob(SC.data_ptr(), CNT.data_ptr(), groups, M, k, inv_t, S, raw[0].contiguous().data_ptr(), logp2[pad:].data_ptr(),
                                   step2[pad:].data_ptr(), None, 0, _lib.stream_ptr()), "digat_pl_log_prob")
    torch.cuda.synchronize()
    assert (logp2[:pad] == 9.0).all() and (logp2[pad + groups * S:] == 9.0).all()
    assert (step2[:pad] == 123.0).all() and (step2[pad + groups * S * k:] == 123.0).all()
    _identical((logp2[pad:pad + groups * S], step2[pad:pad + groups * S * k]), (raw[2].reshape(-1), raw[3].reshape(-1)), "raw log_prob")
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (SC, CNT, ST))), "inputs are read only"
    # refusals of the Python entries
    with pytest.raises(ValueError, match="k must be"):
        evaluate.pl_sample(SC, CNT, 129, T)
    with pytest.raises(ValueError, match="temperature must be"):
        evaluate.pl_sample(SC, CNT, k, 0.0)
    with pytest.raises(ValueError, match="PL_MAX_SAMPLE"):
        evaluate.pl_sample(SC, CNT, k, T, samples=2, first_sample=(1 << 22) - 1)
    with pytest.raises(ValueError, match="streams must have"):
        evaluate.pl_sample(SC, CNT, k, T, streams=ST[:2])
    with pytest.raises(ValueError, match="picks must be"):
        evaluate.pl_log_prob(SC, CNT, raw[0][:2], T)
    with pytest.raises(ValueError, match="integer positions"):
        evaluate.pl_log_prob(SC, CNT, raw[3], T)
    with pytest.raises(_lib.DigatHipError):
        evaluate.pl_sample(SC.cpu(), CNT.cpu(), k, T)


# ---------------------------------------------------------------------------------------------------------------------
# recommend(sample=) end to end
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


def _well_separated(wide_lists, k, T):
    """Users whose k best shortlist scores and the best score behind them are each further apart than the Gumbel noise can bridge at
    temperature T: the largest key noise of a word is -log(-log(1 - 2^-33)) < 23 and the smallest above -3.2."""
    ids, scores, count = (t.cpu().numpy() for t in wide_lists)
    ok = np.zeros(len(count), dtype=bool)
    for g in range(len(count)):
        s = scores[g, :min(int(count[g]), k + 1)].astype(np.float64)
        ok[g] = len(s) >= 2 and bool(np.all(s[:-1] - s[1:] > 27.0 * T))
    return ok


def _check_sampled(recommend, wide_lists, plain, k, users, what):
    """``recommend(sample=T, seed=, ...)`` against ``sample_lists`` on the shortlist of the same call; the cold limit; the off switch."""
    from digat_amd import util
    streams = torch.as_tensor(np.asarray(users))
    for T, seed in ((0.5, 0), (2.0, 7)):
        got = recommend(sample=T, seed=seed)
        assert got[0].is_cuda and got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        assert tuple(got[0].shape) == (len(users), k)
        want = util.sample_lists(*wide_lists, k, T, seed=seed, streams=streams)
        _identical(got, (want[0][:, 0].contiguous(), want[1][:, 0].contiguous(), want[2]), (what, T, "sample_lists on the shortlist"))
        gi, wi, wc = got[0].cpu().numpy(), wide_lists[0].cpu().numpy(), wide_lists[2].cpu().numpy()
        for g in range(len(users)):
            mine = gi[g][gi[g] >= 0]
            assert len(set(mine.tolist())) == len(mine) and set(mine.tolist()) <= set(wi[g, :wc[g]].tolist()), (what, g, "a subset of the shortlist")
    # the same user alone: the same slate (the default streams are the impression indices)
    one = recommend(sample=0.5, seed=0, users=users[2:3])
    full = recommend(sample=0.5, seed=0)
    _identical(one, tuple(t[2:3] for t in full), (what, "a user alone"))
    # cold: the plain list, where the scores are far enough apart for it to be certain
    cold = recommend(sample=1e-4, seed=3)
    sure = _well_separated(wide_lists, k, 1e-4)
    print(f"{what}: {int(sure.sum())} of {len(sure)} users have lists separated by more than 27e-4")
    assert sure.any(), "no user's scores are distinct enough for the cold limit to be certain"
    rows = torch.from_numpy(np.flatnonzero(sure)).to(_dev())
    _identical(tuple(t[rows] for t in cold), tuple(t[rows] for t in plain), (what, "T = 1e-4 is the plain list"))
    _identical(recommend(sample=None), plain, (what, "sample=None"))


def test_digat_recommend_with_sampling_end_to_end():
    from digat_amd import util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k = np.arange(3, 11), np.arange(1, spec.news_num, dtype=np.int64), 10
    plain = util.recommend(model, dc, users, pool, k, batch_size=256)
    wide = util.recommend(model, dc, users, pool, 80, batch_size=256)
    recommend = lambda users=users, **kw: util.recommend(model, dc, users, pool, k, batch_size=256, **kw)
    _check_sampled(recommend, wide, plain, k, users, "DIGAT")
    # a long shortlist: shortlist_segments' lists
    long = util.recommend_lists(model, dc, users, pool, 200, batch_size=256)
    got = util.recommend(model, dc, users, pool, k, batch_size=256, sample=1.0, seed=2, shortlist=200)
    want = util.sample_lists(*long, k, 1.0, seed=2, streams=torch.as_tensor(users))
    _identical(got, (want[0][:, 0].contiguous(), want[1][:, 0].contiguous(), want[2]), "shortlist 200")
    # --recommend_sample: the lines of main.recommend_lines are these slates, for every impression of the corpus
    from digat_amd import main
    everybody = np.arange(spec.impressions)
    lines = main.recommend_lines(model, dc, k, 256, sample=0.5, seed=4)
    ids, _, count = util.recommend(model, dc, everybody, pool, k, batch_size=256, sample=0.5, seed=4)
    ids, count = ids.cpu().numpy(), count.cpu().numpy()
    assert lines == ['%d [%s]' % (i + 1, ','.join(str(int(v)) for v in ids[i, :count[i]])) for i in range(spec.impressions)]
    assert lines != main.recommend_lines(model, dc, k, 256)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_sampling_end_to_end(pre):
    from digat_amd import nrms
    m, dev = D.model(pre, _dev()), D.dev_set(_dev())
    users, k = np.arange(D.USERS), 5
    plain = nrms.recommend(m, dev, users, k=k, batch_size=4)
    wide = nrms.recommend(m, dev, users, k=40, batch_size=4)
    recommend = lambda users=users, **kw: nrms.recommend(m, dev, users, k=k, batch_size=4, **kw)
    _check_sampled(recommend, wide, plain, k, users, pre)


def test_recommend_slates_and_the_log_prob_of_its_own_slates():
    from digat_amd import evaluate, util
    spec, corpus, _ = _corpus()
    model, dc = _model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k, T = np.arange(12), np.arange(1, spec.news_num, dtype=np.int64), 3, 0.7
    log = util.recommend_slates(model, dc, users, pool, k, T, samples=4, seed=5, batch_size=256)
    assert tuple(log["slates"].shape) == (12, 4, 3) and tuple(log["ids"].shape) == (12, 24) and log["logp"].dtype == torch.float64
    short = util.recommend(model, dc, users, pool, 24, batch_size=256)
    _identical((log["ids"], log["scores"], log["count"]), short, "the shortlist is the plain call's")
    logp, step, covered = util.slate_log_prob(log["ids"], log["scores"], log["count"], log["slates"], T)
    assert bool(covered.all())
    _identical((logp, step), (log["logp"], log["step_logp"]), "slate_log_prob of its own slates")
    # the model's scores of its own shortlist in place are recommend's bits: the propensity can be rebuilt from the ids alone
    again = util.score_lists(model, dc, users, log["ids"], log["count"], batch_size=256)
    _identical(util.slate_log_prob(log["ids"], again, log["count"], log["slates"], T)[:2], (log["logp"], log["step_logp"]), "score_lists")
    # sample 0 of the log is the list recommend(sample=) serves
    served = util.recommend(model, dc, users, pool, k, batch_size=256, sample=T, seed=5)
    _identical(served[:2], (log["slates"][:, 0].contiguous(), log["slate_scores"][:, 0].contiguous()), "recommend(sample=)")
    # a hotter target policy on the same log: weights that average to about one
    lt, _, cov = util.slate_log_prob(log["ids"], log["scores"], log["count"], log["slates"], 2 * T)
    out = evaluate.off_policy_value(np.ones(48), lt.cpu().numpy().reshape(-1), log["logp"].cpu().numpy().reshape(-1),
                                    units=np.arange(0, 49, 4), replicates=200)
    assert bool(cov.all()) and abs(out["snips"]["value"] - 1.0) < 1e-12 and 1.0 <= out["ess"] <= 48.0
