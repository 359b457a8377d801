"""CPU suite: the numpy contract of the Plackett-Luce sampler (``evaluate.pl_draws_host``, ``pl_sample_host``, ``pl_log_prob_host``,
``pl_bound``), ``evaluate.off_policy_value``, the CPU road of ``util.sample_lists`` / ``slate_log_prob``, the refusals of
``recommend(sample=)`` and the flags, ``synthetic.planted_match`` — and that every input the GPU suite draws is robust, so that
tests/test_hip_pl_sample.py may compare picks exactly (same generator, same seeds: tests/pl_sample_common.py)."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

import pl_sample_common as P


# ---------------------------------------------------------------------------------------------------------------------
# the draws
# ---------------------------------------------------------------------------------------------------------------------
def test_draws_split_by_first_sample_and_by_batch_and_a_slate_has_distinct_words():
    from digat_amd import evaluate
    streams = np.array([0, 7, (1 << 32) - 1, 123456789, 7], dtype=np.int64)
    whole = evaluate.pl_draws_host(streams, 5, 1024, seed=11)
    assert whole.dtype == np.uint32 and whole.shape == (5, 5, 1024)
    for s in range(5):
        assert np.array_equal(evaluate.pl_draws_host(streams, 1, 1024, seed=11, first_sample=s)[:, 0], whole[:, s])
    assert np.array_equal(evaluate.pl_draws_host(streams, 2, 1024, seed=11, first_sample=3), whole[:, 3:])
    for g in range(5):
        assert np.array_equal(evaluate.pl_draws_host(streams[g:g + 1], 5, 1024, seed=11)[0], whole[g])
    assert np.array_equal(whole[1], whole[4]), "the same stream: the same words"
    assert np.array_equal(evaluate.pl_draws_host(streams, 5, 70, seed=11), whole[:, :, :70]), "a word does not depend on M"
    for g in range(4):
        for s in range(5):
            assert len(np.unique(whole[g, s])) == 1024
    assert not np.array_equal(evaluate.pl_draws_host(streams, 5, 1024, seed=12), whole)
    # the construction, written out for one word
    h = lambda x: int(evaluate._hash32(np.array([x], dtype=np.uint64))[0])
    g, s, p = 3, 4, 1000
    want = h((((s << 10 | p) * 0x9E3779B9) & 0xFFFFFFFF) + h(11 + int(streams[g])))
    assert int(whole[g, s, p]) == want
    # uniform enough: the mean of 25 600 words
    assert abs(float(whole.astype(np.float64).mean()) / 2.0 ** 32 - 0.5) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# the probabilities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0.5, 1.0, 8.0])
def test_probabilities_of_all_orderings_sum_to_one(T):
    from digat_amd import evaluate
    scores = np.array([[0.3, -1.2, 2.0, 0.7]], dtype=np.float32)
    for k, n in ((4, 24), (2, 12)):
        slates = np.array(list(itertools.permutations(range(4), k)), dtype=np.int32)[None, :, :]
        assert slates.shape == (1, n, k)
        logp, step = evaluate.pl_log_prob_host(scores, None, slates, T)
        assert abs(float(np.exp(logp).sum()) - 1.0) < 1e-12, (k, float(np.exp(logp).sum()))
        assert np.allclose(step.astype(np.float64).sum(axis=2), logp, rtol=0, atol=1e-6)
    # against the formula, plain Python
    a = [float(x) / T for x in scores[0]]
    p = math.exp(a[2]) / sum(math.exp(x) for x in a) * math.exp(a[0]) / sum(math.exp(a[i]) for i in (0, 1, 3))
    got = float(evaluate.pl_log_prob_host(scores, None, np.array([[[2, 0]]]), T)[0][0, 0])
    assert abs(math.exp(got) - p) < 1e-14


def test_a_slate_ends_at_its_first_bad_entry_and_dead_positions_carry_no_mass():
    from digat_amd import evaluate
    scores = np.array([[1.0, np.nan, 0.5, np.inf, -np.inf, 0.25, 9.0]], dtype=np.float32)
    count = np.array([6])                                            # position 6 lies beyond the count
    full = evaluate.pl_log_prob_host(scores, count, np.array([[[0, 2, 5]]]), 1.0, parts=True)
    assert full[2]["length"][0, 0] == 3 and full[2]["live"][0] == 3
    assert abs(float(full[0][0, 0]) - math.log(math.exp(1.0) / (math.exp(1.0) + math.exp(0.5) + math.exp(0.25))
                                               * math.exp(0.5) / (math.exp(0.5) + math.exp(0.25)))) < 1e-14
    for bad, length in (([0, 1, 2], 1), ([0, 3, 2], 1), ([0, 4, 2], 1), ([0, 6, 2], 1), ([0, -1, 2], 1), ([0, 7, 2], 1), ([0, 2, 0], 2),
                        ([-1, 0, 2], 0)):
        logp, step, parts = evaluate.pl_log_prob_host(scores, count, np.array([[bad]]), 1.0, parts=True)
        assert parts["length"][0, 0] == length, bad
        assert (step[0, 0, length:] == 0).all() and np.array_equal(step[0, 0, :length], full[1][0, 0, :length]), bad
    empty = evaluate.pl_log_prob_host(scores, np.array([0]), np.array([[[0, 2, 5]]]), 1.0)
    assert float(empty[0][0, 0]) == 0.0 and (empty[1] == 0).all()


def test_slate_frequencies_match_the_plackett_luce_probabilities():
    from digat_amd import evaluate
    n = 20000
    row = np.array([0.3, -1.2, 2.0, 0.7], dtype=np.float32)
    scores = np.tile(row, (n, 1))
    picks, n_out, logp, step = evaluate.pl_sample_host(scores, None, 2, 1.5, seed=3)
    assert (n_out == 2).all() and picks.shape == (n, 1, 2)
    slates = np.array(list(itertools.permutations(range(4), 2)), dtype=np.int32)
    prob = np.exp(evaluate.pl_log_prob_host(row[None, :], None, slates[None, :, :], 1.5)[0][0])
    seen = 0
    for (i, j), p in zip(slates, prob):
        hits = (picks[:, 0, 0] == i) & (picks[:, 0, 1] == j)
        freq = float(hits.mean())
        assert abs(freq - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), ((i, j), freq, p)
        assert np.allclose(np.exp(logp[hits, 0]), p, rtol=1e-12), "a slate's logp is that slate's probability"
        seen += int(hits.sum())
    assert seen == n
    # samples of one list are streams of another call: (stream g, sample 0) of n lists is not (stream 0, sample s) — but both are draws
    many = evaluate.pl_sample_host(row[None, :], None, 2, 1.5, seed=3, samples=4096)[0][0]
    first = np.array([(many[:, 0] == i).mean() for i in range(4)])
    want = np.exp(row.astype(np.float64) / 1.5) / np.exp(row.astype(np.float64) / 1.5).sum()
    assert (np.abs(first - want) <= 5.0 * np.sqrt(want * (1 - want) / 4096)).all()


def test_a_cold_temperature_gives_the_top_k_order():
    from digat_amd import evaluate
    rng = np.random.default_rng(0)
    G, M, k = 6, 50, 10
    scores = np.stack([rng.permutation(M) * 0.1 for _ in range(G)]).astype(np.float32)
    count = np.array([50, 50, 7, 0, 50, 31], dtype=np.int32)
    picks, n_out, logp, step = evaluate.pl_sample_host(scores, count, k, 1e-3, seed=5, samples=2)
    flat = np.concatenate([scores[g, :count[g]] for g in range(G)])
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    _, ids, cnt = evaluate.topk_segments_host(flat, start, k)
    for g in range(G):
        assert n_out[g] == cnt[g]
        for s in range(2):
            assert np.array_equal(picks[g, s, :cnt[g]], ids[g, :cnt[g]]) and (picks[g, s, cnt[g]:] == -1).all()
    # adjacent scores are 100 apart in a: the first seven steps are all but certain; from the eighth on every entry left lies 700
    # below a_max, on the clamp, and the reported step is the uniform one over what is left (the contract's stated limit)
    assert (np.abs(step[0, :, :7]) < 1e-30).all()
    assert abs(float(step[0, 0, 8]) + math.log(42.0)) < 1e-6


def test_split_by_first_sample_and_by_batch_and_the_log_prob_of_its_own_picks():
    from digat_amd import evaluate
    scores, count, streams = P.make_case(1, 65)
    whole = evaluate.pl_sample_host(scores, count, 10, 1.0, seed=9, samples=3, streams=streams)
    for s in range(3):
        one = evaluate.pl_sample_host(scores, count, 10, 1.0, seed=9, samples=1, first_sample=s, streams=streams)
        assert np.array_equal(one[0][:, 0], whole[0][:, s]) and np.array_equal(one[2][:, 0].view(np.uint64), whole[2][:, s].view(np.uint64))
    for g in (0, 3, 9):
        one = evaluate.pl_sample_host(scores[g:g + 1], count[g:g + 1], 10, 1.0, seed=9, samples=3, streams=streams[g:g + 1])
        assert np.array_equal(one[0][0], whole[0][g]) and np.array_equal(one[3][0].view(np.uint32), whole[3][g].view(np.uint32))
    logp, step = evaluate.pl_log_prob_host(scores, count, whole[0], 1.0)
    assert np.array_equal(logp.view(np.uint64), whole[2].view(np.uint64)) and np.array_equal(step.view(np.uint32), whole[3].view(np.uint32))
    assert whole[1][1] == 0 and (whole[0][1] == -1).all() and (whole[2][1] == 0).all(), "an empty list"
    assert whole[1][4] == 3 and (whole[0][4, :, 3:] == -1).all(), "fewer live entries than k"
    live3 = set(np.flatnonzero(np.isfinite(scores[3])).tolist())
    assert set(whole[0][3].reshape(-1).tolist()) <= live3, "NaN and the infinities are never drawn"
    default = evaluate.pl_sample_host(scores, count, 10, 1.0, seed=9)
    named = evaluate.pl_sample_host(scores, count, 10, 1.0, seed=9, streams=np.arange(len(scores)))
    assert np.array_equal(default[0], named[0]), "the default stream is the list's index"


def test_the_clamp_keeps_every_step_finite():
    from digat_amd import evaluate
    scores = np.array([[0.0, -1000.0, -2000.0, -1e30]], dtype=np.float32)
    logp, step, parts = evaluate.pl_log_prob_host(scores, None, np.array([[[3, 2, 1, 0]]]), 1.0, parts=True)
    assert np.isfinite(logp).all() and np.isfinite(step).all()
    assert abs(float(parts["step"][0, 0, 0]) + 700.0) < 1e-9 and float(parts["step"][0, 0, 3]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# robustness
# ---------------------------------------------------------------------------------------------------------------------
def test_a_near_tie_is_not_robust(monkeypatch):
    from digat_amd import evaluate
    scores = np.array([[1.0, 1.0, -3.0], [1.0, 0.5, -3.0]], dtype=np.float32)
    assert evaluate.pl_sample_host(scores, None, 2, 1.0, return_robust=True)[4].all()
    real = evaluate.pl_draws_host

    def forced(streams, samples, M, seed=0, first_sample=0):
        w = real(streams, samples, M, seed, first_sample)
        w[0, 0, 1] = w[0, 0, 0]                                      # list 0: two equal scores behind one word: equal keys
        return w
    monkeypatch.setattr(evaluate, "pl_draws_host", forced)
    picks, _, _, _, robust = evaluate.pl_sample_host(scores, None, 2, 1.0, return_robust=True)
    assert robust.tolist() == [False, True]
    assert picks[0, 0].tolist() in ([0, 1], [2, 0]), "equal keys: the lower position first"
    if picks[0, 0, 0] == 2:
        assert picks[0, 0, 1] == 0
    # a pair that only matters below the cut does not count: k = 1 looks at the top two keys
    third = evaluate.pl_sample_host(np.array([[9.0, 1.0, 1.0]], dtype=np.float32), None, 1, 0.01, return_robust=True)
    assert third[4].all()


@pytest.mark.parametrize("M", P.MS)
def test_every_input_of_the_gpu_suite_is_robust(M):
    from digat_amd import evaluate
    for T in P.TS:
        seed = P.seed_of(M, T)
        scores, count, streams = P.make_case(seed, M)
        out = evaluate.pl_sample_host(scores, count, 128, T, seed=seed, samples=3, streams=streams, return_robust=True)
        assert out[4].all(), (M, T, np.flatnonzero(~out[4]).tolist())
        assert out[1][1] == 0 and out[1][8] == 0 and out[1][7] == 0 and out[1][4] == min(M, 3)
        if T == 1.0:                                                 # the GPU suite's call without count and streams
            assert evaluate.pl_sample_host(scores, None, 10, T, seed=seed, return_robust=True)[4].all(), (M, "count None")
    for name, (scores, count, streams, k, T, seed) in P.extra_cases().items():
        out = evaluate.pl_sample_host(scores, count, k, T, seed=seed, samples=3, streams=streams, return_robust=True)
        assert out[4].all(), name


def test_the_bound_is_what_the_kernel_file_derives():
    from digat_amd import evaluate
    assert evaluate.pl_bound(100, 0.0) == 116 * 2.0 ** -53
    assert evaluate.pl_bound(100, -3.0) == 116 * 2.0 ** -53 * 4.0
    assert evaluate.pl_bound(1, 0.0, -700.0) == 17 * 2.0 ** -53 + 700 * 2.0 ** -52
    assert evaluate.pl_bound(1, 0.0, -2.0, float32=True) == 17 * 2.0 ** -53 + 2 * 2.0 ** -52 + 2 * 2.0 ** -23
    steps, lz = np.array([[-1.0, -2.0]]), np.array([[0.5, 0.25]])
    per = evaluate.pl_bound(np.array([[4]]), lz, steps)
    assert np.array_equal(evaluate.pl_bound(np.array([[4]]), lz, steps, total=True), per.sum(axis=-1) + 3 * 2.0 ** -53 * 3.0)


# ---------------------------------------------------------------------------------------------------------------------
# off-policy value
# ---------------------------------------------------------------------------------------------------------------------
def test_off_policy_value_on_policy_is_the_mean_and_a_toy_by_hand():
    from digat_amd import evaluate
    rng = np.random.default_rng(2)
    r, lp = rng.random(300), -rng.random(300) * 5
    out = evaluate.off_policy_value(r, lp, lp, replicates=200)
    assert abs(out["ips"]["value"] - r.mean()) < 1e-15 and abs(out["snips"]["value"] - r.mean()) < 1e-15
    assert abs(out["ess"] - 300.0) < 1e-9 and out["max_weight"] == 1.0 and out["n"] == 300
    assert out["ips"]["lo"] <= out["ips"]["value"] <= out["ips"]["hi"] and out["ips"]["replicates"] == 200
    same = evaluate.metric_intervals(r, ("ips",), 200)["ips"]
    assert same == out["ips"], "no new resampling code: metric_intervals' own fields"
    # two slates: weights 2 and 1/2, rewards 1 and 0
    toy = evaluate.off_policy_value([1.0, 0.0], [math.log(0.5), math.log(0.25)], [math.log(0.25), math.log(0.5)], replicates=50)
    assert abs(toy["ips"]["value"] - 1.0) < 1e-15 and abs(toy["snips"]["value"] - 0.8) < 1e-15
    assert abs(toy["ess"] - 2.5 ** 2 / 4.25) < 1e-12 and abs(toy["max_weight"] - 2.0) < 1e-15
    clipped = evaluate.off_policy_value([1.0, 0.0], [math.log(0.5), math.log(0.25)], [math.log(0.25), math.log(0.5)], clip=1.0, replicates=50)
    assert abs(clipped["ips"]["value"] - 0.5) < 1e-15 and abs(clipped["snips"]["value"] - 1.0 / 1.5) < 1e-15 and clipped["max_weight"] == 1.0
    # units keep a user's slates together: the statistic is unchanged, the replicates are not those of the rows
    r4, lt, ll = np.array([1.0, 0.0, 1.0, 1.0]), np.log([0.5, 0.25, 0.2, 0.2]), np.log([0.25, 0.5, 0.2, 0.1])
    rows = evaluate.off_policy_value(r4, lt, ll, replicates=100)
    units = evaluate.off_policy_value(r4, lt, ll, units=np.array([0, 2, 4]), replicates=100)
    assert abs(units["ips"]["value"] - rows["ips"]["value"]) < 1e-15 and abs(units["snips"]["value"] - rows["snips"]["value"]) < 1e-15
    for bad, text in ((dict(reward=[1.0], logp_target=[0.0, 0.0], logp_logging=[0.0]), "one entry per logged slate"),
                      (dict(reward=[1.0], logp_target=[-np.inf], logp_logging=[0.0]), "must be finite"),
                      (dict(reward=[1.0], logp_target=[0.0], logp_logging=[0.0], clip=0.0), "clip must be positive")):
        with pytest.raises(ValueError, match=text):
            evaluate.off_policy_value(**bad)


# ---------------------------------------------------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------------------------------------------------
def test_guards_of_the_twins():
    from digat_amd import evaluate
    sc = np.zeros((3, 8), dtype=np.float32)
    ok = dict(scores=sc, count=None, k=2, temperature=1.0)
    for change, text in ((dict(k=0), "k must be"), (dict(k=129), "k must be"), (dict(k=1.5), "k must be"),
                         (dict(scores=np.zeros((3, 1025), dtype=np.float32)), "PL_MAX_LIST"), (dict(scores=np.zeros((3, 0), dtype=np.float32)), "PL_MAX_LIST"),
                         (dict(scores=np.zeros(8, dtype=np.float32)), r"\[G, M\]"),
                         (dict(temperature=0.0), "temperature must be"), (dict(temperature=-1.0), "temperature must be"),
                         (dict(temperature=float("nan")), "temperature must be"), (dict(temperature=float("inf")), "temperature must be"),
                         (dict(temperature=1e-300), "too small"),
                         (dict(samples=0), "samples must be"), (dict(first_sample=-1), "first_sample must be"),
                         (dict(samples=2, first_sample=(1 << 22) - 1), "PL_MAX_SAMPLE"),
                         (dict(count=np.zeros(2)), "count must have"), (dict(streams=np.zeros(2, dtype=np.int64)), "streams must have"),
                         (dict(streams=np.array([0, 1, 1 << 32])), r"\[0, 2\^32\)"), (dict(streams=np.array([0, -1, 2])), r"\[0, 2\^32\)"),
                         (dict(streams=np.zeros(3)), "integer")):
        with pytest.raises(ValueError, match=text):
            evaluate.pl_sample_host(**{**ok, **change})
    assert evaluate.pl_sample_host(sc, None, 2, 1.0, samples=1, first_sample=(1 << 22) - 1)[0].shape == (3, 1, 2)
    with pytest.raises(ValueError, match="picks must be"):
        evaluate.pl_log_prob_host(sc, None, np.zeros((2, 1, 2), dtype=np.int32), 1.0)
    with pytest.raises(ValueError, match="integer positions"):
        evaluate.pl_log_prob_host(sc, None, np.zeros((3, 1, 2)), 1.0)
    with pytest.raises(ValueError, match="PL_MAX_SAMPLE"):
        evaluate.pl_draws_host(np.arange(2), 1 << 22, 4, first_sample=1)
    with pytest.raises(ValueError, match="PL_MAX_LIST"):
        evaluate.pl_draws_host(np.arange(2), 1, 1025)
    assert evaluate.PL_MAX_LIST == evaluate.SHORTLIST_MAX_K == 1024 and evaluate.PL_MAX_K == evaluate.TOPK_MAX_K == 128


def test_the_header_limits_are_the_ones_python_mirrors():
    import os
    import re
    from conftest import REPO
    from digat_amd import evaluate
    text = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    value = lambda name: re.search(r"#define %s\s+(.+)" % name, text).group(1).strip()
    assert int(value("DIGAT_PL_MAX_LIST")) == evaluate.PL_MAX_LIST and int(value("DIGAT_PL_MAX_K")) == evaluate.PL_MAX_K
    assert value("DIGAT_PL_MAX_SAMPLE") == "(1 << 22)" and evaluate.PL_MAX_SAMPLE == 1 << 22
    assert float(value("DIGAT_PL_CLAMP").strip("()")) == evaluate.PL_CLAMP == -700.0


def test_the_library_refuses_before_any_launch():
    """The C entries' argument checks come before anything touches a device: they answer on a machine without one."""
    import ctypes
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    assert L.digat_pl_sample_workspace_bytes(4096, 1024, 128, 8) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def sample(scores=p, G=1, M=4, k=2, inv_t=1.0, samples=1, first=0, picks=p, n=p, logp=p, step=p):
        return L.digat_pl_sample(scores, None, G, M, k, inv_t, 0, samples, first, None, picks, n, logp, step, None, 0, None)

    def log_prob(scores=p, G=1, M=4, k=2, inv_t=1.0, samples=1, picks=p, logp=p, step=p):
        return L.digat_pl_log_prob(scores, None, G, M, k, inv_t, samples, picks, logp, step, None, 0, None)
    assert sample(G=0) == 0 and log_prob(G=0) == 0, "nobody: no launch"
    arg, shape = sample(scores=None), sample(k=0)
    assert arg != 0 and shape != 0 and arg != shape
    for bad in (dict(picks=None), dict(n=None), dict(logp=None), dict(step=None), dict(G=-1), dict(inv_t=0.0), dict(inv_t=-1.0),
                dict(inv_t=float("nan")), dict(inv_t=float("inf")), dict(inv_t=1e300), dict(logp=p + 4), dict(scores=p + 2)):
        assert sample(**bad) == arg, bad
    for bad in (dict(k=129), dict(M=0), dict(M=1025), dict(G=1 << 31), dict(samples=0), dict(first=-1), dict(samples=2, first=(1 << 22) - 1)):
        assert sample(**bad) == shape, bad
    for bad in (dict(picks=None), dict(logp=None), dict(scores=None), dict(inv_t=float("nan")), dict(picks=p + 1)):
        assert log_prob(**bad) == arg, bad
    for bad in (dict(k=0), dict(M=1025), dict(samples=0)):
        assert log_prob(**bad) == shape, bad


# ---------------------------------------------------------------------------------------------------------------------
# util: the CPU road, the refusals, the flags
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_lists_and_slate_log_prob_on_cpu_tensors():
    from digat_amd import evaluate, util
    scores, count, streams = P.make_case(2, 65)
    rng = np.random.default_rng(4)
    ids = np.stack([rng.permutation(5000)[:65] for _ in range(len(scores))]).astype(np.int64)
    IDS, SC, CNT = torch.from_numpy(ids), torch.from_numpy(scores), torch.from_numpy(count)
    out_ids, out_scores, n_out, logp, step = util.sample_lists(IDS, SC, CNT, 10, 2.0, seed=6, samples=3, streams=streams)
    picks, want_n, want_logp, want_step = evaluate.pl_sample_host(scores, count, 10, 2.0, seed=6, samples=3, streams=streams)
    assert out_ids.dtype == torch.int64 and out_scores.dtype == torch.float32 and tuple(out_ids.shape) == (16, 3, 10)
    hit = picks >= 0
    g = np.arange(16)[:, None, None]
    assert np.array_equal(out_ids.numpy(), np.where(hit, ids[g, np.maximum(picks, 0)], -1))
    want_scores = np.where(hit, scores[g, np.maximum(picks, 0)], -np.inf).astype(np.float32)
    assert np.array_equal(out_scores.numpy().view(np.uint32), want_scores.view(np.uint32)), "the input score bits"
    assert np.array_equal(n_out.numpy(), want_n) and np.array_equal(logp.numpy(), want_logp) and np.array_equal(step.numpy(), want_step)
    # the same slates, by id, under the same scores: the same probabilities, all covered
    lp, st, covered = util.slate_log_prob(IDS, SC, CNT, out_ids, 2.0)
    assert covered.all() and np.array_equal(lp.numpy().view(np.uint64), want_logp.view(np.uint64))
    assert np.array_equal(st.numpy().view(np.uint32), want_step.view(np.uint32))
    # a news that is absent ends the slate there and is reported
    broken = out_ids.clone()
    broken[0, 1, 2] = 4999999
    lp2, st2, cov2 = util.slate_log_prob(IDS, SC, CNT, broken, 2.0)
    assert not cov2[0, 1] and cov2.sum() == cov2.numel() - 1
    assert np.array_equal(st2[0, 1, :2].numpy(), want_step[0, 1, :2]) and (st2[0, 1, 2:] == 0).all()
    # under other scores: the twin on the same positions
    other = torch.from_numpy(rng.standard_normal(scores.shape).astype(np.float32))
    lp3, _, cov3 = util.slate_log_prob(IDS, other, CNT, out_ids, 0.7)
    assert cov3.all() and np.array_equal(lp3.numpy(), evaluate.pl_log_prob_host(other.numpy(), count, picks, 0.7)[0])
    with pytest.raises(ValueError, match="slates must be"):
        util.slate_log_prob(IDS, SC, CNT, out_ids[:3], 2.0)


def test_sample_limits_and_the_refused_combinations():
    from digat_amd import nrms, util
    assert util.sample_limits(10, 0.5, None) == (10, 80, 0.5) and util.sample_limits(128, 2.0, None) == (128, 1024, 2.0)
    assert util.sample_limits(10, 0.5, 1024) == (10, 1024, 0.5) and util.sample_limits(10, 0.5, 10) == (10, 10, 0.5)
    for k, sample, shortlist, text in ((0, 1.0, None, "k must be"), (129, 1.0, None, "k must be"), (10, 0.0, None, "temperature"),
                                       (10, -1.0, None, "temperature"), (10, float("nan"), None, "temperature"),
                                       (10, float("inf"), None, "temperature"), (10, 1.0, 9, "shortlist must lie"), (10, 1.0, 1025, "shortlist must lie")):
        with pytest.raises(ValueError, match=text):
            util.sample_limits(k, sample, shortlist)
    assert util.user_streams(np.arange(4)) is not None and util.user_streams((np.zeros((2, 5)), np.zeros((2, 5)))) is None

    def never(*a, **k):
        raise AssertionError("refused before anything is scored")
    with pytest.raises(ValueError, match="temperature"):
        util.shortlist_then_sample(never, 10, 0.0)
    with pytest.raises(ValueError, match="samples must be"):
        util.shortlist_then_sample(never, 10, 1.0, samples=0)
    # both recommends refuse before they look at the model or the corpus
    for fn in (lambda **kw: util.recommend(None, None, np.arange(2), np.arange(1, 9), 3, **kw),
               lambda **kw: nrms.recommend(None, None, np.arange(2), k=3, **kw)):
        for kw in (dict(sample=1.0, diversity=0.3), dict(sample=1.0, diversity=0.0), dict(sample=1.0, calibration=0.5),
                   dict(sample=1.0, max_per_category=2), dict(sample=1.0, calibration_target=np.zeros((2, 3))), dict(sample=1.0, category=np.zeros(9))):
            with pytest.raises(ValueError, match="sample does not combine"):
                fn(**kw)
        for kw in (dict(seed=3), dict(streams=np.arange(2))):
            with pytest.raises(ValueError, match="belong to a sampled call"):
                fn(**kw)
        for kw in (dict(sample=0.0), dict(sample=float("nan")), dict(sample=1.0, shortlist=2)):
            with pytest.raises(ValueError):
                fn(**kw)
    with pytest.raises(ValueError, match="sample does not combine with index"):
        nrms.recommend(None, None, np.arange(2), k=3, sample=1.0, index=object())


def test_config_parses_the_sample_flags(capsys):
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not hasattr(c, "recommend_sample") and not hasattr(c, "recommend_seed"), "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_sample", "0.5"])
    assert c.recommend_sample == 0.5 and c.recommend_seed == 0 and c.recommend_shortlist == 0
    assert not hasattr(c, "recommend_calibration") and not hasattr(c, "recommend_diversity")
    c = Config(["--mode", "recommend", "--recommend_sample", "2", "--recommend_seed", "7", "--recommend_shortlist", "1024"])
    assert c.recommend_sample == 2.0 and c.recommend_seed == 7 and c.recommend_shortlist == 1024
    c = Config(["--mode", "recommend", "--recommend_calibration", "0.5"])
    assert not hasattr(c, "recommend_sample") and not hasattr(c, "recommend_seed")
    for bad, text in ((["--recommend_sample", "0"], "positive and finite"), (["--recommend_sample", "-1"], "positive and finite"),
                      (["--recommend_sample", "nan"], "positive and finite"),
                      (["--recommend_sample", "1", "--recommend_diversity", "0.3"], "does not combine"),
                      (["--recommend_sample", "1", "--recommend_calibration", "0.3"], "does not combine"),
                      (["--recommend_sample", "1", "--recommend_report", "0,0.1"], "does not combine"),
                      (["--recommend_sample", "1", "--recommend_max_per_category", "2"], "does not combine"),
                      (["--recommend_seed", "3"], "--recommend_seed needs --recommend_sample"),
                      (["--recommend_sample", "1", "--recommend_shortlist", "-1"], "must not be negative")):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend"] + bad)
        assert text in capsys.readouterr().err, bad


# ---------------------------------------------------------------------------------------------------------------------
# the planted match
# ---------------------------------------------------------------------------------------------------------------------
def test_planted_match_is_the_corpus_own_and_leaves_make_corpus_alone():
    import dataclasses
    from digat_amd import synthetic
    spec = synthetic.SynthSpec(news_num=600, impressions=150, seed=17, signal=2.0, embedding_dim=32, max_history_num=12, category_num=6)
    before = synthetic.make_corpus(spec)
    pref, news_sub = synthetic.planted_match(before)
    after = synthetic.make_corpus(spec)
    for f in dataclasses.fields(before):
        a, b = getattr(before, f.name), getattr(after, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f.name
    rng = np.random.default_rng(spec.seed)                                   # what _plant_preferences itself made of the same spec
    planted = synthetic._plant_preferences(spec, before.news_category, np.zeros((spec.news_num, spec.embedding_dim), dtype=np.float32),
                                           np.zeros((spec.impressions, spec.max_history_num), dtype=np.int32))
    assert np.array_equal(planted["news_sub"], news_sub) and np.array_equal(planted["pref"], pref)
    assert pref.shape == (150, 3) and news_sub.shape == (600,) and (pref[:, 0] >= 0).all() and (pref == -1).any()
    assert np.array_equal(news_sub // spec.subtopics_per_category, before.news_category)
    # the signal is there: a history holds the user's preferred sub-topics far more often than chance
    hist = before.history
    match = ((news_sub[hist][:, :, None] == pref[:, None, :]) & (hist[:, :, None] > 0)).any(axis=2).sum() / max(1, (hist > 0).sum())
    assert match > 0.5
    # the reward: 1 for a preferred sub-topic, 1/2 for its category, empty slots out of the mean
    S = spec.subtopics_per_category
    user = 0
    sub0 = int(pref[user, 0])
    same_sub = int(np.flatnonzero(news_sub == sub0)[0])
    same_cat = np.flatnonzero((news_sub // S == sub0 // S) & ~np.isin(news_sub, pref[user]))
    other = np.flatnonzero(~np.isin(news_sub // S, pref[user][pref[user] >= 0] // S))
    slate = np.array([[[same_sub, int(other[0]), -1]]])
    assert synthetic.planted_reward(pref[:1], news_sub, slate, S)[0, 0] == 0.5
    if len(same_cat):
        assert synthetic.planted_reward(pref[:1], news_sub, np.array([[[int(same_cat[0]), same_sub, int(other[0]), int(other[1])]]]), S)[0, 0] == 0.375
    assert synthetic.planted_reward(pref[:1], news_sub, np.array([[[-1, -1]]]), S)[0, 0] == 0.0
    with pytest.raises(ValueError, match="planted-signal"):
        synthetic.planted_match(synthetic.make_corpus(dataclasses.replace(spec, signal=0.0)))
