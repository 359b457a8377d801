"""GPU suite: ``digat_pl_expect`` (``evaluate.pl_expect``) and what stands on it — ``util.slate_step_values``,
``util.off_policy_report``.  ``logp`` and ``step_logp`` are held bit for bit to ``evaluate.pl_log_prob`` on the same inputs, ``length``,
``step_value`` and the contractual zeros exactly to the host twin (``evaluate.pl_expect_host``; cases and twin results from
tests/pl_expect_common.py), ``step_mean`` inside ``evaluate.pl_expect_bound``, the worst error-to-bound ratio printed."""
import numpy as np
import pytest
import torch

import pl_expect_common as E

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(_dev())             # a copy: the shared cases are read-only


def _identical(a, b, what=""):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and np.array_equal(E.bits(x), E.bits(y)), what


@pytest.mark.parametrize("T", E.TS)
@pytest.mark.parametrize("k", E.KS)
@pytest.mark.parametrize("M", E.MS)
def test_probabilities_are_log_probs_and_the_expectation_is_within_the_bound(M, k, T):
    from digat_amd import evaluate
    for S in E.SS:
        (scores, count, values, picks), want = E.case_and_twin(M, k, S, T)
        SC, CNT, VL, PK = _t(scores), _t(count), _t(values), _t(picks)
        got = evaluate.pl_expect(SC, CNT, PK, VL, T)
        assert all(t.is_cuda for t in got) and tuple(got[2].shape) == (E.G, S, k)
        _identical(got[:2], evaluate.pl_log_prob(SC, CNT, PK, T), "logp and step_logp are pl_log_prob's")
        ratio = E.same(got, want, (M, k, S, T))
        print(f"pl_expect M={M} k={k} S={S} T={T}: worst |step_mean - twin| / bound = {ratio:.4f}")
        assert (want[4][1] == 0).all() and (want[4][2] <= 3).all(), "an empty list and a short one are among the cases"
    if k == 10 and T == 1.0:                                              # count=None is M
        _identical(evaluate.pl_expect(SC, None, PK, VL, T), evaluate.pl_expect(SC, torch.full_like(CNT, M), PK, VL, T), "count None")


def test_a_spread_above_700_temperatures_sits_on_the_clamp():
    from digat_amd import evaluate
    scores, count, values, picks, T = E.clamp_case()
    want = evaluate.pl_expect_host(scores, count, picks, values, T, parts=True)
    got = evaluate.pl_expect(_t(scores), _t(count), _t(picks), _t(values), T)
    _identical(got[:2], evaluate.pl_log_prob(_t(scores), _t(count), _t(picks), T), "clamp: pl_log_prob's bits")
    ratio = E.same(got, want, "clamp")
    print(f"pl_expect clamp: worst |step_mean - twin| / bound = {ratio:.4f}")
    assert (scores.max(axis=1) - scores.min(axis=1) > 700.0 * T).all(), "every list has entries on the clamp"
    assert int(want[4].max()) == picks.shape[2], "a full slate ends among the clamped entries"


@pytest.mark.parametrize("M,k", [(65, 10), (1024, 128)])
def test_two_calls_and_a_list_alone_agree_bit_for_bit(M, k):
    from digat_amd import evaluate
    scores, count, values, picks = E.make_case(M, k, 3, groups=65)
    SC, CNT, VL, PK = _t(scores), _t(count), _t(values), _t(picks)
    whole = evaluate.pl_expect(SC, CNT, PK, VL, 1.0)
    _identical(whole, evaluate.pl_expect(SC, CNT, PK, VL, 1.0), "two calls")
    for g in (0, 1, 2, 3, 4, 37, 64):
        one = evaluate.pl_expect(SC[g:g + 1], CNT[g:g + 1], PK[g:g + 1], VL[g:g + 1], 1.0)
        _identical(one, tuple(t[g:g + 1] for t in whole), ("alone", g))
    assert int(whole[4].max()) == min(M, k) and int(whole[4].min()) == 0


def test_slate_step_values_is_pl_expect_on_the_matched_positions_and_the_report_runs():
    from digat_amd import evaluate, util
    rng = np.random.default_rng(21)
    G, M, k, S = 64, 80, 10, 2
    ids = _t(np.stack([rng.permutation(5000)[:M] for _ in range(G)]).astype(np.int64))
    scores = _t(rng.standard_normal((G, M)).astype(np.float32) * 2.0)
    count_host = rng.integers(12, M + 1, size=G).astype(np.int32)
    count_host[3] = 4                                                    # fewer entries than k
    count = _t(count_host)
    values = _t(rng.standard_normal((G, M)).astype(np.float32))
    slates, slate_scores, n_out, logp, step = util.sample_lists(ids, scores, count, k, 1.0, seed=6, samples=S)
    target = scores + _t(rng.standard_normal((G, M)).astype(np.float32))
    out = util.slate_step_values(ids, target, count, slates, 0.5, values)
    assert len(out) == 6 and all(t.is_cuda for t in out) and bool(out[5].all())
    _identical(out[:5], evaluate.pl_expect(target, count, util.slate_positions(ids, count, slates), values, 0.5), "slate_step_values")
    assert torch.equal(out[4], n_out[:, None].expand(G, S))
    log = {"ids": ids, "scores": scores, "count": count, "slates": slates, "slate_scores": slate_scores, "n_out": n_out, "logp": logp,
           "step_logp": step, "temperature": 1.0, "seed": 6}
    reward = rng.uniform(size=(G, S, k))
    rep = util.off_policy_report(log, target, reward, values=values, temperature=0.5, replicates=200, units=np.arange(0, G * S + 1, S))
    assert rep["n"] == G * S and rep["dropped"] == 0
    for name in ("ips", "snips", "pdis", "dr"):
        assert all(np.isfinite(rep[name][f]) for f in ("value", "lo", "hi", "se")), name
    assert np.isfinite(rep["step_ess"]).all() and np.isfinite(rep["step_max_weight"]).all() and rep["step_ess"].shape == (k,)
    assert np.isfinite(rep["ess"]) and np.isfinite(rep["max_weight"])
