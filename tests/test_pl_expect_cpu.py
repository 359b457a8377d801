"""CPU suite: the host side of the doubly robust off-policy value — ``evaluate.pl_expect_host`` (the numpy float64 twin of
``digat_pl_expect``), ``evaluate.off_policy_steps`` and the ABI entry.  The estimators are held to the truth by exhaustive
enumeration: over ALL ordered slates of a small list, the logging policy's expectation of either estimator is the target's value."""
import itertools
import os
import re

import numpy as np
import pytest

import pl_expect_common as E
from conftest import REPO


def _enumeration(k, seed=0, M=5):
    """Every ordered slate of k out of M as one list with S slates, arbitrary logging and target scores, an item-and-position reward
    table, a value per item and a weight per position; the twin's float64 steps under either policy."""
    from digat_amd import evaluate
    rng = np.random.default_rng(seed)
    picks = np.array(list(itertools.permutations(range(M), k)), dtype=np.int32)[None]            # [1, S, k]
    logging, target = (rng.standard_normal((1, M)).astype(np.float32) for _ in range(2))
    table = rng.standard_normal((M, k))
    values = rng.standard_normal((1, M)).astype(np.float32)
    weight = rng.uniform(0.5, 1.5, size=k)
    t_log, t_tgt = 0.7, 1.3
    log = evaluate.pl_log_prob_host(logging, None, picks, t_log, parts=True)
    tgt = evaluate.pl_expect_host(target, None, picks, values, t_tgt, parts=True)
    reward = table[picks[0], np.arange(k)[None, :]]                                              # [S, k]
    return picks, reward, table, values, weight, log, tgt


def _per_slate(reward, tgt, log, **kw):
    """Either estimator of every slate alone: ``off_policy_steps`` on one row is that row's term.  The float64 steps of the twins'
    parts are used: the float32 ``step_logp`` would put 2^-24 into every ratio."""
    from digat_amd import evaluate
    pdis, dr = [], []
    for s in range(reward.shape[0]):
        out = evaluate.off_policy_steps(reward[s:s + 1], tgt[5]["step"][0, s:s + 1], log[2]["step"][0, s:s + 1], tgt[4][0, s:s + 1],
                                        tgt[2][0, s:s + 1], tgt[3][0, s:s + 1], replicates=1, **kw)
        pdis.append(out["pdis"]["value"])
        dr.append(out["dr"]["value"])
    return np.array(pdis), np.array(dr)


@pytest.mark.parametrize("seed", [0, 1])
def test_both_estimators_are_unbiased_over_all_sixty_slates(seed):
    picks, reward, table, values, weight, log, tgt = _enumeration(3, seed)
    assert picks.shape == (1, 60, 3)
    mu, pi = np.exp(log[0][0]), np.exp(tgt[0][0])
    assert abs(mu.sum() - 1.0) < 1e-12 and abs(pi.sum() - 1.0) < 1e-12
    truth = float(np.sum(pi * reward.sum(axis=1)))
    pdis, dr = _per_slate(reward, tgt, log, position_weight=weight)
    for name, est in (("pdis", pdis), ("dr", dr)):
        got, scale = float(np.sum(mu * est)), float(np.sum(np.abs(mu * est)))
        print(f"seed {seed}: truth {truth!r} {name} {got!r}")
        assert abs(got - truth) <= 1e-12 * scale, (name, got, truth)
    assert np.abs(dr - pdis).max() > 1e-3, "the value model moves the single terms"


def test_dr_has_no_variance_when_the_values_are_the_reward_of_a_single_step():
    from digat_amd import evaluate
    picks, _, _, _, _, log, _ = _enumeration(1, 3)
    rng = np.random.default_rng(5)
    target = rng.standard_normal((1, 5)).astype(np.float32)
    values = rng.standard_normal((1, 5)).astype(np.float32)
    tgt = evaluate.pl_expect_host(target, None, picks, values, 0.9, parts=True)
    reward = values[0].astype(np.float64)[picks[0]]                                              # [5, 1]
    truth = float(np.sum(np.exp(tgt[0][0]) * reward[:, 0]))
    pdis, dr = _per_slate(reward, tgt, log)
    assert np.abs(dr - truth).max() <= 1e-12 * abs(truth), (dr, truth)
    assert np.abs(pdis - truth).max() > 1e-2


@pytest.mark.parametrize("M,k,S,T", [(5, 3, 2, 1.0), (65, 10, 3, 0.05), (129, 128, 1, 8.0)])
def test_twin_is_the_log_prob_twin_with_the_expectation_beside_it(M, k, S, T):
    from digat_amd import evaluate
    (scores, count, values, picks), want = E.case_and_twin(M, k, S, T)
    logp, step, mean, used, length, parts = want
    ref = evaluate.pl_log_prob_host(scores, count, picks, T, parts=True)
    assert np.array_equal(E.bits(logp), E.bits(ref[0])) and np.array_equal(E.bits(step), E.bits(ref[1]))
    assert np.array_equal(length, ref[2]["length"]) and length.dtype == np.int32
    assert mean.dtype == np.float64 and used.dtype == np.float32 and mean.shape == used.shape == (E.G, S, k)
    beyond = np.arange(k)[None, None, :] >= length[:, :, None]
    assert not mean[beyond].any() and not used[beyond].any() and not step[beyond].any()
    assert (length[1] == 0).all() and (length[2] <= 3).all() and int(length[4, 0]) <= k // 2, "the empty list, the short one and the -1"
    if k >= 3 and M >= 2:
        assert int(length[2, 0]) == 2, "cut by the repeat"
    assert (np.abs(mean) <= parts["absolute"] * (1 + 1e-15)).all()
    # a direct evaluation of one step
    g, s = 0, 0
    n = int(length[g, s])
    assert n == min(M, k)
    v = np.where(np.isfinite(values[g]), values[g], 0).astype(np.float64)
    a = scores[g].astype(np.float64) * (1.0 / T)
    w = np.exp(np.maximum(a - a.max(), -700.0))
    left = np.ones(M, dtype=bool)
    left[picks[g, s, :n - 1]] = False
    assert abs(mean[g, s, n - 1] - np.sum(w[left] * v[left]) / np.sum(w[left])) <= 1e-12 * parts["absolute"][g, s, n - 1] + 1e-300
    assert used[g, s, n - 1] == np.float32(v[picks[g, s, n - 1]])
    # values that are all 0: exactly 0; a value that is not finite: as if it were 0
    zero = evaluate.pl_expect_host(scores, count, picks, np.zeros_like(values), T)
    assert not zero[2].any() and not zero[3].any() and not np.signbit(zero[2]).any()
    cleaned = evaluate.pl_expect_host(scores, count, picks, np.where(np.isfinite(values), values, np.float32(0)), T)
    assert not np.isfinite(values).all()
    assert np.array_equal(E.bits(cleaned[2]), E.bits(mean)) and np.array_equal(E.bits(cleaned[3]), E.bits(used))
    if M >= 64:
        shown = ~beyond & (parts["absolute"] > 0)
        assert (np.abs(mean[shown]) / parts["absolute"][shown]).min() < 1e-2, "signed values: the mean cancels somewhere"
    with pytest.raises(ValueError):
        evaluate.pl_expect_host(scores, count, picks, values[:, :-1] if M > 1 else values[:-1], T)


def test_bound_has_the_stated_form():
    from digat_amd import evaluate
    b = evaluate.pl_expect_bound(np.array([1, 1024]), np.array([2.0, 2.0]), np.array([-1.0, 0.0]))
    assert np.array_equal(b, np.array([14 * 2.0 ** -53 * 2.0 + 2.0 ** -52, 2060 * 2.0 ** -53 * 2.0]))


def _steps_case(n=12, k=4, seed=2):
    rng = np.random.default_rng(seed)
    reward = rng.uniform(size=(n, k))
    lt, ll = -rng.uniform(0.5, 3.0, size=(n, k)), -rng.uniform(0.5, 3.0, size=(n, k))
    length = rng.integers(0, k + 1, size=n).astype(np.int32)
    length[0], length[1] = k, 0
    return reward, lt, ll, length, rng.standard_normal((n, k)), rng.standard_normal((n, k))


def test_steps_follow_their_formulas_with_clip_and_units():
    from digat_amd import evaluate
    reward, lt, ll, length, sm, sv = _steps_case()
    n, k = reward.shape
    D = np.array([1.0, 0.5, 0.25, 2.0])
    for clip in (None, 1.5):
        pdis, dr, rho_all = np.zeros(n), np.zeros(n), np.zeros((n, k))
        for i in range(n):
            before = 1.0
            for t in range(int(length[i])):
                rho = float(np.exp(np.sum(lt[i, :t + 1] - ll[i, :t + 1])))
                rho = rho if clip is None else min(rho, clip)
                rho_all[i, t] = rho
                pdis[i] += rho * reward[i, t]
                dr[i] += rho * (reward[i, t] - D[t] * sv[i, t]) + before * D[t] * sm[i, t]
                before = rho
        out = evaluate.off_policy_steps(reward, lt, ll, length, sm, sv, position_weight=D, clip=clip, replicates=50, seed=3)
        assert abs(out["pdis"]["value"] - pdis.mean()) <= 1e-12 * np.abs(pdis).mean()
        assert abs(out["dr"]["value"] - dr.mean()) <= 1e-12 * np.abs(dr).mean()
        assert out["n"] == n and out["ess"].shape == (k,) and out["max_weight"].shape == (k,)
        assert np.allclose(out["max_weight"], rho_all.max(axis=0), rtol=1e-12)
        assert np.allclose(out["ess"], rho_all.sum(axis=0) ** 2 / (rho_all ** 2).sum(axis=0), rtol=1e-12)
        if clip is not None:
            assert out["max_weight"].max() <= clip and rho_all.max() == clip
        want = evaluate.metric_intervals(np.stack([pdis, dr], axis=1), ("pdis", "dr"), 50, 0.95, 3)
        for name in ("pdis", "dr"):
            assert out[name]["lo"] == pytest.approx(want[name]["lo"], rel=1e-12) and out[name]["hi"] == pytest.approx(want[name]["hi"], rel=1e-12)
        units = np.arange(0, n + 1, 3)
        grouped = evaluate.off_policy_steps(reward, lt, ll, length, sm, sv, position_weight=D, clip=clip, units=units, replicates=50, seed=3)
        want = evaluate.metric_intervals(np.stack([pdis, dr], axis=1), ("pdis", "dr"), 50, 0.95, 3, units=units)
        for name in ("pdis", "dr"):
            assert grouped[name]["value"] == pytest.approx(out[name]["value"], rel=1e-12)
            assert grouped[name]["lo"] == pytest.approx(want[name]["lo"], rel=1e-12) and grouped[name]["se"] == pytest.approx(want[name]["se"], rel=1e-12)
    plain = evaluate.off_policy_steps(reward, lt, ll, length, replicates=10)
    assert plain["dr"] == plain["pdis"], "without a value model dr is pdis"
    same_len = evaluate.off_policy_steps(reward, lt, ll, length, sm, sv, replicates=10, length_logging=length.astype(np.int64))
    assert same_len["n"] == n


def test_steps_refuse_what_they_cannot_weigh():
    from digat_amd import evaluate
    reward, lt, ll, length, sm, sv = _steps_case()
    n, k = reward.shape
    for name, arrays in (("reward", (reward.copy(), lt, ll, length, sm, sv)), ("target", (reward, lt.copy(), ll, length, sm, sv)),
                         ("logging", (reward, lt, ll.copy(), length, sm, sv)), ("mean", (reward, lt, ll, length, sm.copy(), sv)),
                         ("value", (reward, lt, ll, length, sm, sv.copy()))):
        index = {"reward": 0, "target": 1, "logging": 2, "mean": 4, "value": 5}[name]
        arrays[index][3, 1] = np.nan if name != "target" else -np.inf
        with pytest.raises(ValueError, match="finite"):
            evaluate.off_policy_steps(*arrays, replicates=10)
    other = length.copy()
    other[5] = (other[5] + 1) % (k + 1)
    with pytest.raises(ValueError, match="slate 5"):
        evaluate.off_policy_steps(reward, lt, ll, length, sm, sv, replicates=10, length_logging=other)
    for bad in (lambda: evaluate.off_policy_steps(reward, lt[:, :-1], ll, length),
                lambda: evaluate.off_policy_steps(reward[0], lt[0], ll[0], length),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length[:-1]),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length.astype(np.float64)),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length + k),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length, sm),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length, sm[:, :-1], sv),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length, sm, sv, position_weight=np.ones(k + 1)),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length, clip=0.0),
                lambda: evaluate.off_policy_steps(reward, lt + 800.0, ll, length),
                lambda: evaluate.off_policy_steps(reward, lt, ll, length, units=np.array([0, 5]))):
        with pytest.raises(ValueError):
            bad()


def test_slate_step_values_and_the_report_run_on_cpu_tensors():
    import torch
    from digat_amd import evaluate, util
    rng = np.random.default_rng(11)
    G, M, k, S = 12, 20, 4, 2
    ids = torch.from_numpy(np.stack([rng.permutation(1000)[:M] for _ in range(G)]).astype(np.int64))
    scores = torch.from_numpy(rng.standard_normal((G, M)).astype(np.float32))
    count = torch.from_numpy(rng.integers(6, M + 1, size=G).astype(np.int32))
    values = torch.from_numpy(rng.standard_normal((G, M)).astype(np.float32))
    slates, slate_scores, n_out, logp, step = util.sample_lists(ids, scores, count, k, 1.0, seed=4, samples=S)
    log = {"ids": ids, "scores": scores, "count": count, "slates": slates, "slate_scores": slate_scores, "n_out": n_out, "logp": logp,
           "step_logp": step, "temperature": 1.0, "seed": 4}
    out = util.slate_step_values(ids, scores, count, slates, 1.0, values)
    assert len(out) == 6 and bool(out[5].all())
    want = evaluate.pl_expect_host(scores.numpy(), count.numpy(), util.slate_positions(ids, count, slates).numpy(), values.numpy(), 1.0)
    for got, ref in zip(out[:5], want):
        assert np.array_equal(E.bits(got), E.bits(ref))
    assert np.array_equal(E.bits(out[0]), E.bits(logp)) and np.array_equal(E.bits(out[1]), E.bits(step)), "the policy's own log"
    target = scores + torch.from_numpy(rng.standard_normal((G, M)).astype(np.float32)) * 0.3
    reward = rng.uniform(size=(G, S, k))
    rep = util.off_policy_report(log, target, reward, values=values, position_weight=np.ones(k), replicates=100)
    assert {"ips", "snips", "pdis", "dr", "ess", "max_weight", "step_ess", "step_max_weight", "n", "dropped"} <= set(rep)
    assert rep["n"] == G * S and rep["dropped"] == 0
    for name in ("ips", "snips", "pdis", "dr"):
        assert all(np.isfinite(rep[name][f]) for f in ("value", "lo", "hi", "se")), name
    assert "dr" not in util.off_policy_report(log, target, reward, replicates=20)
    # on the logging policy itself every ratio is 1: all three weighted estimators are the mean summed reward
    own = util.off_policy_report(log, scores, reward, values=values, replicates=20)
    assert own["pdis"]["value"] == pytest.approx(reward.sum(axis=2).mean(), rel=1e-6) and own["ips"]["value"] == pytest.approx(own["pdis"]["value"], rel=1e-6)
    # a target that cannot draw a logged item: the slate is left out and counted
    blind = target.clone()
    first = util.slate_positions(ids, count, slates)[0, 0, 1].item()
    blind[0, first] = float("-inf")
    cut = util.off_policy_report(log, blind, reward, values=values, replicates=20)
    assert cut["dropped"] >= 1 and cut["n"] == G * S - cut["dropped"]
    with pytest.raises(ValueError):
        util.off_policy_report(log, blind, reward, values=values, replicates=20, units=np.arange(0, G * S + 1, S))


def test_entry_is_declared_and_exported():
    from digat_amd import _lib, build
    build.build(verbose=False)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "digat_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+digat_pl_expect\s*\(", text)
    assert "digat_pl_expect" in _lib.EXPORTED and hasattr(_lib.lib(), "digat_pl_expect")
    declared = re.search(r"digat_pl_expect\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(_lib.lib().digat_pl_expect.argtypes) == len(declared.split(",")) == 17
    assert _lib.lib().digat_version() == 4
