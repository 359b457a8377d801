"""CPU suite of the bootstrap instrument: the host twin of ``digat_bootstrap_sums`` (draws, sums, segment sums), the statistics
built on it (``metric_intervals``, ``compare_metrics``, ``rank_metric_columns`` / ``rank_metrics_intervals``,
``impression_metrics`` on host scores), every refusal, and the C entries' argument checks — which return before any HIP call."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import bootstrap_common as BC
import dot_rank_common as R
from conftest import REPO

NEW = ("digat_bootstrap_workspace_bytes", "digat_bootstrap_sums", "digat_segment_sums_f64")


# ---------------------------------------------------------------------------------------------------------------------
# hash and draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,seed,r0", [(1, 3, 0, 0), (37, 5, 123, 3), (1000, 2, 0xFFFFFFFF, 0), (7, 4, 5, (1 << 32) // 7 - 2),
                                         (3, 2, 9, (1 << 31) - 2)])
def test_vectorised_draws_equal_the_scalar_restatement(n, B, seed, r0):
    from digat_amd import evaluate
    idx = evaluate.bootstrap_draws_host(n, B, seed, r0)
    assert idx.shape == (B, n) and idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n
    want = [[BC.draw(n, r0 + b, j, seed) for j in range(n)] for b in range(B)]
    assert idx.tolist() == want
    if r0 == (1 << 32) // 7 - 2:
        assert (r0 * n) < (1 << 32) <= (r0 + B) * n, "these counters cross 2^32: the inner hash changes on the way"


def test_first_replicate_shifts_replicates_and_changes_nothing_else():
    from digat_amd import evaluate
    whole = evaluate.bootstrap_draws_host(50, 9, seed=4)
    assert np.array_equal(evaluate.bootstrap_draws_host(50, 4, seed=4, first_replicate=5), whole[5:])
    assert np.array_equal(evaluate.bootstrap_draws_host(50, 5, seed=4), whole[:5])
    assert not np.array_equal(evaluate.bootstrap_draws_host(50, 9, seed=5), whole), "the seed matters"
    assert np.array_equal(evaluate.bootstrap_draws_host(50, 9, seed=4 + (1 << 32)), whole), "the low 32 bits of the seed are the seed"
    v = BC.real_values(1, 50, 3)
    sums = evaluate.bootstrap_sums_host(v, 9, seed=4)
    assert np.array_equal(evaluate.bootstrap_sums_host(v, 4, seed=4, first_replicate=5), sums[5:])
    assert np.array_equal(evaluate.bootstrap_sums_host(v[:, 1], 9, seed=4), sums[:, 1:2]), "a column's sums do not depend on the others"


def test_importing_evaluate_does_not_import_torch():
    import subprocess
    code = "import sys; from digat_amd import evaluate; evaluate.bootstrap_draws_host(5, 2); assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0


@pytest.mark.parametrize("seed", range(5))
def test_draws_are_uniform_and_replicate_means_have_the_standard_error(seed):
    """n = 1000, B = 2000.  The unit counts are multinomial(B n, 1/n): their chi-square over its n degrees of freedom has mean 1 and
    standard deviation sqrt(2 / n), held to six of them; the replicate means' standard deviation is an estimate of sigma / sqrt(n)
    from B samples, relative standard deviation 1 / sqrt(2 B), held to six of them.  Measured on the host twin: chi-square
    0.982 - 1.067, se ratio 0.988 - 1.026 over the five seeds."""
    from digat_amd import evaluate
    n, B = 1000, 2000
    idx = evaluate.bootstrap_draws_host(n, B, seed)
    count = np.bincount(idx.ravel(), minlength=n).astype(np.float64)
    chi = ((count - B) ** 2 / B).sum() / n
    print("chi-square / n", chi)
    assert abs(chi - 1.0) <= 6.0 * math.sqrt(2.0 / n)
    v = np.random.default_rng(100 + seed).standard_normal(n)
    means = evaluate.bootstrap_sums_host(v, B, seed)[:, 0] / n
    ratio = means.std(ddof=1) / (v.std(ddof=0) / math.sqrt(n))          # the bootstrap's own sigma: the plug-in one
    print("se ratio", ratio)
    assert abs(ratio - 1.0) <= 6.0 / math.sqrt(2.0 * B)


def test_host_sums_are_correctly_rounded():
    from digat_amd import evaluate
    v = np.array([[1e16, 1.0], [1.0, 2.0 ** -60], [-1e16, 1.0], [1.0, 1.0]])
    idx = evaluate.bootstrap_draws_host(4, 6, seed=2)
    got = evaluate.bootstrap_sums_host(v, 6, seed=2)
    from fractions import Fraction
    for b in range(6):
        for k in range(2):
            exact = sum(Fraction(float(v[i, k])) for i in idx[b])
            assert got[b, k] == float(exact), (b, k)


# ---------------------------------------------------------------------------------------------------------------------
# segment sums
# ---------------------------------------------------------------------------------------------------------------------
def test_segment_sums_host_adds_left_to_right():
    from digat_amd import evaluate
    v = BC.real_values(3, 40, 3)
    start = np.array([0, 0, 1, 1, 17, 40, 40])
    got = evaluate.segment_sums_host(v, start)
    assert got.shape == (6, 3)
    for u in range(6):
        for k in range(3):
            s = 0.0
            for r in range(start[u], start[u + 1]):
                s += float(v[r, k])
            assert got[u, k] == s, (u, k)
    assert (got[0] == 0).all() and (got[2] == 0).all() and np.array_equal(got[1], v[0])
    assert evaluate.segment_sums_host(v[:, 0], start).shape == (6, 1)
    for bad in (np.array([0, 5, 3, 40]), np.array([1, 40]), np.array([0, 39]), np.zeros(0, dtype=np.int64), np.array([0.0, 40.0])):
        with pytest.raises(ValueError, match="start"):
            evaluate.segment_sums_host(v, bad)


# ---------------------------------------------------------------------------------------------------------------------
# the statistics on hand-built replicates
# ---------------------------------------------------------------------------------------------------------------------
def test_interval_and_paired_fields_on_hand_built_replicates():
    from digat_amd import evaluate
    stats = np.array([3.0, 1.0, 2.0, 5.0, 4.0])
    f = evaluate.interval_fields(2.5, stats, 0.5)                   # quantiles 0.25 and 0.75 of 1..5: positions 1 and 3
    assert f == {"value": 2.5, "lo": 2.0, "hi": 4.0, "se": math.sqrt(2.5), "replicates": 5, "level": 0.5}
    f = evaluate.interval_fields(0.0, stats, 0.9)                   # positions 0.2 and 3.8
    assert f["lo"] == pytest.approx(1.2, rel=1e-15) and f["hi"] == pytest.approx(4.8, rel=1e-15)
    assert math.isnan(evaluate.interval_fields(1.0, [7.0], 0.95)["se"]) and evaluate.interval_fields(1.0, [7.0], 0.95)["lo"] == 7.0
    d = np.array([0.5, -0.25, 0.0, 1.0, 2.0, 0.0, 3.0, 0.75])       # 3 of 8 <= 0, 7 of 8 >= 0, 5 of 8 > 0
    p = evaluate.paired_fields(2.0, 1.5, d, 0.5)
    assert p["a"] == 2.0 and p["b"] == 1.5 and p["diff"] == 0.5 and p["p"] == 2.0 * 4 / 9 and p["wins"] == 5 / 8
    assert p["lo"] == BC.quantile_linear(d, 0.25) and p["hi"] == BC.quantile_linear(d, 0.75) and p["se"] == pytest.approx(np.std(d, ddof=1), rel=1e-15)
    assert list(p) == ["a", "b", "diff", "lo", "hi", "se", "p", "wins"]
    assert evaluate.paired_fields(1.0, 1.0, np.zeros(9), 0.95) == {"a": 1.0, "b": 1.0, "diff": 0.0, "lo": 0.0, "hi": 0.0, "se": 0.0, "p": 1.0,
                                                                  "wins": 0.0}
    assert evaluate.paired_fields(1.0, 0.0, np.ones(999), 0.95)["p"] == 2.0 / 1000, "never 0: (0 + 1) / (B + 1), two-sided"


# ---------------------------------------------------------------------------------------------------------------------
# metric_intervals / compare_metrics against a direct numpy computation from the draws
# ---------------------------------------------------------------------------------------------------------------------
def _direct(values, den, B, seed, level):
    """name-less direct computation: per column, the interval fields from ``bootstrap_draws_host`` and ``math.fsum``."""
    from digat_amd import evaluate
    n, c = values.shape
    idx = evaluate.bootstrap_draws_host(n, B, seed)
    fs = lambda x: math.fsum(float(t) for t in x)
    out = []
    for k in range(c):
        dk = None if den is None else den[:, k if den.shape[1] > 1 else 0]
        total = float(np.sum(np.ascontiguousarray(values[:, k])))
        value = total / n if dk is None else total / float(np.sum(np.ascontiguousarray(dk)))
        stats = [fs(values[idx[b], k]) / (n if dk is None else fs(dk[idx[b]])) for b in range(B)]
        out.append((value, np.array(stats)))
    return out


def test_metric_intervals_host_path_is_the_direct_computation():
    from digat_amd import evaluate
    n, B, seed, level = 300, 64, 11, 0.9
    v = BC.real_values(2, n, 3)
    got = evaluate.metric_intervals(v, names=("x", "y", "z"), replicates=B, level=level, seed=seed)
    want = {name: BC.direct_interval(s, value, level) for name, (value, s) in zip("xyz", _direct(v, None, B, seed, level))}
    BC.same_fields(got, want, 1e-14, "means")
    assert evaluate.metric_intervals(torch.from_numpy(v), names=("x", "y", "z"), replicates=B, level=level, seed=seed) == got, "a CPU tensor"
    assert list(evaluate.metric_intervals(v[:, 0], replicates=4)) == ["column0"]
    # ratios: one shared denominator, and one per column
    den1 = np.random.default_rng(3).integers(1, 6, size=n).astype(np.float64)
    got = evaluate.metric_intervals(v, replicates=B, level=level, seed=seed, denominators=den1)
    want = {"column%d" % k: BC.direct_interval(s, value, level) for k, (value, s) in enumerate(_direct(v, den1[:, None], B, seed, level))}
    BC.same_fields(got, want, 1e-14, "shared denominator")
    den3 = np.random.default_rng(4).integers(1, 6, size=(n, 3)).astype(np.float64)
    got = evaluate.metric_intervals(v, replicates=B, level=level, seed=seed, denominators=den3)
    want = {"column%d" % k: BC.direct_interval(s, value, level) for k, (value, s) in enumerate(_direct(v, den3, B, seed, level))}
    BC.same_fields(got, want, 1e-14, "own denominators")


def test_metric_intervals_units_resample_whole_units():
    from digat_amd import evaluate
    rows, B, seed, level = 120, 48, 5, 0.8
    v = BC.integer_values(6, rows, 2)
    start = np.array([0, 0, 1, 1, 2, 30, 31, 90, 120, 120])             # empty units, single-row units, long ones
    units = evaluate.segment_sums_host(v, start)
    count = np.diff(start).astype(np.float64)
    got = evaluate.metric_intervals(v, replicates=B, level=level, seed=seed, units=start)
    want = {"column%d" % k: BC.direct_interval(s, value, level) for k, (value, s) in enumerate(_direct(units, count[:, None], B, seed, level))}
    BC.same_fields(got, want, 1e-14, "units")
    assert got["column0"]["value"] == pytest.approx(v[:, 0].mean(), rel=1e-14), "the statistic stays the mean over rows"
    den = np.random.default_rng(8).integers(1, 4, size=rows).astype(np.float64)
    got = evaluate.metric_intervals(v, replicates=B, level=level, seed=seed, units=start, denominators=den)
    dunits = evaluate.segment_sums_host(den, start)
    want = {"column%d" % k: BC.direct_interval(s, value, level) for k, (value, s) in enumerate(_direct(units, dunits, B, seed, level))}
    BC.same_fields(got, want, 1e-14, "units with denominators")


def test_compare_metrics_host_path_is_the_direct_computation_and_is_paired():
    from digat_amd import evaluate
    n, B, seed, level = 250, 80, 2, 0.95
    a, b = BC.real_values(7, n, 2), BC.real_values(8, n, 2)
    got = evaluate.compare_metrics(a, b, names=("u", "v"), replicates=B, level=level, seed=seed)
    da, db = _direct(a, None, B, seed, level), _direct(b, None, B, seed, level)          # the same draws for both: paired
    want = {name: BC.direct_paired(da[k][0], db[k][0], da[k][1] - db[k][1], level) for k, name in enumerate("uv")}
    BC.same_fields(got, want, 1e-13, "paired")
    # with denominators on both sides
    den = np.random.default_rng(9).integers(1, 5, size=n).astype(np.float64)
    got = evaluate.compare_metrics(a, b, replicates=B, level=level, seed=seed, denominators_a=den, denominators_b=den)
    da, db = _direct(a, den[:, None], B, seed, level), _direct(b, den[:, None], B, seed, level)
    want = {"column%d" % k: BC.direct_paired(da[k][0], db[k][0], da[k][1] - db[k][1], level) for k in range(2)}
    BC.same_fields(got, want, 1e-13, "paired ratios")
    same = evaluate.compare_metrics(a, a, replicates=B, seed=seed)["column0"]
    assert (same["diff"], same["lo"], same["hi"], same["se"], same["p"], same["wins"]) == (0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_a_planted_difference_is_found_and_a_null_one_is_not():
    """n = 2000, per-unit noise 0.05 between the two models, shift 0.01, seed 0: the standard error of the mean difference is
    0.05 / sqrt(2000) = 0.0011, so the shift stands nine of them from 0 and the null difference within two.  Host twin: shift interval
    [0.0076, 0.0120], p = 0.001; null (two independent noises) interval [-0.0046, 0.0017], p = 0.36."""
    from digat_amd import evaluate
    rng = np.random.default_rng(0)
    n = 2000
    base, noise = rng.standard_normal((n, 1)), 0.05 * rng.standard_normal((n, 1))
    shifted = evaluate.compare_metrics(base + 0.01 + noise, base, replicates=2000, seed=0)["column0"]
    null = evaluate.compare_metrics(base + noise, base + 0.05 * rng.standard_normal((n, 1)), replicates=2000, seed=0)["column0"]
    print(shifted, null)
    assert shifted["p"] < 0.01 and shifted["lo"] > 0.0 and shifted["lo"] < 0.01 + noise.mean() < shifted["hi"] and shifted["wins"] > 0.99
    assert null["lo"] < 0.0 < null["hi"] and null["p"] > 0.05
    own = evaluate.metric_intervals(base, replicates=2000, seed=0)["column0"]
    assert own["se"] > 10 * shifted["se"], "the unpaired spread of either model dwarfs the paired one: that is what pairing buys"


# ---------------------------------------------------------------------------------------------------------------------
# rank metrics
# ---------------------------------------------------------------------------------------------------------------------
def _rank_case(seed):
    rng = np.random.default_rng(seed)
    G, P = 23, 90
    scores = rng.standard_normal((G, P)).astype(np.float32)
    pos, start = R.make_targets(rng, G, P, per_user=(0, 1, 3, 0, 7), chunk=32)          # users without targets among them
    skip = rng.integers(0, P, size=(G, 6))                                              # skipped targets are not ranked
    return R.brute_ranks(scores, pos, start, skip=skip), start


@pytest.mark.parametrize("seed", (1, 2))
def test_rank_metric_columns_reproduce_rank_metrics(seed):
    from digat_amd import evaluate
    rank, start = _rank_case(seed)
    assert (rank < 0).any() and (np.diff(start) == 0).any()
    ks = (1, 10, 50)
    want = evaluate.rank_metrics(rank, start, ks)
    col = evaluate.rank_metric_columns(rank, start, ks)
    assert set(col) == {"targets", "has", "rr"} | {f"hits@{k}" for k in ks} | {f"share@{k}" for k in ks}
    assert all(v.shape == (len(start) - 1,) and v.dtype == np.float64 for v in col.values())
    assert col["has"].sum() == want["users"] and col["targets"].sum() == want["targets"]
    for k in ks:
        assert col[f"hits@{k}"].sum() / col["targets"].sum() == want[f"recall@{k}"]
        assert col[f"share@{k}"].sum() / col["has"].sum() == pytest.approx(want[f"user_recall@{k}"], rel=1e-14)
    assert col["rr"].sum() / col["has"].sum() == pytest.approx(want["mrr"], rel=1e-14)
    got = evaluate.rank_metrics_intervals(rank, start, ks, replicates=40, level=0.9, seed=3)
    assert set(got) == {"mrr"} | {f"recall@{k}" for k in ks} | {f"user_recall@{k}" for k in ks}, "median_rank and the counts get no interval"
    for name, f in got.items():
        assert f["value"] == pytest.approx(want[name], rel=1e-14) and f["lo"] <= f["hi"] and f["replicates"] == 40, name
    # the same draws as a direct computation over the users with a target
    keep = col["has"] > 0
    idx = evaluate.bootstrap_draws_host(int(keep.sum()), 40, 3)
    stats = [col["hits@10"][keep][i].sum() / col["targets"][keep][i].sum() for i in idx]
    assert got["recall@10"]["lo"] == pytest.approx(BC.quantile_linear(stats, 0.05), rel=1e-14)
    with pytest.raises(ValueError, match="ks"):
        evaluate.rank_metrics_intervals(rank, start, tuple(range(1, 9)), replicates=4)
    with pytest.raises(ValueError, match="at least one row"):
        evaluate.rank_metrics_intervals(np.zeros(0, dtype=np.int32), np.array([0, 0]), (10,), replicates=4)
    assert "median_rank" in evaluate.rank_metrics_intervals.__doc__


def test_nrms_retrieval_metrics_intervals_on_cpu_tensors():
    import dot_topk_common as D
    from digat_amd import evaluate, nrms
    m, dev = D.model("nrms"), R.dev_with_rows()
    plain = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4)
    again = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4, intervals=None)
    with_iv = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4, intervals=30, seed=2)
    assert list(plain) == list(again) and "intervals" not in plain and list(with_iv) == list(plain) + ["intervals"]
    for key in plain:
        assert np.array_equal(np.asarray(plain[key]), np.asarray(again[key]), equal_nan=True), key
        assert np.array_equal(np.asarray(plain[key]), np.asarray(with_iv[key]), equal_nan=True), key
    assert with_iv["intervals"] == evaluate.rank_metrics_intervals(plain["rank"], plain["target_start"], (5, 20), replicates=30, seed=2)


# ---------------------------------------------------------------------------------------------------------------------
# impression metrics on host scores
# ---------------------------------------------------------------------------------------------------------------------
def test_impression_metrics_are_what_scoring_averages():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    counts = rng.integers(2, 30, size=60)
    imp = np.repeat(np.arange(60), counts)
    scores = np.round(rng.standard_normal(len(imp)) * 4) / 4
    labels = np.zeros(len(imp), dtype=np.int64)
    for s, e in zip(np.r_[0, np.cumsum(counts)][:-1], np.cumsum(counts)):
        labels[s + rng.choice(e - s, size=rng.integers(1, e - s), replace=False)] = 1
    per = evaluate.impression_metrics(scores, imp, labels)
    assert per.shape == (60, 4) and per.dtype == np.float64 and np.isfinite(per).all()
    want = evaluate.scoring(labels, evaluate.impression_ranks(scores, imp), imp)
    assert tuple(float(np.mean(np.ascontiguousarray(per[:, k]))) for k in range(4)) == want, "scoring keeps its bits"
    assert np.array_equal(evaluate.impression_metrics(torch.from_numpy(scores), imp, labels), per)
    # the reference formulas on one impression, by hand: scores 3 > 2 > 1, the middle one clicked
    one = evaluate.impression_metrics(np.array([3.0, 2.0, 1.0]), np.zeros(3, dtype=np.int64), np.array([0, 1, 0]))
    assert one.shape == (1, 4) and one[0].tolist() == pytest.approx([0.5, 0.5, 1.0 / math.log2(3.0), 1.0 / math.log2(3.0)], rel=1e-15)
    # an impression without a negative has no AUC: metric_intervals names it
    bad = evaluate.impression_metrics(np.array([3.0, 2.0, 1.0, 5.0]), np.array([0, 0, 1, 1]), np.array([0, 1, 1, 1]))
    assert np.isfinite(bad[0]).all() and not np.isfinite(bad[1]).all()
    with pytest.raises(ValueError, match="row 1"):
        evaluate.metric_intervals(bad, names=evaluate.METRIC_NAMES, replicates=10)
    got = evaluate.metric_intervals(per, names=evaluate.METRIC_NAMES, replicates=50)
    assert list(got) == ["auc", "mrr", "ndcg5", "ndcg10"] and all(got[k]["value"] == pytest.approx(w, rel=1e-14) for k, w in zip(got, want))


def test_util_compare_models_on_cpu_scores():
    from digat_amd import evaluate, util
    import types
    rng = np.random.default_rng(6)
    imp = np.repeat(np.arange(40), 6)
    labels = np.tile(np.array([1, 0, 0, 1, 0, 0]), 40)
    sa, sb = rng.standard_normal(len(imp)).astype(np.float32), rng.standard_normal(len(imp)).astype(np.float32)
    dc = types.SimpleNamespace(row_impression=torch.from_numpy(imp))
    table = {"a": sa, "b": sb}
    score_fn = lambda model, dc, start, end, batch_size: torch.from_numpy(table[model.name][start:end])
    models = [types.SimpleNamespace(name=k, graph_encoder=None) for k in "ab"]
    got = util.compare_models(models[0], models[1], dc, labels, replicates=60, seed=1, batch_size=8, score_fn=score_fn)
    want = evaluate.compare_metrics(evaluate.impression_metrics(sa, imp, labels), evaluate.impression_metrics(sb, imp, labels),
                                    names=evaluate.METRIC_NAMES, replicates=60, seed=1)
    assert got == want and list(got) == ["auc", "mrr", "ndcg5", "ndcg10"]
    m = util.compute_scores(models[0], dc, 8, labels=labels, score_fn=score_fn)[1]
    assert tuple(got[k]["a"] for k in got) == pytest.approx(m, rel=1e-14)
    own = util.compare_models(models[0], models[0], dc, labels, replicates=20, score_fn=score_fn)["auc"]
    assert (own["diff"], own["lo"], own["hi"], own["p"]) == (0.0, 0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="labels"):
        util.compare_models(models[0], models[1], dc, None, score_fn=score_fn)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_python_entries_refuse_bad_arguments():
    from digat_amd import _lib, evaluate
    v = np.ones((5, 2))
    for call, match in ((lambda: evaluate.metric_intervals(np.ones((5, 17))), "values must have between 1 and BOOTSTRAP_MAX_COLUMNS = 16 columns"),
                        (lambda: evaluate.bootstrap_sums_host(np.ones((5, 17)), 3), "values .* columns"),
                        (lambda: evaluate.metric_intervals(np.ones((5, 9)), denominators=np.ones((5, 9))), "values .* columns"),
                        (lambda: evaluate.metric_intervals(np.ones((0, 2))), "values must have at least one row"),
                        (lambda: evaluate.bootstrap_draws_host(0, 3), "n = 0"),
                        (lambda: evaluate.metric_intervals(v, replicates=0), "replicates"),
                        (lambda: evaluate.bootstrap_draws_host(5, -1), "replicates"),
                        (lambda: evaluate.bootstrap_draws_host(5, 2.5), "replicates"),
                        (lambda: evaluate.bootstrap_draws_host(5, 2, first_replicate=-1), "first_replicate"),
                        (lambda: evaluate.bootstrap_draws_host(5, 3, first_replicate=(1 << 31) - 2), "first_replicate"),
                        (lambda: evaluate.metric_intervals(v, level=0.0), "level"),
                        (lambda: evaluate.metric_intervals(v, level=1.0), "level"),
                        (lambda: evaluate.compare_metrics(v, v, level=1.5), "level"),
                        (lambda: evaluate.metric_intervals(v, units=np.array([0, 3, 2, 5])), "start"),
                        (lambda: evaluate.metric_intervals(v, units=np.array([0, 4])), "start"),
                        (lambda: evaluate.metric_intervals(np.array([[1.0, 2.0], [np.nan, 1.0]])), "values must be finite: row 1"),
                        (lambda: evaluate.metric_intervals(np.array([1.0, 2.0, np.inf, np.nan])), "values must be finite: row 2"),
                        (lambda: evaluate.metric_intervals(v, denominators=np.array([1.0, 1.0, 1.0, -np.inf, 1.0])), "denominators must be finite: row 3"),
                        (lambda: evaluate.metric_intervals(v, denominators=np.ones(4)), "denominators must be"),
                        (lambda: evaluate.metric_intervals(v, denominators=np.ones((5, 3))), "denominators must be"),
                        (lambda: evaluate.metric_intervals(v, names=("one",)), "names"),
                        (lambda: evaluate.metric_intervals(np.ones((2, 2, 2))), "values must be"),
                        (lambda: evaluate.compare_metrics(v, np.ones((5, 3))), "values_a and values_b must have the same shape"),
                        (lambda: evaluate.compare_metrics(v, np.ones((4, 2))), "values_a and values_b must have the same shape"),
                        (lambda: evaluate.compare_metrics(np.ones((5, 9)), np.ones((5, 9))), "values_a and values_b .* 18 columns"),
                        (lambda: evaluate.compare_metrics(v, np.array([[1.0, 1.0]] * 4 + [[1.0, np.nan]])), "values_b must be finite: row 4")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(_lib.DigatHipError, match="GPU only"):
        evaluate.bootstrap_sums(torch.ones(5, 2), 3)
    with pytest.raises(_lib.DigatHipError, match="GPU only"):
        evaluate.segment_sums(torch.ones(5, 2), np.array([0, 5]))


def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == 4 == _lib.ABI_VERSION, "an addition: the ABI version stays"
    assert int(re.search(r"#define DIGAT_BOOTSTRAP_MAX_COLUMNS (\d+)", header).group(1)) == evaluate.BOOTSTRAP_MAX_COLUMNS == BC.MAX_COLUMNS
    assert int(re.search(r"#define DIGAT_BOOTSTRAP_SLICE (\d+)", header).group(1)) == evaluate.BOOTSTRAP_SLICE == BC.SLICE
    kernels = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert '#include "digat_bootstrap.inc"' in kernels
    source = open(os.path.join(REPO, "digat_amd", "csrc", "digat_bootstrap.inc")).read()
    assert "atomicAdd" not in source, "the determinism contract: no floating-point atomics"


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_double * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    ARG, SHAPE, WS = 1, 2, 3
    sums = lambda values=p, n=5, c=2, B=3, r0=0, out=p, ws=None, wsb=0: L.digat_bootstrap_sums(values, n, c, B, r0, 7, out, ws, wsb, None)
    assert sums(values=None) == ARG and sums(out=None) == ARG and sums(values=p + 4) == ARG and sums(out=p + 4) == ARG and sums(ws=p + 4) == ARG
    assert sums(n=0) == ARG and sums(n=-1) == ARG and sums(c=0) == ARG and sums(B=-1) == ARG and sums(r0=-1) == ARG
    assert sums(n=1 << 31) == SHAPE and sums(c=17) == SHAPE and sums(r0=(1 << 31) - 2) == SHAPE and sums(B=(1 << 31) + 1) == SHAPE
    assert sums(r0=(1 << 31) + 1, B=0) == SHAPE
    assert sums(n=BC.SLICE + 1) == WS and sums(n=BC.SLICE + 1, ws=p, wsb=2 * 2 * 3 * 8 - 1) == WS
    assert sums(B=0) == 0, "no replicates: nothing to launch"
    need = L.digat_bootstrap_workspace_bytes
    assert need(BC.SLICE, 16, 1000) == 0 and need(1, 1, 1) == 0, "one slice: the sums are written directly"
    assert need(BC.SLICE + 1, 2, 3) == 2 * 2 * 3 * 8 and need(73152, 4, 10000) == 9 * 4 * 10000 * 8
    assert need(0, 2, 3) == 0 and need(5, 17, 3) == 0 and need(5, 2, -1) == 0
    seg = lambda values=p, rows=4, c=2, start=p, units=2, out=p: L.digat_segment_sums_f64(values, rows, c, start, units, out, None)
    assert seg(values=None) == ARG and seg(start=None) == ARG and seg(out=None) == ARG and seg(rows=-1) == ARG and seg(c=0) == ARG
    assert seg(units=-1) == ARG and seg(values=p + 4) == ARG and seg(start=p + 4) == ARG and seg(out=p + 4) == ARG
    assert seg(c=(1 << 20) + 1) == SHAPE and seg(units=1 << 37, c=4) == SHAPE
    assert seg(units=0) == 0 and seg(values=None, rows=0, units=0) == 0
    assert b"argument" in L.digat_error_string(ARG)


def test_config_parses_the_bootstrap_flags():
    from digat_amd.config import Config
    c = Config(["--mode", "dev"])
    assert not hasattr(c, "bootstrap") and "compare_model_path" not in c.attribute_dict, "off: no attribute"
    c = Config(["--mode", "dev", "--bootstrap", "200"])
    assert (c.bootstrap, c.bootstrap_level, c.compare_model_path) == (200, 0.95, "")
    c = Config(["--mode", "test", "--bootstrap", "50", "--bootstrap_level", "0.9", "--compare_model_path", "other"])
    assert (c.bootstrap, c.bootstrap_level, c.compare_model_path) == (50, 0.9, "other")
    for bad in (["--bootstrap", "-1"], ["--bootstrap", "10", "--bootstrap_level", "1.0"], ["--compare_model_path", "other"]):
        with pytest.raises(SystemExit):
            Config(["--mode", "dev"] + bad)


def test_main_formats_one_line_per_metric():
    from digat_amd import main
    rng = np.random.default_rng(2)
    per = rng.random((50, 4))
    lines = main.interval_lines(per, 40, 0.9, 3)
    assert len(lines) == 4 and [line.split(" interval : ")[0] for line in lines] == ["AUC", "MRR", "nDCG@5", "nDCG@10"]
    assert all("40 bootstrap replicates over 50 impressions, level 0.9, seed 3" in line for line in lines)
    lines = main.compare_lines(per, per[::-1].copy(), 40, 0.9, 3)
    assert len(lines) == 4 and all(line.split(" difference : ")[0] in ("AUC", "MRR", "nDCG@5", "nDCG@10") and " p " in line and "seed 3" in line
                                   for line in lines)
