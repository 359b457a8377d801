"""GPU suite: the bootstrap resampling kernel (``digat_bootstrap_sums``), the unit sums (``digat_segment_sums_f64``) and what is built
on them.  The kernel is held to the host twin (``evaluate.bootstrap_sums_host``: the same draws, correctly rounded sums) — exactly
on integer data, within the bound of a double sum in any order on reals — and to its determinism contract by bits; the statistics to
the host path's dicts; the callers end to end."""
import shutil

import numpy as np
import pytest
import torch

import bootstrap_common as BC
import dot_rank_common as R
import dot_topk_common as D
import test_hip_diversify as TH
from mind_common import FIXTURE

pytestmark = pytest.mark.gpu

S = BC.SLICE
NS = (1, 2, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 3)
CS, BS = (1, 2, 3, 4, 8, 15, 16), (1, 2, 7, 65)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def grid_case(i, n):
    """The i-th n of the grid with the other axes rotating over their values: ``(c, B, seed, first_replicate)``."""
    return CS[i % 7], BS[(i + i // 4) % 4], 1000 + i, (0, 3, 1 << 20)[i % 3]


@pytest.mark.parametrize("i,n", list(enumerate(NS)))
def test_kernel_is_the_host_twin(i, n):
    from digat_amd import evaluate
    c, B, seed, r0 = grid_case(i, n)
    idx = evaluate.bootstrap_draws_host(n, B, seed, r0)
    ints = BC.integer_values(i, n, c)
    got = evaluate.bootstrap_sums(_t(ints), B, seed, r0)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, c) and got.is_cuda
    want = evaluate.bootstrap_sums_host(ints, B, seed, r0)
    assert np.array_equal(got.cpu().numpy(), want), "integer-valued data below 2^53: exact"
    assert np.array_equal(want, np.stack([ints[idx[b]].sum(axis=0) for b in range(B)]))
    reals = BC.real_values(i, n, c)
    got = evaluate.bootstrap_sums(_t(reals), B, seed, r0).cpu().numpy()
    want, bound = evaluate.bootstrap_sums_host(reals, B, seed, r0), BC.sum_bound(reals, idx)
    err = np.abs(got - want)
    print("n %d c %d B %d: worst error / bound %.3g" % (n, c, B, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (n, c, B, float(err.max()))


def test_every_axis_value_of_the_grid_is_met():
    cases = [grid_case(i, n) for i, n in enumerate(NS)]
    assert {c[0] for c in cases} == set(CS) and {c[1] for c in cases} == set(BS) and {c[3] for c in cases} == {0, 3, 1 << 20}
    assert S == 8192 and max(NS) > 2 * S, "one, two and three slices"


@pytest.mark.parametrize("n", (300, S + 5, 2 * S + 3))
def test_bit_identity(n):
    from digat_amd import evaluate
    B, B1, seed = 9, 4, 77
    a, b = BC.real_values(n, n, 4), BC.real_values(n + 1, n, 4)
    ab = _t(np.concatenate([a, b], axis=1))
    whole = evaluate.bootstrap_sums(ab, B, seed)
    assert _bits(evaluate.bootstrap_sums(ab, B, seed), whole), "the same call twice"
    split = torch.cat([evaluate.bootstrap_sums(ab, B1, seed), evaluate.bootstrap_sums(ab, B - B1, seed, first_replicate=B1)])
    assert _bits(split, whole), "split by first_replicate"
    apart = torch.cat([evaluate.bootstrap_sums(_t(a), B, seed), evaluate.bootstrap_sums(_t(b), B, seed)], dim=1)
    assert _bits(apart, whole), "[a | b] in one call against a and b apart"
    for k in (0, 5):                                                  # an odd column count takes the 8-byte loads, one column alone too
        assert _bits(evaluate.bootstrap_sums(ab[:, k], B, seed), whole[:, k:k + 1]), k
    assert _bits(evaluate.bootstrap_sums(ab[:, 1:4], B, seed), whole[:, 1:4]), "three columns"
    # a float32 or strided input against its float64 contiguous copy
    f32 = ab.to(torch.float32)
    assert _bits(evaluate.bootstrap_sums(f32, B, seed), evaluate.bootstrap_sums(f32.to(torch.float64), B, seed)), "float32"
    wide = torch.zeros((n, 19), dtype=torch.float64, device=_dev())
    wide[:, 1:17:2] = ab
    assert _bits(evaluate.bootstrap_sums(wide[:, 1:17:2], B, seed), whole), "strided"
    assert _bits(evaluate.bootstrap_sums(ab.t().contiguous().t(), B, seed), whole), "column-major"
    # a table at an address that is 8 but not 16 bytes aligned: the narrow loads, the same bits
    odd = torch.empty(n * 8 + 1, dtype=torch.float64, device=_dev())[1:].view(n, 8)
    odd.copy_(ab)
    assert odd.data_ptr() % 16 == 8 and _bits(evaluate.bootstrap_sums(odd, B, seed), whole), "8-byte-aligned table"
    assert not _bits(evaluate.bootstrap_sums(ab, B, seed + 1), whole)


def test_counter_edges():
    from digat_amd import evaluate
    n, B = 7, 6
    v = BC.integer_values(3, n, 3)
    r0 = (1 << 32) // n - 2                                         # the counters r n + j cross 2^32 inside these replicates
    assert r0 * n < (1 << 32) < (r0 + B) * n
    assert np.array_equal(evaluate.bootstrap_sums(_t(v), B, 5, r0).cpu().numpy(), evaluate.bootstrap_sums_host(v, B, 5, r0))
    top = (1 << 31) - B                                             # the upper limit: first_replicate + replicates = 2^31
    assert np.array_equal(evaluate.bootstrap_sums(_t(v), B, 5, top).cpu().numpy(), evaluate.bootstrap_sums_host(v, B, 5, top))
    n = S + 1                                                       # two slices at the top: counters near 2^44
    v = BC.integer_values(4, n, 2)
    assert np.array_equal(evaluate.bootstrap_sums(_t(v), 2, 5, (1 << 31) - 2).cpu().numpy(), evaluate.bootstrap_sums_host(v, 2, 5, (1 << 31) - 2))
    with pytest.raises(ValueError, match="first_replicate"):
        evaluate.bootstrap_sums(_t(v), B, 5, top + 1)


def test_guards():
    from digat_amd import _lib, evaluate
    n, c, B, seed = S + 9, 5, 7, 3
    v = BC.real_values(8, n, c)
    V = _t(v)
    want = evaluate.bootstrap_sums(V, B, seed)
    # a workspace full of NaN bytes changes nothing
    _lib.workspace(0, _dev(), "bootstrap").fill_(0xFF)
    assert _bits(evaluate.bootstrap_sums(V, B, seed), want), "poisoned workspace"
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = evaluate.bootstrap_sums(V, B, seed)
    side.synchronize()
    assert _bits(on_side, want), "side stream"
    # the raw entry: guard regions on both sides of the output and of an exactly sized workspace; the input is read only
    L, pad = _lib.lib(), 64
    need = int(L.digat_bootstrap_workspace_bytes(n, c, B))
    assert need == 2 * c * B * 8
    out = torch.full((pad + B * c + pad,), 55.0, dtype=torch.float64, device=_dev())
    ws = torch.full((pad + need // 8 + pad,), 66.0, dtype=torch.float64, device=_dev())
    keep = V.clone()
    _lib.check(L.digat_bootstrap_sums(V.data_ptr(), n, c, B, 0, seed, out[pad:].data_ptr(), ws[pad:].data_ptr(), need, _lib.stream_ptr()),
               "digat_bootstrap_sums")
    torch.cuda.synchronize()
    assert (out[:pad] == 55).all() and (out[pad + B * c:] == 55).all() and (ws[:pad] == 66).all() and (ws[pad + need // 8:] == 66).all()
    assert _bits(out[pad:pad + B * c].view(B, c), want) and _bits(V, keep)
    # a call the wrapper splits by replicates (its slice partials would pass the cap) gives the same bits
    cap, evaluate._BOOTSTRAP_WORKSPACE = evaluate._BOOTSTRAP_WORKSPACE, 3 * 2 * c * 8
    try:
        assert _bits(evaluate.bootstrap_sums(V, B, seed), want), "three replicates per call"
    finally:
        evaluate._BOOTSTRAP_WORKSPACE = cap
    with pytest.raises(ValueError, match="columns"):
        evaluate.bootstrap_sums(torch.zeros((4, 17), device=_dev()), 3)
    with pytest.raises(ValueError, match="at least one row"):
        evaluate.bootstrap_sums(torch.zeros((0, 2), device=_dev()), 3)
    with pytest.raises(ValueError, match="replicates"):
        evaluate.bootstrap_sums(V, 0)


@pytest.mark.parametrize("name,rows,c,start", [("empty units", 50, 3, (0, 0, 1, 1, 20, 50, 50)), ("U = 1", 9, 2, (0, 9)), ("one long unit", 5000, 1, (0, 5000)),
                                               ("16 columns", 700, 16, tuple(range(0, 701, 7))), ("no rows", 0, 2, (0, 0, 0))])
def test_segment_sums_are_bit_exact_to_the_host_twin(name, rows, c, start):
    from digat_amd import evaluate
    v = BC.real_values(len(name), rows, c)
    got = evaluate.segment_sums(_t(v), np.asarray(start))
    want = evaluate.segment_sums_host(v, np.asarray(start))
    assert tuple(got.shape) == (len(start) - 1, c) and np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)), name
    assert _bits(evaluate.segment_sums(_t(v.astype(np.float32)), torch.tensor(start)), evaluate.segment_sums(_t(v.astype(np.float32).astype(np.float64)), start))
    with pytest.raises(ValueError, match="start"):
        evaluate.segment_sums(_t(v), np.asarray(start) + 1)


def _ranking_case(seed, impressions, max_c, quant):
    """The generator of test_hip_parity.test_device_ranks_and_metrics_match_host."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(2, max_c + 1, size=impressions)
    imp = np.repeat(np.arange(impressions), counts)
    scores = rng.standard_normal(len(imp)).astype(np.float32)
    if quant:
        scores = np.round(scores * quant) / quant
    labels = np.zeros(len(imp), dtype=np.int64)
    starts = np.r_[0, np.cumsum(counts)]
    for s, e in zip(starts[:-1], starts[1:]):
        k = rng.integers(1, max(2, min(4, e - s)))
        labels[s + rng.choice(e - s, size=min(k, e - s - 1), replace=False)] = 1
    return scores, imp, labels


@pytest.mark.parametrize("seed,impressions,max_c,quant", [(1, 300, 40, 0), (2, 50, 300, 8), (3, 1, 2, 0), (4, 2000, 60, 4)])
def test_impression_metrics_on_the_device(seed, impressions, max_c, quant):
    """Per impression against the host values: the AUC is integer arithmetic until its one division — the same bits —, the other
    three are sums of at most 10 terms 1 / log2(r + 1) over such a sum, every term within a few ulp on either side (log2, a
    division, an addition): 64 half-ulps.  The column means against ``device_ranks_and_metrics``' own: two double sums of I terms in
    different orders, each within I 2^-54 relative of the exact sum of these non-negative terms."""
    from digat_amd import evaluate
    scores, imp, labels = _ranking_case(seed, impressions, max_c, quant)
    per = evaluate.impression_metrics(_t(scores), imp, labels)
    assert per.is_cuda and per.dtype == torch.float64 and tuple(per.shape) == (impressions, 4)
    got = per.cpu().numpy()
    want = evaluate.impression_metrics(scores, imp, labels)
    assert np.array_equal(got[:, 0], want[:, 0]), "AUC"
    assert (np.abs(got[:, 1:] - want[:, 1:]) <= 64 * 2.0 ** -53 * np.abs(want[:, 1:])).all()
    _, mean = evaluate.device_ranks_and_metrics(_t(scores), imp, labels)
    mine = got.sum(axis=0) / impressions
    assert (np.abs(mine - np.asarray(mean)) <= impressions * 2.0 ** -53 * np.abs(mean)).all(), (mine, mean)


def test_statistics_on_the_device_are_the_host_paths():
    from digat_amd import evaluate
    n, B, seed = 700, 120, 6
    # integer-valued columns: field for field
    a, b = BC.integer_values(1, n, 3), BC.integer_values(2, n, 3)
    den = np.random.default_rng(3).integers(1, 9, size=n).astype(np.float64)
    start = np.r_[0, np.sort(np.random.default_rng(4).integers(0, n + 1, size=40)), n]
    for kw in ({}, {"denominators": den}, {"units": start}, {"units": start, "denominators": den}):
        host = evaluate.metric_intervals(a, names="xyz", replicates=B, seed=seed, level=0.9, **kw)
        dev = evaluate.metric_intervals(_t(a), names="xyz", replicates=B, seed=seed, level=0.9,
                                        **{k: (_t(v) if k == "denominators" else v) for k, v in kw.items()})
        BC.same_fields(dev, host, 0, str(sorted(kw)))
    host = evaluate.compare_metrics(a, b, replicates=B, seed=seed, denominators_a=den, denominators_b=den)
    BC.same_fields(evaluate.compare_metrics(_t(a), _t(b), replicates=B, seed=seed, denominators_a=_t(den), denominators_b=den), host, 0, "paired")
    BC.same_fields(evaluate.compare_metrics(_t(a), _t(b), replicates=B, seed=seed, units=start),
                   evaluate.compare_metrics(a, b, replicates=B, seed=seed, units=start), 0, "paired units")
    # real columns: every replicate statistic is off by at most bound / denominator (integer denominators are exact); a quantile is a
    # convex combination of order statistics and moves by no more than the largest such error, the standard deviation by no more
    # than sqrt(B / (B - 1)) of it, the value by the bound of the full sum: twice the largest error covers each
    ra, rb = np.abs(BC.real_values(5, n, 2)) + 1.0, np.abs(BC.real_values(6, n, 2)) + 1.0
    idx = evaluate.bootstrap_draws_host(n, B, seed)
    for den_k in (None, den):
        low = n if den_k is None else float(den_k[idx].sum(axis=1).min())
        tol = {k: 2.0 * max(float(BC.sum_bound(ra, idx)[:, k].max()), n * 2.0 ** -53 * float(ra[:, k].sum())) / low for k in range(2)}
        tol_b = {k: 2.0 * max(float(BC.sum_bound(rb, idx)[:, k].max()), n * 2.0 ** -53 * float(rb[:, k].sum())) / low for k in range(2)}
        host = evaluate.metric_intervals(ra, replicates=B, seed=seed, denominators=den_k)
        dev = evaluate.metric_intervals(_t(ra), replicates=B, seed=seed, denominators=_t(den_k))
        for k, name in enumerate(host):
            for f in ("value", "lo", "hi", "se"):
                assert abs(dev[name][f] - host[name][f]) <= tol[k], (name, f)
            assert dev[name]["replicates"] == B and dev[name]["level"] == 0.95
        host = evaluate.compare_metrics(ra, rb, replicates=B, seed=seed, denominators_a=den_k, denominators_b=den_k)
        dev = evaluate.compare_metrics(_t(ra), _t(rb), replicates=B, seed=seed, denominators_a=_t(den_k), denominators_b=_t(den_k))
        for k, name in enumerate(host):
            for f, t in (("a", tol[k]), ("b", tol_b[k]), ("diff", tol[k] + tol_b[k]), ("lo", tol[k] + tol_b[k]), ("hi", tol[k] + tol_b[k]),
                         ("se", tol[k] + tol_b[k])):
                assert abs(dev[name][f] - host[name][f]) <= t, (name, f)


def test_rank_metrics_intervals_on_the_device_are_the_host_paths():
    from digat_amd import evaluate
    rng = np.random.default_rng(1)
    G, P = 40, 90
    pos, start = R.make_targets(rng, G, P, per_user=(0, 1, 3, 0, 7), chunk=32)
    rank = R.brute_ranks(rng.standard_normal((G, P)).astype(np.float32), pos, start, skip=rng.integers(0, P, size=(G, 6)))
    host = evaluate.rank_metrics_intervals(rank, start, (1, 10, 50), replicates=100, seed=2)
    dev = evaluate.rank_metrics_intervals(rank, start, (1, 10, 50), replicates=100, seed=2, device=_dev())
    # hits and targets are integers (exact); shares and reciprocal ranks are reals: the means of at most 40 of them
    for name in host:
        for f in ("value", "lo", "hi", "se"):
            assert dev[name][f] == host[name][f] if name.startswith("recall@") else abs(dev[name][f] - host[name][f]) <= 2 * 40 * 2.0 ** -53, (name, f)


def test_util_compare_models_end_to_end():
    from digat_amd import evaluate, util
    spec, corpus, _ = TH._corpus()
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    model = TH._model()
    labels = corpus.row_label
    own = util.compare_models(model, model, dc, labels, replicates=100, batch_size=256)
    assert list(own) == ["auc", "mrr", "ndcg5", "ndcg10"]
    for f in own.values():
        assert f["diff"] == 0.0 and f["lo"] == 0.0 and f["hi"] == 0.0 and f["p"] == 1.0 and f["a"] == f["b"]
    other = TH._model()
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for p in other.graph_encoder.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    got = util.compare_models(model, other, dc, labels, replicates=100, seed=3, batch_size=256)
    I = int(np.unique(corpus.row_impression).size)
    for side, m in (("a", model), ("b", other)):
        metrics = util.compute_scores(m, dc, 256, labels=labels)[1]
        for k, want in zip(got, metrics):
            assert abs(got[k][side] - want) <= I * 2.0 ** -53 * abs(want), (side, k)
    for f in got.values():
        assert all(np.isfinite(v) for v in f.values()) and f["lo"] <= f["hi"] and f["diff"] == f["a"] - f["b"] and 0.0 < f["p"] <= 1.0


def test_nrms_retrieval_metrics_without_intervals_is_todays_dict():
    from digat_amd import evaluate, nrms
    m, dev = D.model("nrms", _dev()), R.dev_with_rows(_dev())
    plain = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4)
    none = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4, intervals=None)
    want = evaluate.rank_metrics(plain["rank"], plain["target_start"], (5, 20))
    assert list(plain) == list(none) == list(want) + ["rank", "target_start", "target_ids"]
    assert all(np.array_equal(np.asarray(plain[k]), np.asarray(none[k]), equal_nan=True) for k in plain)
    assert all(np.array_equal(np.asarray(plain[k]), np.asarray(want[k]), equal_nan=True) for k in want)
    with_iv = nrms.retrieval_metrics(m, dev, ks=(5, 20), batch_size=4, intervals=50, seed=1)
    assert list(with_iv) == list(plain) + ["intervals"] and all(np.array_equal(np.asarray(plain[k]), np.asarray(with_iv[k]), equal_nan=True) for k in plain)
    host = evaluate.rank_metrics_intervals(plain["rank"], plain["target_start"], (5, 20), replicates=50, seed=1)
    assert list(with_iv["intervals"]) == list(host)
    for name in host:
        assert with_iv["intervals"][name] == pytest.approx(host[name], rel=1e-13, abs=1e-15, nan_ok=True), name


def test_main_dev_prints_the_interval_lines_below_todays_four(tmp_path, capsys):
    from digat_amd.main import main
    from test_hip_mind import SMALL
    root, models = tmp_path / "data", tmp_path / "models"
    shutil.copytree(FIXTURE, root)
    common = ["--data_root", str(root), "--news_encoder", "MSA", "--data_cache", str(tmp_path / "cache")] + SMALL
    main(["--mode", "train", "--max_steps", "1", "--model_dir", str(models)] + common)
    capsys.readouterr()
    main(["--mode", "dev", "--dev_model_path", str(models / "MSA-DIGAT")] + common)
    before = capsys.readouterr().out.splitlines()
    main(["--mode", "dev", "--dev_model_path", str(models / "MSA-DIGAT"), "--bootstrap", "200", "--compare_model_path", str(models / "MSA-DIGAT")] + common)
    after = capsys.readouterr().out.splitlines()
    four = [line for line in before if line.split(" : ")[0] in ("AUC", "MRR", "nDCG@5", "nDCG@10")]
    assert len(four) == 4 and not any("interval" in line or "difference" in line for line in before)
    at = after.index(four[0])
    assert after[at:at + 4] == four, "today's four lines, character for character"
    assert after[at + 4].startswith("Inference time")
    intervals = after[at + 5:at + 9]
    for line, name, mean in zip(intervals, ("AUC", "MRR", "nDCG@5", "nDCG@10"), four):
        assert line.startswith(name + " interval : [") and "(200 bootstrap replicates over" in line and "level 0.95, seed 0)" in line, line
        lo, hi = (float(v) for v in line.split("[")[1].split("]")[0].split(", "))
        assert lo <= float(mean.split(" : ")[1]) <= hi, line
    compared = after[at + 9:]
    assert len(compared) == 4 and all(line.startswith(name + " difference : ") and "= +0.0000  [+0.0000, +0.0000]" in line and "p 1.0000" in line
                                      for line, name in zip(compared, ("AUC", "MRR", "nDCG@5", "nDCG@10"))), compared
