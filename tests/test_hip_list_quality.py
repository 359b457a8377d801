"""GPU suite: the list-quality kernel (``digat_list_quality``) and the diversity sweep on it (``recommend_report``).  The kernel is
held to the host contract (``evaluate.list_quality_host``) on the similarities ``digat_dot_scores`` gives for the same rows — every
integer exactly, ``sim_max`` by bits, ``sim_sum`` within the bound of a double sum in any order — and on integer data to numpy
integer arithmetic alone, ``sim_sum`` included."""
import os
import shutil

import numpy as np
import pytest
import torch

import diversify_common as V
import dot_rank_common as R
import dot_topk_common as D
import list_quality_common as Q
import test_hip_diversify as TH
from mind_common import FIXTURE

pytestmark = pytest.mark.gpu

KS, DS, GS, KBS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128), (1, 20, 100, 400), (1, 3, 65), (1, 16, 65, 128)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def grid_case(n, k):
    """The n-th list length of the grid with the other axes rotating over their values: ``(G, d, N, kb, category?, exposure?)``."""
    G, d, N = (GS[n % 3] if k != 128 else 65), DS[(n + n // 4) % 4], (4096 if n % 2 else 300)
    return G, d, N, KBS[n % 4], n % 2 == 0, n % 3 != 1


def float_case(seed, G, k, kb, N, d):
    """``test_hip_diversify.float_case``'s rows (exact copies among them, a zero row) and lists, and a base list that shares about
    half its leading ids with the list."""
    vec, ids, count, _, _ = TH.float_case(seed, G, k, N, d)
    rng = np.random.default_rng(1000 + seed)
    base, base_count = V.make_lists(rng, G, kb, N)
    m = min(k, kb)
    base[:, :m] = np.where(rng.random((G, m)) < 0.5, ids[:, :m], base[:, :m])
    category = (rng.integers(-4, 12, size=N) * 1000003).astype(np.int32)       # arbitrary int32 values, few enough to repeat in a list
    exposure = rng.integers(0, 3, size=N).astype(np.int32)
    return vec, ids, count, base, base_count, category, exposure


@pytest.mark.parametrize("n,k", list(enumerate(KS)))
def test_kernel_is_the_host_contract_on_the_devices_own_similarities(n, k):
    from digat_amd import evaluate
    G, d, N, kb, with_cat, with_exp = grid_case(n, k)
    vec, ids, count, base, base_count, category, exposure = float_case(n, G, k, kb, N, d)
    VEC, IDS, CNT = _t(vec), _t(ids), _t(count)
    sim = TH.device_gram(IDS, VEC)
    EXP = _t(exposure) if with_exp else None
    got = evaluate.list_quality(IDS, CNT, VEC, _t(category) if with_cat else None, _t(base), _t(base_count), EXP)
    want = evaluate.list_quality_host(ids, count, sim, category if with_cat else None, base, base_count, news_num=N,
                                      exposure=exposure if with_exp else None)
    assert ("exposure" in got) == with_exp and ("categories" in got) == with_cat and (not with_exp or got["exposure"] is EXP)
    Q.same(got, want, Q.sum_bound(ids, count, sim, N), (G, k, d, kb))
    # count=None is k, base_count=None is kb
    got = evaluate.list_quality(IDS, None, VEC, base_ids=_t(base))
    Q.same(got, evaluate.list_quality_host(ids, None, sim, base_ids=base, news_num=N), Q.sum_bound(ids, None, sim, N), "counts None")


def test_every_axis_value_of_the_grid_is_met():
    cases = [grid_case(n, k) for n, k in enumerate(KS)]
    assert {c[0] for c in cases} == set(GS) and {c[1] for c in cases} == set(DS) and {c[3] for c in cases} == set(KBS)
    assert {c[4] for c in cases} == {True, False} and {c[5] for c in cases} == {True, False}
    assert {(c[4], c[5]) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}


def test_kernel_is_numpy_integer_arithmetic_on_integer_data():
    """Integers in [-2, 2], d = 20: every similarity and every partial sum is an integer far below 2^24 — no device Gram on the
    expected side, and ``sim_sum`` is exact whatever the order."""
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    G, k, kb, N, d = 5, 128, 65, 700, 20
    vec = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    ids, count = V.make_lists(rng, G, k, N)
    base, base_count = V.make_lists(rng, G, kb, N)
    base[:, :40] = ids[:, 5:45]
    category = rng.integers(0, 60, size=N).astype(np.int32)
    exposure = np.zeros(N, dtype=np.int32)
    safe = np.where((ids >= 0) & (ids < N), ids, 0)
    rows = vec[safe].astype(np.int64)
    sim = np.einsum("gid,gjd->gij", rows, rows).astype(np.float32)
    EXP = _t(exposure)
    got = evaluate.list_quality(_t(ids), _t(count), _t(vec), _t(category), _t(base), _t(base_count), EXP)
    want = evaluate.list_quality_host(ids, count, sim, category, base, base_count, news_num=N, exposure=exposure)
    Q.same(got, want, None, "integers")
    for g in range(G):
        el = Q.elements_of(ids[g], count[g], N)
        gram = rows[g][el] @ rows[g][el].T                            # int64
        assert float(got["sim_sum"][g]) == float(np.triu(gram, 1).sum()), g
    g = 0
    mine = Q.brute_force(ids[g], count[g], N, sim[g], category, base[g], base_count[g])
    assert {key: (float if key.startswith("sim") else int)(got[key][g]) for key in mine} == mine


def test_a_lists_outputs_do_not_depend_on_the_batch():
    from digat_amd import evaluate
    G, k, kb, N, d = 65, 128, 65, 2000, 100
    vec, ids, count, base, base_count, category, _ = float_case(21, G, k, kb, N, d)
    VEC, CAT = _t(vec), _t(category)
    whole_exp = torch.zeros(N, dtype=torch.int32, device=_dev())
    whole = evaluate.list_quality(_t(ids), _t(count), VEC, CAT, _t(base), _t(base_count), whole_exp)
    again = evaluate.list_quality(_t(ids), _t(count), VEC, CAT, _t(base), _t(base_count))
    assert all(torch.equal(whole[key].view(torch.uint8), again[key].view(torch.uint8)) for key in again), "run to run"
    for g in (0, 1, 2, 31, 64):
        one = evaluate.list_quality(_t(ids[g:g + 1]), _t(count[g:g + 1]), VEC, CAT, _t(base[g:g + 1]), _t(base_count[g:g + 1]))
        Q.same(one, {key: whole[key][g:g + 1] for key in one}, None, g)              # sim_sum by bits
    halves = torch.zeros(N, dtype=torch.int32, device=_dev())
    for a, b in ((0, 30), (30, G)):
        evaluate.list_quality(_t(ids[a:b]), _t(count[a:b]), exposure=halves)
    assert torch.equal(halves, whole_exp) and int(whole_exp.sum()) == int(whole["elements"].sum())


def test_exposure_under_contention():
    from digat_amd import evaluate
    N = 1000
    exposure = torch.zeros(N, dtype=torch.int32, device=_dev())
    got = evaluate.list_quality(torch.full((65, 128), 777, dtype=torch.int64, device=_dev()), exposure=exposure)
    assert int(exposure[777]) == 65 * 128 and int(exposure.sum()) == 65 * 128 and (got["elements"] == 128).all()
    assert set(got) == {"elements", "exposure"}


def test_without_vectors_the_integer_outputs_are_unchanged():
    from digat_amd import evaluate
    G, k, kb, N, d = 3, 65, 16, 500, 20
    vec, ids, count, base, base_count, category, exposure = float_case(4, G, k, kb, N, d)
    a, b = _t(exposure), _t(exposure)
    full = evaluate.list_quality(_t(ids), _t(count), _t(vec), _t(category), _t(base), _t(base_count), a)
    bare = evaluate.list_quality(_t(ids), _t(count), None, _t(category), _t(base), _t(base_count), b)
    assert set(full) - set(bare) == {"sim_sum", "sim_max"} and set(bare) <= set(full)
    Q.same(bare, {key: full[key] for key in bare}, None, "vectors=None")


def test_guards():
    from digat_amd import _lib, evaluate
    G, k, kb, N, d = 3, 65, 16, 500, 20
    vec, ids, count, base, base_count, category, exposure = float_case(9, G, k, kb, N, d)
    VEC, IDS, CNT, CAT, BASE, BCNT = _t(vec), _t(ids), _t(count), _t(category), _t(base), _t(base_count)
    call = lambda: evaluate.list_quality(IDS, CNT, VEC, CAT, BASE, BCNT, _t(exposure))
    want = {key: value.cpu().numpy() for key, value in call().items()}
    assert want["elements"][1] == 0 and want["sim_sum"][1] == 0.0 and np.isneginf(want["sim_max"][1]) and want["categories"][1] == 0, "an empty list"
    # a workspace full of NaN bytes changes nothing
    ws = _lib.workspace(0, _dev(), "list_quality")
    ws.fill_(0xFF)
    Q.same(call(), want, None, "poisoned workspace")
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = call()
    side.synchronize()
    Q.same(on_side, want, None, "side stream")
    # outputs full of garbage, guard regions on both sides of each: every output byte is written, nothing else is
    L, pad = _lib.lib(), 64
    raw = {key: torch.full((pad + G + pad,), 55, dtype=dtype, device=_dev())
           for key, dtype in (("elements", torch.int32), ("sim_sum", torch.float64), ("sim_max", torch.float32), ("categories", torch.int32),
                              ("category_max", torch.int32), ("overlap", torch.int32))}
    EXP = torch.full((pad + N + pad,), 7, dtype=torch.int32, device=_dev())
    EXP[pad:pad + N] = _t(exposure)
    inputs = [t.clone() for t in (IDS, CNT, VEC, CAT, BASE, BCNT)]
    _lib.check(L.digat_list_quality(IDS.data_ptr(), CNT.data_ptr(), G, k, N, VEC.data_ptr(), d, CAT.data_ptr(), BASE.data_ptr(), BCNT.data_ptr(), kb,
                                    EXP[pad:].data_ptr(), *(raw[key][pad:].data_ptr() for key in raw), None, 0, _lib.stream_ptr()),
               "digat_list_quality")
    torch.cuda.synchronize()
    for key, t in raw.items():
        assert (t[:pad] == 55).all() and (t[pad + G:] == 55).all(), key
    assert (EXP[:pad] == 7).all() and (EXP[pad + N:] == 7).all()
    Q.same({**{key: t[pad:pad + G] for key, t in raw.items()}, "exposure": EXP[pad:pad + N]}, want, None, "raw call")
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (IDS, CNT, VEC, CAT, BASE, BCNT))), "inputs are read only"
    # nobody
    nobody = evaluate.list_quality(IDS[:0], CNT[:0], VEC, CAT, BASE[:0], BCNT[:0], _t(exposure))
    assert all(tuple(nobody[key].shape) == (0,) for key in raw) and torch.equal(nobody["exposure"], _t(exposure))
    # refusals of the Python entry
    with pytest.raises(ValueError, match=r"\[G, k\]"):
        evaluate.list_quality(torch.zeros((3, 129), dtype=torch.int64, device=_dev()), vectors=VEC)
    with pytest.raises(ValueError, match="one entry per list"):
        evaluate.list_quality(IDS, CNT[:2], VEC)
    with pytest.raises(ValueError, match="base_count needs base_ids"):
        evaluate.list_quality(IDS, CNT, VEC, base_count=BCNT)
    with pytest.raises(ValueError, match=r"\[G, kb\]"):
        evaluate.list_quality(IDS, CNT, VEC, base_ids=BASE[:2])
    with pytest.raises(ValueError, match="all of one N"):
        evaluate.list_quality(IDS, CNT, VEC, CAT[:5])
    with pytest.raises(ValueError, match="int32"):
        evaluate.list_quality(IDS, CNT, VEC, exposure=torch.zeros(N, dtype=torch.int64, device=_dev()))
    with pytest.raises(ValueError, match="how many news"):
        evaluate.list_quality(IDS, CNT, base_ids=BASE)
    with pytest.raises(ValueError, match="d >= 1"):
        evaluate.list_quality(IDS, CNT, VEC[:, :0])


# ---------------------------------------------------------------------------------------------------------------------
# recommend_report end to end
# ---------------------------------------------------------------------------------------------------------------------
def _host_row(f, lists, short, unit, category, N, k, pool):
    """The report's row for one diversity, restated on the host from the lists: ``quality_summary(list_quality_host(...))`` on the
    device's own Gram."""
    from digat_amd import evaluate
    ids, _, count = lists
    q = evaluate.list_quality_host(ids.cpu().numpy(), count.cpu().numpy(), TH.device_gram(ids, unit), category, short[0][:, :k].cpu().numpy(),
                                   torch.clamp(short[2], max=k).cpu().numpy(), N, np.zeros(N, dtype=np.int32))
    return q, {"diversity": f, **evaluate.quality_summary(q, pool=pool)}


def test_digat_recommend_report_end_to_end(monkeypatch):
    from digat_amd import util
    spec, corpus, _ = TH._corpus()
    model, dc = TH._model(), util.DeviceCorpus.from_numpy(corpus, _dev())
    users, pool, k, N = np.arange(6), np.arange(1, spec.news_num, dtype=np.int64), 10, spec.news_num
    calls, inner = [], util.score_rows
    monkeypatch.setattr(util, "score_rows", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    short = util.recommend(model, dc, users, pool, 40, batch_size=256)
    one_recommend = len(calls)
    unit = util.unit_rows(dc.news_embedding)
    for q_cap in (0, 2):
        del calls[:]
        rows, lists = util.recommend_report(model, dc, users, pool, k, (0.0, 0.3), max_per_category=q_cap, batch_size=256, return_lists=True)
        assert len(calls) == one_recommend, "the scoring callable ran once for both diversities"
        for f, row, got in zip((0.0, 0.3), rows, lists):
            want = util.recommend(model, dc, users, pool, k, batch_size=256, diversity=f, max_per_category=q_cap)
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want)), (q_cap, f)
            q, want_row = _host_row(f, got, short, unit, corpus.news_category, N, k, pool)
            assert list(row) == list(want_row) and row == pytest.approx(want_row, rel=1e-12, abs=1e-12, nan_ok=True), (q_cap, f)
            if q_cap == 0 and f == 0.0:
                assert np.array_equal(q["overlap"], q["elements"]) and np.array_equal(q["elements"], got[2].cpu().numpy())
            if q_cap:
                assert (q["category_max"] <= 2).all()


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_report_end_to_end(pre):
    from digat_amd import evaluate, nrms, util
    m, dev = D.model(pre, _dev()), R.dev_with_rows(_dev())
    users, k = np.arange(D.USERS), 5
    _, target_ids, target_start = nrms._clicked_targets(dev, users)
    with torch.no_grad():
        cache, _ = nrms.news_caches(m, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask)
    short = nrms.recommend(m, dev, users, k=20, batch_size=4)
    rows, lists = nrms.recommend_report(m, dev, users, k=k, diversities=(0.0, 0.3), targets=(target_ids, target_start), batch_size=4,
                                        return_lists=True)
    for f, row, got in zip((0.0, 0.3), rows, lists):
        want = nrms.recommend(m, dev, users, k=k, batch_size=4, diversity=f)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want)), (pre, f)
        metrics = evaluate.rank_metrics(evaluate.list_ranks(want[0], want[2], target_ids, target_start), target_start, ks=(k,))
        assert {name: row[name] for name in ("recall@5", "user_recall@5", "mrr")} == {name: metrics[name] for name in ("recall@5", "user_recall@5", "mrr")}
        _, want_row = _host_row(f, got, short, util.unit_rows(cache), None, D.NEWS, k, np.arange(1, D.NEWS))
        quality = {name: row[name] for name in want_row}
        assert quality == pytest.approx(want_row, rel=1e-12, abs=1e-12, nan_ok=True), (pre, f)
        assert np.isnan(row["categories"]) and 0.0 <= row["ild"] <= 2.0 and row["lists"] == D.USERS


def test_main_prints_one_row_per_diversity_on_the_fixture(tmp_path, capsys):
    from digat_amd.main import main
    from test_hip_mind import SMALL
    root, models = tmp_path / "data", tmp_path / "models"
    shutil.copytree(FIXTURE, root)
    common = ["--data_root", str(root), "--news_encoder", "MSA", "--data_cache", str(tmp_path / "cache")] + SMALL
    main(["--mode", "train", "--max_steps", "1", "--model_dir", str(models)] + common)
    capsys.readouterr()
    recs = tmp_path / "recommend.txt"
    main(["--mode", "recommend", "--test_model_path", str(models / "MSA-DIGAT"), "--recommend_k", "5", "--recommend_report", "0,0.3",
          "--recommend_max_per_category", "2", "--recommend_output", str(recs)] + common)
    out = capsys.readouterr().out
    rows = [line for line in out.splitlines() if line.startswith("diversity ")]
    assert len(rows) == 2 and rows[0].startswith("diversity 0.000 : ") and rows[1].startswith("diversity 0.300 : "), out
    for line in rows:
        fields = line.split(" : ")[1].split()
        named = dict(zip(fields[::2], fields[1::2]))
        assert list(named)[:8] == ["lists", "ild", "max_sim", "categories", "category_max_share", "overlap", "coverage", "gini"], line
        assert int(named["lists"]) == len(recs.read_text().split("\n")) and 0.0 <= float(named["ild"]) <= 2.0 and 0.0 < float(named["coverage"]) <= 1.0
        assert {"recall@5", "user_recall@5", "mrr"} <= set(named), "the fixture's test split is labelled"
    assert os.path.exists(recs) and "Recommended 5 news" in out
