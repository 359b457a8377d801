"""CPU suite: list quality without a GPU — ``evaluate.list_quality_host`` (the yardstick the GPU suite holds the kernel to)
against a brute force in plain Python on awkward lists; ``evaluate.quality_summary`` on hand-computed cases; the refusals of the
Python entries; the library's entry declared, exported, bound and refusing bad arguments before any launch;
``util.recommend_report`` and ``nrms.recommend_report`` on CPU tensors; the CLI flag."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import diversify_common as V
import dot_rank_common as R
import dot_topk_common as D
import list_quality_common as Q
import test_diversify_cpu as TD
from conftest import REPO

OK, ARG, SHAPE = 0, 1, 2
NEW = ("digat_list_quality_workspace_bytes", "digat_list_quality")


# ---------------------------------------------------------------------------------------------------------------------
# list_quality_host against plain Python
# ---------------------------------------------------------------------------------------------------------------------
def host_case(seed, G, k, kb, N):
    rng = np.random.default_rng(seed)
    ids, count = V.make_lists(rng, G, k, N)
    base, base_count = V.make_lists(rng, G, kb, N)
    base[:, :min(k, kb)] = np.where(rng.random((G, min(k, kb))) < 0.5, ids[:, :min(k, kb)], base[:, :min(k, kb)])    # some overlap
    sim = rng.standard_normal((G, k, k)).astype(np.float32)
    sim[:, ::3, ::2] = np.round(sim[:, ::3, ::2])                   # ties, zeros of both signs
    category = rng.integers(-3, 9, size=N).astype(np.int32) * 1000003
    exposure = rng.integers(0, 5, size=N).astype(np.int32)
    return ids, count, base, base_count, sim, category, exposure


@pytest.mark.parametrize("G,k,kb,N", [(1, 1, 1, 5), (3, 2, 16, 40), (4, 17, 5, 30), (5, 64, 65, 300), (3, 128, 128, 50)])
def test_host_contract_is_the_brute_force(G, k, kb, N):
    from digat_amd import evaluate
    ids, count, base, base_count, sim, category, exposure = host_case(G + k, G, k, kb, N)
    got = evaluate.list_quality_host(ids, count, sim, category, base, base_count, news_num=N, exposure=exposure)
    assert got["elements"].dtype == np.int32 and got["sim_sum"].dtype == np.float64 and got["sim_max"].dtype == np.float32
    want_exposure = exposure.astype(np.int64)
    for g in range(G):
        one = Q.brute_force(ids[g], count[g], N, sim[g], category, base[g], base_count[g])
        for key, value in one.items():
            if key == "sim_max":
                assert Q.bits(got[key][g]) == Q.bits(np.float32(value)), (g, key)
            else:
                assert got[key][g] == value, (g, key, got[key][g], value)
        for p in Q.elements_of(ids[g], count[g], N):
            want_exposure[ids[g][p]] += 1
    assert np.array_equal(got["exposure"], want_exposure) and got["exposure"] is not exposure
    assert np.array_equal(exposure, host_case(G + k, G, k, kb, N)[6]), "the input histogram is left alone"
    assert G == 1 or got["elements"][1] == 0, "make_lists: list 1 is empty"
    # count None is k; the parts go by their inputs
    full = evaluate.list_quality_host(ids, None, news_num=N)
    assert set(full) == {"elements"} and full["elements"].tolist() == [len(Q.elements_of(ids[g], None, N)) for g in range(G)]
    assert set(evaluate.list_quality_host(ids, count, category=category)) == {"elements", "categories", "category_max"}
    assert set(evaluate.list_quality_host(ids, count, base_ids=base, news_num=N)) == {"elements", "overlap"}


def test_host_contract_by_hand():
    from digat_amd import evaluate
    nan, ids = np.float32("nan"), np.array([[4, 9, 4, 2, 7, -1]])
    sim = np.full((1, 6, 6), 100.0, dtype=np.float32)               # whatever is no pair of elements is never read
    el = [0, 2, 3]                                                  # count 4, id 9 outside N = 8
    sim[0][np.ix_(el, el)] = np.array([[0, nan, -0.0], [0, 0, -2.5], [0, 0, 0]], dtype=np.float32)
    got = evaluate.list_quality_host(ids, [4], sim, category=np.array([5, 5, -7, 5, -7, 5, 5, 5]), base_ids=np.array([[2, 4, 9]]),
                                     base_count=[2], exposure=np.zeros(8, dtype=np.int32))
    assert got["elements"].tolist() == [3] and math.isnan(got["sim_sum"][0])
    assert Q.bits(got["sim_max"]).tolist() == Q.bits(np.float32(0.0)).tolist(), "NaNs are passed over; a zero maximum is +0.0"
    assert got["categories"].tolist() == [1] and got["category_max"].tolist() == [3]       # ids 4, 4, 2: -7, -7, -7
    assert got["overlap"].tolist() == [3]                            # both 4s and the 2
    assert got["exposure"].tolist() == [0, 0, 1, 0, 2, 0, 0, 0]
    none = evaluate.list_quality_host(ids, [1], sim)
    assert none["sim_sum"].tolist() == [0.0] and np.isneginf(none["sim_max"]).all(), "fewer than two elements"
    empty = evaluate.list_quality_host(ids, [0], sim, category=np.zeros(8, dtype=np.int64), base_ids=ids)
    assert [empty[key].tolist() for key in ("elements", "categories", "category_max", "overlap")] == [[0]] * 4


def test_sum_bound_is_the_stated_one():
    ids, sim = np.array([[0, 1, 2, 7]]), np.arange(16, dtype=np.float32).reshape(1, 4, 4) - 3
    assert Q.sum_bound(ids, [4], sim, 5).tolist() == [3 * 2.0 ** -52 * (2 + 1 + 3)]       # pairs (0,1) (0,2) (1,2): -2, -1, 3


# ---------------------------------------------------------------------------------------------------------------------
# quality_summary
# ---------------------------------------------------------------------------------------------------------------------
def test_quality_summary_by_hand():
    from digat_amd import evaluate
    q = {"elements": np.array([4, 1, 0, 2], dtype=np.int32), "sim_sum": np.array([3.0, 0.0, 0.0, -0.5]),
         "sim_max": np.array([0.9, -np.inf, -np.inf, -0.5], dtype=np.float32), "categories": np.array([2, 1, 0, 2], dtype=np.int32),
         "category_max": np.array([3, 1, 0, 1], dtype=np.int32), "overlap": np.array([2, 1, 0, 0], dtype=np.int32)}
    s = evaluate.quality_summary(q)
    assert s["lists"] == 4
    assert s["ild"] == pytest.approx(((1 - 3.0 / 6) + (1 + 0.5 / 1)) / 2, abs=1e-15)
    assert s["max_sim"] == pytest.approx((float(np.float32(0.9)) - 0.5) / 2, abs=1e-15)
    assert s["categories"] == pytest.approx(5 / 4) and s["category_max_share"] == pytest.approx((3 / 4 + 1 + 1 / 2) / 3)
    assert s["overlap"] == pytest.approx((2 / 4 + 1 + 0) / 3)
    assert math.isnan(s["coverage"]) and math.isnan(s["gini"])
    as_tensors = evaluate.quality_summary({key: torch.from_numpy(v) for key, v in q.items()})
    assert as_tensors == pytest.approx(s, nan_ok=True)
    # exposure: equal -> gini 0; one exposed id of n -> (n - 1) / n; the pool picks the ids
    n = 7
    equal = evaluate.quality_summary(q, exposure=np.full(n, 3))
    assert equal["coverage"] == 1.0 and equal["gini"] == pytest.approx(0.0, abs=1e-15)
    one = np.zeros(n, dtype=np.int32)
    one[2] = 11
    single = evaluate.quality_summary(q, exposure=one)
    assert single["coverage"] == pytest.approx(1 / n) and single["gini"] == pytest.approx((n - 1) / n, abs=1e-15)
    pooled = evaluate.quality_summary(q, exposure=one, pool=[2, 5, 5, 6])
    assert pooled["coverage"] == pytest.approx(1 / 3) and pooled["gini"] == pytest.approx(2 / 3, abs=1e-15)
    assert evaluate.quality_summary({**q, "exposure": one})["coverage"] == pytest.approx(1 / n), "the dict's own histogram"
    assert evaluate.quality_summary(q, exposure=np.array([1, 2, 3, 4]))["gini"] == pytest.approx(2 * 30 / (4 * 10) - 5 / 4)


def test_quality_summary_of_nothing_is_nan():
    from digat_amd import evaluate
    empty = {key: np.zeros(0, dtype=np.int32) for key in ("elements", "categories", "category_max", "overlap")}
    empty.update(sim_sum=np.zeros(0), sim_max=np.zeros(0, dtype=np.float32))
    s = evaluate.quality_summary(empty, exposure=np.zeros(0, dtype=np.int32))
    assert s.pop("lists") == 0 and all(math.isnan(v) for v in s.values()), s
    s = evaluate.quality_summary({"elements": np.array([1, 0], dtype=np.int32)}, exposure=np.zeros(5, dtype=np.int32))
    assert s["lists"] == 2 and s["coverage"] == 0.0
    assert all(math.isnan(s[key]) for key in ("ild", "max_sim", "categories", "category_max_share", "overlap", "gini")), s
    lone = {"elements": np.array([1, 1], dtype=np.int32), "sim_sum": np.zeros(2), "sim_max": np.full(2, -np.inf, dtype=np.float32)}
    assert math.isnan(evaluate.quality_summary(lone)["ild"]) and math.isnan(evaluate.quality_summary(lone)["max_sim"])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_python_entries_refuse_bad_arguments():
    from digat_amd import _lib, evaluate
    ids = np.zeros((3, 4), dtype=np.int64)
    for bad, match in ((dict(ids=np.zeros(4, dtype=np.int64)), r"\[G, k\]"), (dict(ids=np.zeros((3, 129), dtype=np.int64)), r"\[G, k\]"),
                       (dict(ids=np.zeros((3, 0), dtype=np.int64)), r"\[G, k\]"), (dict(count=[1, 2]), "one entry per list"),
                       (dict(sim=np.zeros((3, 4, 5), dtype=np.float32)), r"\[G, k, k\]"), (dict(category=np.zeros((2, 2))), r"category must be \[N\]"),
                       (dict(base_count=[1, 1, 1]), "base_count needs base_ids"), (dict(base_ids=np.zeros((2, 4), dtype=np.int64)), r"\[G, kb\]"),
                       (dict(base_ids=np.zeros((3, 129), dtype=np.int64)), r"\[G, kb\]"),
                       (dict(base_ids=ids, base_count=[1]), "base_count must have one entry"),
                       (dict(category=np.zeros(5), exposure=np.zeros(6, dtype=np.int32)), "all of one N"),
                       (dict(category=np.zeros(5), news_num=6), "all of one N"), (dict(exposure=np.zeros((2, 2))), r"exposure must be \[N\]")):
        with pytest.raises(ValueError, match=match):
            evaluate.list_quality_host(**{"ids": ids, **bad})
    with pytest.raises(_lib.DigatHipError, match="GPU only"):
        evaluate.list_quality(torch.from_numpy(ids), category=torch.zeros(5, dtype=torch.int32))


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
    assert int(re.search(r"#define\s+DIGAT_ABI_VERSION\s+(\d+)", header).group(1)) == 4
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_mmr.inc"') < hip.index('#include "digat_listq.inc"')              # it calls mmr_gram
    listq = open(os.path.join(REPO, "digat_amd", "csrc", "digat_listq.inc")).read()
    assert "mmr_gram(" in listq and "mfma" not in listq.split("*/")[-1].split("struct ListqArgs")[1], "one Gram in the sources: mmr_gram"
    assert L.digat_list_quality_workspace_bytes(4096, 128, 128) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)

    def call(ids=p, count=p, G=3, k=16, N=100, vectors=p, d=20, category=p, base=p, base_count=p, kb=16, exposure=p, el=p, ssum=p, smax=p,
             cats=p, cmax=p, over=p):
        return L.digat_list_quality(ids, count, G, k, N, vectors, d, category, base, base_count, kb, exposure, el, ssum, smax, cats, cmax, over,
                                    None, 0, None)
    for name in ("ids", "el", "ssum", "smax", "cats", "cmax", "over"):
        assert call(**{name: None}) == ARG, name
    assert call(base=None, over=None) == ARG                        # a base count without base ids
    assert call(vectors=None) == ARG and call(category=None) == ARG and call(base=None, base_count=None) == ARG    # outputs without their input
    assert call(d=0) == ARG and call(d=-3) == ARG and call(G=-1) == ARG and call(N=-1) == ARG
    for k in (0, -1, 129):
        assert call(k=k) == SHAPE and call(kb=k) == SHAPE, k
    assert call(d=(1 << 24) + 1) == SHAPE and call(G=1 << 31) == SHAPE
    assert call(G=0) == OK and call(G=0, d=1 << 24, k=128, kb=128) == OK
    assert call(G=0, count=None, vectors=None, d=0, ssum=None, smax=None, category=None, cats=None, cmax=None, base=None, base_count=None,
                kb=0, over=None, exposure=None) == OK               # nothing but the elements


# ---------------------------------------------------------------------------------------------------------------------
# the sweep on CPU tensors, and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_util_recommend_report_on_cpu_tensors(monkeypatch):
    from digat_amd import evaluate, util
    TD.fake_scoring(monkeypatch)
    calls = []
    inner = util.score_rows
    monkeypatch.setattr(util, "score_rows", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1])
    dc, model = TD.host_corpus(), types.SimpleNamespace()
    users, pool, k = np.array([0, 3, 4, 1]), np.arange(1, 60), 5
    util.recommend(model, dc, users, pool, k)
    one_recommend, diversities = len(calls), (0.0, 0.3, 1.0)
    targets = (np.array([3, 9, 11, 2, 50]), np.array([0, 2, 2, 3, 5]))
    del calls[:]
    rows, lists = util.recommend_report(model, dc, users, pool, k, diversities, shortlist=12, max_per_category=2, targets=targets,
                                        return_lists=True)
    assert len(calls) == one_recommend, "one scoring pass for all diversities"
    assert [r["diversity"] for r in rows] == list(diversities) and len(lists) == 3
    unit = util.unit_rows(dc.news_embedding)
    short = util.recommend(model, dc, users, pool, 12)
    for f, row, got in zip(diversities, rows, lists):
        want = util.recommend(model, dc, users, pool, k, diversity=f, shortlist=12, max_per_category=2)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), f
        q = evaluate.list_quality_host(got[0].numpy(), got[2].numpy(), evaluate.mmr_gram_stock(got[0], unit).numpy(), dc.news_category.numpy(),
                                       short[0][:, :k].numpy(), torch.clamp(short[2], max=k).numpy(), 60, np.zeros(60, dtype=np.int32))
        assert (q["category_max"] <= 2).all()
        m = evaluate.rank_metrics(evaluate.list_ranks(got[0], got[2], *targets), targets[1], ks=(k,))
        want_row = {"diversity": f, **evaluate.quality_summary(q, pool=pool), **{n: m[n] for n in ("recall@5", "user_recall@5", "mrr")}}
        assert row == pytest.approx(want_row, nan_ok=True) and list(row) == list(want_row)
    plain = util.recommend_report(model, dc, users, pool, k, (0.0,))[0]
    assert plain["overlap"] == 1.0 and "mrr" not in plain, "diversity 0 without a cap is the plain top-k"
    with pytest.raises(ValueError):
        util.recommend_report(model, dc, users, pool, k, ())
    with pytest.raises(ValueError, match="diversity must lie"):
        util.recommend_report(model, dc, users, pool, k, (0.2, 1.5))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_report_on_cpu_tensors(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), R.dev_with_rows()
    users, k = np.arange(D.USERS), 4
    _, target_ids, target_start = nrms._clicked_targets(dev, users)
    category = (np.arange(D.NEWS) % 5).astype(np.int32)
    rows, lists = nrms.recommend_report(m, dev, users, k=k, diversities=(0.0, 0.6), shortlist=12, category=category, max_per_category=1,
                                        targets=(target_ids, target_start), return_lists=True)
    for f, row, got in zip((0.0, 0.6), rows, lists):
        want = nrms.recommend(m, dev, users, k=k, diversity=f, shortlist=12, category=category, max_per_category=1)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (pre, f)
        metrics = evaluate.rank_metrics(evaluate.list_ranks(want[0], want[2], target_ids, target_start), target_start, ks=(k,))
        assert all(row[name] == metrics[name] for name in ("recall@4", "user_recall@4", "mrr"))
        assert row["lists"] == D.USERS and row["category_max_share"] == pytest.approx(1 / k) and row["categories"] == k, "one per category"
        assert 0.0 <= row["ild"] <= 2.0 and 0.0 < row["coverage"] <= D.USERS * k / (D.NEWS - 1)
    assert math.isnan(nrms.recommend_report(m, dev, users, k=k, diversities=(0.3,))[0]["categories"]), "this corpus carries no category"


def test_main_reads_the_clicked_candidates_of_every_impression():
    from digat_amd import main
    dc = types.SimpleNamespace(row_impression=torch.tensor([0, 0, 0, 2, 2, 3]), row_candidate=torch.tensor([7, 8, 9, 4, 5, 6]),
                               history=torch.zeros(5, 3, dtype=torch.int64))
    ids, start = main.clicked_targets(dc, np.array([0, 1, 1, 0, 0, 1]))
    assert ids.tolist() == [8, 9, 6] and start.tolist() == [0, 2, 2, 2, 3, 3] and ids.dtype == start.dtype == np.int64


def test_config_parses_the_report_flag():
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not hasattr(c, "recommend_report") and "recommend_report" not in c.attribute_dict, "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_report", "0,0.1,0.3"])
    assert c.recommend_report == (0.0, 0.1, 0.3) and c.recommend_shortlist == 0 and c.recommend_max_per_category == 0
    assert not hasattr(c, "recommend_diversity"), "the lists file still goes by --recommend_diversity alone"
    c = Config(["--mode", "recommend", "--recommend_report", "0.5", "--recommend_k", "7", "--recommend_shortlist", "50",
                "--recommend_max_per_category", "2", "--recommend_diversity", "0.3"])
    assert (c.recommend_report, c.recommend_k, c.recommend_shortlist, c.recommend_max_per_category, c.recommend_diversity) == ((0.5,), 7, 50, 2, 0.3)
    for bad in ("", "a,b", "0,1.5", "-0.1", ","):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend", "--recommend_report", bad])
