"""CPU suite: retrieval evaluation without a GPU — the rank-of-target entries are declared, exported and refuse bad arguments before
any launch; the host contract ``evaluate.dot_rank_host`` against a brute-force ``sorted()`` and against ``dot_topk_host``;
``rank_metrics`` / ``shortlist_for`` / ``list_ranks`` on hand-written inputs; ``nrms.retrieval_metrics`` on CPU tensors against
brute force over the stock scores."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import dot_rank_common as R
import dot_topk_common as D
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_dot_rank_workspace_bytes", "digat_dot_rank")


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
    assert '#include "digat_dot_rank.inc"' in hip
    assert hip.index('#include "digat_dot_topk.inc"') < hip.index('#include "digat_dot_rank.inc"')       # it uses dot_tile


def test_workspace_query_is_non_decreasing():
    from digat_amd import _lib, evaluate
    q = _lib.lib().digat_dot_rank_workspace_bytes
    ch = evaluate.DOT_TOPK_CHUNK
    for users, pool, targets in ((1, 1, 1), (64, 65237, 64), (4096, 65237, 5 * 4096), (3, 2 * ch + 1, 6147)):
        assert q(users, pool, targets) >= 4 * targets                                 # one key per target
    users_axis = [q(u, 5000, 100) for u in (0, 1, 63, 64, 65, 4096)]
    pool_axis = [q(100, p, 100) for p in (0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 65237)]
    target_axis = [q(100, 5000, t) for t in (0, 1, 63, 64, 65, 1000, 1 << 20)]
    for axis in (users_axis, pool_axis, target_axis):
        assert all(a <= b for a, b in zip(axis, axis[1:])), axis
    assert q(-1, 10, 10) == 0 and q(10, -1, 10) == 0 and q(10, 10, -1) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    G, N, P, T = 5, 300, 100, 12
    need = L.digat_dot_rank_workspace_bytes(G, P, T)
    assert need > 0

    def call(users=p, news=p, pool=p, G=G, N=N, P=P, d=20, skip=p, skip_len=5, pos=p, start=p, T=T, out_r=p, out_s=p, ws=p, ws_bytes=need):
        return L.digat_dot_rank(users, news, pool, G, N, P, d, skip, skip_len, pos, start, T, out_r, out_s, ws, ws_bytes, None)
    for name in ("users", "news", "pos", "start", "out_r", "out_s", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(G=-1) == ARG and call(N=-1) == ARG and call(P=-1) == ARG and call(T=-1) == ARG
    assert call(d=0) == ARG and call(d=-4) == ARG
    for skip_len in (-1, 257):
        assert call(skip_len=skip_len) == ARG, skip_len
    assert call(pool=None) == ARG                                   # no pool: P must be N
    assert call(ws=p + 4) == ARG                                    # 8-byte alignment
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(T=1 << 20) == WORKSPACE                             # sized for 12 targets
    assert call(G=1 << 40, P=1 << 40, ws_bytes=1 << 62) == SHAPE
    assert call(T=1 << 31, ws_bytes=1 << 62) == SHAPE and call(T=1 << 40, ws_bytes=1 << 62) == SHAPE
    assert call(G=0) == OK and call(T=0) == OK
    assert call(T=0, ws=None, ws_bytes=0) == OK                     # no target: no workspace
    assert call(G=0, T=0, ws=None, ws_bytes=0) == OK


def _host_case(rng, G, P, N, integers):
    S = rng.integers(-2, 3, size=(G, P)).astype(np.float32) if integers else rng.standard_normal((G, P)).astype(np.float32)
    pool = rng.integers(0, N, size=P).astype(np.int64)                                     # unsorted, with repeats
    skip = np.stack([pool[rng.integers(0, P, size=12)] for _ in range(G)])                 # rows with repeats
    return S, pool, skip


def test_dot_rank_host_matches_a_brute_force_sort():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    G, P, N = 4, 60, 45
    S, pool, skip = _host_case(rng, G, P, N, integers=True)
    S[0, 3], S[0, 17], S[1, 0] = np.nan, np.nan, np.nan
    S[2, 5], S[2, 9], S[2, 11] = -0.0, 0.0, -0.0
    S[3, 7], S[3, 8], S[3, 20] = np.inf, -np.inf, np.inf
    assert len(np.unique(pool)) < P
    every = np.tile(np.arange(P, dtype=np.int64), G)
    starts = np.arange(G + 1, dtype=np.int64) * P
    for pl, sk in ((None, None), (pool, None), (pool, skip), (None, skip)):
        got = evaluate.dot_rank_host(S, every, starts, pool=pl, skip=sk)
        want = R.brute_ranks(S, every, starts, pool=pl, skip=sk)
        assert got.dtype == np.int32 and np.array_equal(got, want), (pl is None, sk is None)
        if sk is not None:
            assert (got == -1).any(), "some target is skipped"
    # NaNs behind every number, in position order; signed zeros tie by position; -inf is the last number
    r = evaluate.dot_rank_host(S, every, starts).reshape(G, P)
    assert r[0, 3] == P - 2 and r[0, 17] == P - 1 and r[1, 0] == P - 1
    assert r[2, 5] < r[2, 9] < r[2, 11] and r[2, 11] - r[2, 5] <= int((S[2] == 0).sum()) - 1
    assert r[3, 7] == 0 and r[3, 20] == 1 and r[3, 8] == P - 1
    for g in range(G):
        assert sorted(r[g].tolist()) == list(range(P))
    # targets out of range, repeated, a user without targets, an id outside [0, news_num)
    pos = np.array([5, 5, -1, P, 0, 59, 7], dtype=np.int64)
    st = np.array([0, 4, 4, 5, 7], dtype=np.int64)
    got = evaluate.dot_rank_host(S, pos, st, pool=pool, skip=skip, news_num=N)
    assert np.array_equal(got, R.brute_ranks(S, pos, st, pool=pool, skip=skip, news_num=N))
    assert got[0] == got[1] and got[2] == -1 and got[3] == -1
    small = int(np.sort(np.unique(pool))[len(np.unique(pool)) // 2])
    cut = evaluate.dot_rank_host(S, every, starts, pool=pool, news_num=small)
    assert np.array_equal(cut, R.brute_ranks(S, every, starts, pool=pool, news_num=small))
    assert ((cut == -1) == np.tile(pool >= small, G)).all()
    for bad in (np.array([0, 4, 4, 5, 6]), np.array([1, 4, 4, 5, 7]), np.array([0, 5, 4, 5, 7]), np.array([0, 4, 7]),
                np.array([0.0, 4.0, 4.0, 5.0, 7.0])):
        with pytest.raises(ValueError, match="target_start"):
            evaluate.dot_rank_host(S, pos, bad)
    with pytest.raises(ValueError):
        evaluate.dot_rank_host(S[0], pos, st)
    with pytest.raises(ValueError, match="pool"):
        evaluate.dot_rank_host(S, pos, st, pool=pool[:5])


@pytest.mark.parametrize("k", [1, 10, 128])
def test_rank_below_k_is_the_slot_in_dot_topk_host(k):
    from digat_amd import evaluate
    rng = np.random.default_rng(k)
    for n in range(8):
        G, P, N = 3, (40, 150, 300)[n % 3], 200
        S, pool, skip = _host_case(rng, G, P, N, integers=(n % 2 == 0))
        S[rng.integers(0, G), rng.integers(0, P, size=3)] = np.nan
        S[rng.integers(0, G), rng.integers(0, P, size=3)] = -0.0
        pl, sk = (pool if n & 2 else None), (skip if n & 4 else None)
        ids = np.arange(P) if pl is None else pl
        every = np.tile(np.arange(P, dtype=np.int64), G)
        rank = evaluate.dot_rank_host(S, every, np.arange(G + 1, dtype=np.int64) * P, pool=pl, skip=sk).reshape(G, P)
        top_s, top_i, top_c = evaluate.dot_topk_host(S, k, pool=pl, skip=sk)
        for g in range(G):
            elements = int((rank[g] >= 0).sum())
            assert sorted(rank[g][rank[g] >= 0].tolist()) == list(range(elements))
            assert top_c[g] == min(k, elements)
            for slot in range(int(top_c[g])):
                p = int(np.flatnonzero(rank[g] == slot)[0])
                assert ids[p] == top_i[g, slot] and S[g, p].view(np.uint32) == top_s[g, slot].view(np.uint32), (g, slot)


def test_rank_metrics_and_shortlist_on_hand_written_ranks():
    from digat_amd import evaluate
    rank = np.array([0, 12, -1, 3, 200, -1], dtype=np.int32)
    start = np.array([0, 2, 2, 5, 6])                       # user 1 has no target, user 3 a single unranked one
    m = evaluate.rank_metrics(rank, start, ks=(1, 10, 150, 1000))
    want = {"recall@1": 1 / 6, "recall@10": 2 / 6, "recall@150": 3 / 6, "recall@1000": 4 / 6,
            "user_recall@1": (1 / 2) / 3, "user_recall@10": (1 / 2 + 1 / 3) / 3, "user_recall@150": (1 + 1 / 3) / 3,
            "user_recall@1000": (1 + 2 / 3) / 3, "mrr": (1 + 1 / 4 + 0) / 3, "median_rank": 7.5}
    assert set(m) == set(want) | {"not_ranked", "targets", "users"}
    for name, value in want.items():
        assert m[name] == pytest.approx(value, rel=1e-15, abs=0), name
    assert (m["not_ranked"], m["targets"], m["users"]) == (2, 6, 3)
    assert evaluate.rank_metrics(torch.from_numpy(rank), torch.from_numpy(start), ks=(10,))["recall@10"] == m["recall@10"]
    assert evaluate.shortlist_for(rank, 0.5) == 13 and evaluate.shortlist_for(rank, 2 / 6) == 4 and evaluate.shortlist_for(rank, 1 / 6) == 1
    assert evaluate.shortlist_for(rank, 4 / 6) == 201 and evaluate.shortlist_for(rank, 0.0) == 1
    assert evaluate.shortlist_for(rank, 0.7) is None and evaluate.shortlist_for(rank, 1.0) is None
    for share in (0.1, 0.3, 0.5, 0.6):
        k = evaluate.shortlist_for(rank, share)
        at = lambda k: evaluate.rank_metrics(rank, start, ks=(k,))[f"recall@{k}"]
        assert at(k) >= share and (k == 1 or at(k - 1) < share)
    # nothing ranked
    none = evaluate.rank_metrics(np.array([-1, -1]), np.array([0, 2]), ks=(10,))
    assert none["recall@10"] == 0.0 and none["user_recall@10"] == 0.0 and none["mrr"] == 0.0 and math.isnan(none["median_rank"])
    assert (none["not_ranked"], none["targets"], none["users"]) == (2, 2, 1)
    assert evaluate.shortlist_for(np.array([-1, -1]), 0.1) is None
    # nothing at all
    for start0 in (np.array([0]), np.array([0, 0, 0]), np.zeros(0, dtype=np.int64)):
        empty = evaluate.rank_metrics(np.zeros(0, dtype=np.int32), start0, ks=(10, 500))
        assert all(math.isnan(empty[n]) for n in ("recall@10", "recall@500", "user_recall@10", "mrr", "median_rank"))
        assert (empty["not_ranked"], empty["targets"], empty["users"]) == (0, 0, 0)
    assert evaluate.shortlist_for(np.zeros(0, dtype=np.int32), 0.5) is None
    with pytest.raises(ValueError, match="positive"):
        evaluate.rank_metrics(rank, start, ks=(0,))
    with pytest.raises(ValueError, match="target_start"):
        evaluate.rank_metrics(rank, np.array([0, 2, 5]), ks=(1,))
    with pytest.raises(ValueError, match="share"):
        evaluate.shortlist_for(rank, 1.5)


def test_list_ranks_on_a_hand_written_result():
    from digat_amd import evaluate
    ids = torch.tensor([[4, 9, 2, -1], [7, 7, 3, 5], [-1, -1, -1, -1]])
    count = torch.tensor([3, 4, 0], dtype=torch.int32)
    targets = torch.tensor([9, 5, 2, -1, 7, 5, 4])              # -1 names a fill slot: never found
    start = np.array([0, 4, 6, 7])
    got = evaluate.list_ranks(ids, count, targets, start)
    assert got.dtype == torch.int32 and got.tolist() == [1, -1, 2, -1, 0, 3, -1]
    assert evaluate.list_ranks(ids, None, targets, start).tolist() == [1, -1, 2, 3, 0, 3, -1]      # no count: every slot is in use
    short = torch.tensor([2, 4, 0], dtype=torch.int32)
    assert evaluate.list_ranks(ids, short, targets, start).tolist() == [1, -1, -1, -1, 0, 3, -1]
    assert evaluate.list_ranks(ids, count, targets[:0], np.zeros(4, dtype=np.int64)).tolist() == []
    with pytest.raises(ValueError, match="target_start"):
        evaluate.list_ranks(ids, count, targets, np.array([0, 4, 7]))
    with pytest.raises(ValueError, match="count"):
        evaluate.list_ranks(ids, count[:2], targets, start)
    m = evaluate.rank_metrics(got, start, ks=(2,))
    assert m["recall@2"] == 2 / 7 and m["not_ranked"] == 3


# ---------------------------------------------------------------------------------------------------------------------
# nrms.retrieval_metrics on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def _want(S, hist, mask, users, target_ids, target_start, pool, exclude):
    pos = np.array([int(np.flatnonzero(pool == t)[0]) if (pool == t).any() else -1 for t in target_ids], dtype=np.int64)
    skip = None
    if exclude:
        skip = np.stack([np.where(mask[g], hist[g], 0) for g in users])
    return R.brute_ranks(S[users][:, pool], pos, target_start, pool=pool, skip=skip)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_retrieval_metrics_match_brute_force_over_the_stock_scores(pre):
    from digat_amd import evaluate, nrms
    inp = D.inputs()
    hist, mask, cand = inp["history_ids"], inp["history_mask"], inp["candidate_ids"]
    labels = np.zeros((D.USERS, R.CANDS), dtype=np.int64)
    labels[:, 0], labels[:, 3] = 1, 1
    labels[4] = 0                                                   # impression 4 has no click: not a default user
    labels[6] = 1                                                   # impression 6 clicked everything
    m, dev = D.model(pre), R.dev_with_rows(labels=labels)
    S = D.stock_scores(m, D.dev_set())
    everything = np.arange(1, D.NEWS, dtype=np.int64)
    # default users and targets
    got = nrms.retrieval_metrics(m, dev, ks=(1, 10, 60), batch_size=4)
    users = np.array([g for g in range(D.USERS) if g != 4])
    tid = np.concatenate([cand[g][labels[g] == 1] for g in users])
    tst = np.r_[0, np.cumsum([int(labels[g].sum()) for g in users])]
    assert np.array_equal(got["target_ids"], tid) and np.array_equal(got["target_start"], tst) and got["rank"].dtype == np.int32
    want = _want(S, hist, mask, users, tid, tst, everything, True)
    assert np.array_equal(got["rank"], want)
    metrics = evaluate.rank_metrics(want, tst, ks=(1, 10, 60))
    assert {k: v for k, v in got.items() if k not in ("rank", "target_start", "target_ids")} == metrics
    assert got["users"] == D.USERS - 1 and got["targets"] == len(tid)
    # a clicked news of the user's own history, and row 0, are not ranked under exclude_history
    for t, g in zip(range(len(tid)), np.repeat(users, np.diff(tst))):
        assert (want[t] == -1) == (int(tid[t]) in D.banned_ids(hist[g], mask[g])), t
    # candidates at their word: everything in the pool is ranked
    free = nrms.retrieval_metrics(m, dev, users=np.array([6, 0, 6]), exclude_history=False, ks=(5,))
    ftid = np.concatenate([cand[g][labels[g] == 1] for g in (6, 0, 6)])
    ftst = np.array([0, 5, 7, 12])
    assert np.array_equal(free["target_ids"], ftid) and np.array_equal(free["target_start"], ftst)
    assert np.array_equal(free["rank"], _want(S, hist, mask, np.array([6, 0, 6]), ftid, ftst, everything, False))
    assert ((free["rank"] == -1) == (ftid == 0)).all(), "only row 0 is outside the default pool"
    # explicit targets, a shared pool (unsorted, a repeated id) that omits some of them
    pool = np.r_[np.arange(60, 20, -1), 33, np.arange(5)].astype(np.int64)
    who = np.array([2, 8, 1])
    xt = np.array([33, 70, 0, 4, 21, 33], dtype=np.int64)
    xs = np.array([0, 3, 3, 6])
    exp = nrms.retrieval_metrics(m, dev, users=who, targets=(xt, xs), candidates=pool, ks=(3,))
    assert np.array_equal(exp["rank"], _want(S, hist, mask, who, xt, xs, pool, True)) and exp["rank"][1] == -1
    assert exp["users"] == 2 and np.array_equal(exp["target_ids"], xt)
    people = nrms.retrieval_metrics(m, dev, users=(hist[who], mask[who]), targets=(torch.from_numpy(xt), xs), candidates=pool, ks=(3,))
    assert np.array_equal(people["rank"], exp["rank"])
    nobody = nrms.retrieval_metrics(m, dev, users=np.zeros(0, dtype=np.int64), ks=(3,))
    assert nobody["targets"] == 0 and math.isnan(nobody["recall@3"])


def test_retrieval_metrics_refuses_bad_arguments():
    from digat_amd import nrms
    m, dev = D.model("nrms"), R.dev_with_rows()
    two = np.array([0, 1])
    with pytest.raises(ValueError, match="list_ranks"):
        nrms.retrieval_metrics(m, dev, users=two, candidates=(np.arange(1, 8), np.array([0, 3, 7])))
    for bad in (np.array([0, 3]), np.array([1, 2, 4]), np.array([0, 3, 2]), np.array([0, 2, 3])):
        with pytest.raises(ValueError, match="target_start"):
            nrms.retrieval_metrics(m, dev, users=two, targets=(np.array([5, 6, 7, 8]), bad))
    for bad in (np.array([1, D.NEWS]), np.array([-1, 2])):
        with pytest.raises(ValueError, match="target ids"):
            nrms.retrieval_metrics(m, dev, users=two, targets=(bad, np.array([0, 1, 2])))
        with pytest.raises(ValueError, match="candidate ids"):
            nrms.retrieval_metrics(m, dev, users=two, candidates=bad)
    with pytest.raises(ValueError, match="impression indices"):
        nrms.retrieval_metrics(m, dev, users=np.array([0, D.USERS]))
    with pytest.raises(ValueError, match="need users"):
        nrms.retrieval_metrics(m, dev, targets=(np.array([5]), np.array([0, 1])))
    with pytest.raises(ValueError, match="impression indices"):
        nrms.retrieval_metrics(m, dev, users=(np.zeros((2, D.HIST), dtype=np.int64), np.zeros((2, D.HIST), dtype=bool)))
    with pytest.raises(ValueError, match="does not carry"):
        nrms.retrieval_metrics(m, D.dev_set(), users=two)
    with pytest.raises(ValueError, match="positive"):
        nrms.retrieval_metrics(m, dev, users=two, ks=(0,))
