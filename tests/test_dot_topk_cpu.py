"""CPU suite: NRMS retrieval without a GPU — the inner-product top-k entries are declared, exported and refuse bad arguments before
any launch; ``nrms.recommend`` on CPU tensors (the stock path with ``topk_segments_host``) against a brute-force ``sorted()`` over
the stock scores; its argument checks; ``candidates_csr``."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import dot_topk_common as D
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_dot_topk_workspace_bytes", "digat_dot_topk", "digat_dot_scores")


def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4
    assert int(re.search(r"#define\s+DIGAT_ABI_VERSION\s+(\d+)", header).group(1)) == 4
    for macro, value in (("DIGAT_DOT_TOPK_CHUNK", evaluate.DOT_TOPK_CHUNK), ("DIGAT_DOT_TOPK_USERS", evaluate.DOT_TOPK_USERS),
                         ("DIGAT_DOT_TOPK_SUB", evaluate.DOT_TOPK_SUB)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == value, macro
    assert evaluate.DOT_TOPK_CHUNK % evaluate.DOT_TOPK_SUB == 0
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert '#include "digat_dot_topk.inc"' in hip
    assert hip.index('#include "digat_topk.inc"') < hip.index('#include "digat_dot_topk.inc"')       # it uses topk_select


def test_workspace_query_is_non_decreasing_and_covers_every_slot():
    from digat_amd import _lib, evaluate
    q = _lib.lib().digat_dot_topk_workspace_bytes
    ch = evaluate.DOT_TOPK_CHUNK
    for users, pool, k in ((1, 1, 1), (64, 65237, 10), (4096, 65237, 128), (3, 2 * ch + 1, 7)):
        assert q(users, pool, k) >= users * -(-pool // ch) * k * 8
    users_axis = [q(u, 5000, 10) for u in (0, 1, 63, 64, 65, 4096)]
    pool_axis = [q(100, p, 10) for p in (0, 1, ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, 65237)]
    k_axis = [q(100, 5000, k) for k in (1, 2, 10, 100, 128)]
    for axis in (users_axis, pool_axis, k_axis):
        assert all(a <= b for a, b in zip(axis, axis[1:])), axis
    assert q(-1, 10, 10) == 0 and q(10, -1, 10) == 0 and q(10, 10, 0) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    G, N, P = 5, 300, 100
    need = L.digat_dot_topk_workspace_bytes(G, P, 10)
    assert need > 0

    def call(users=p, news=p, pool=p, G=G, N=N, P=P, d=20, skip=p, skip_len=5, k=10, out_s=p, out_i=p, out_c=p, ws=p, ws_bytes=need):
        return L.digat_dot_topk(users, news, pool, G, N, P, d, skip, skip_len, k, out_s, out_i, out_c, ws, ws_bytes, None)
    for k in (0, -1, 129):
        assert call(k=k) == ARG, k
    for skip_len in (-1, 257):
        assert call(skip_len=skip_len) == ARG, skip_len
    for name in ("users", "news", "out_s", "out_i", "out_c", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(G=-1) == ARG and call(N=-1) == ARG and call(P=-1) == ARG
    assert call(d=0) == ARG and call(d=-4) == ARG
    assert call(pool=None) == ARG                                   # no pool: P must be N
    assert call(ws=p + 4) == ARG                                    # 8-byte alignment
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(k=128) == WORKSPACE                                 # sized for k = 10
    assert call(G=0) == OK
    assert call(G=0, ws=None, ws_bytes=0) == OK
    assert call(G=1 << 40, P=1 << 40, ws_bytes=1 << 62) == SHAPE

    def scores(users=p, news=p, pool=p, G=G, N=N, P=P, d=20, out=p):
        return L.digat_dot_scores(users, news, pool, G, N, P, d, out, None)
    for name in ("users", "news", "out"):
        assert scores(**{name: None}) == ARG, name
    assert scores(G=-1) == ARG and scores(N=-1) == ARG and scores(P=-1) == ARG and scores(d=0) == ARG
    assert scores(pool=None) == ARG
    assert scores(G=0) == OK and scores(P=0) == OK


def test_dot_topk_host_is_the_segment_contract():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    S = rng.integers(-2, 3, size=(4, 30)).astype(np.float32)
    S[1, 3] = np.nan
    pool = rng.permutation(100)[:30].astype(np.int64)
    skip = np.stack([rng.permutation(pool)[:4] for _ in range(4)])
    got = evaluate.dot_topk_host(S, 7, pool=pool, skip=skip)
    for g in range(4):
        want = D.brute_force({int(c): S[g, j] for j, c in enumerate(pool)}, pool, set(skip[g].tolist()), 7)
        assert got[2][g] == 7 and got[1][g].tolist() == [e[0] for e in want]
        assert got[0][g].view(np.uint32).tolist() == [int(np.float32(e[1]).view(np.uint32)) for e in want]
    pos = evaluate.dot_topk_host(S, 3)                                                     # no pool: positions
    assert pos[1][0].tolist() == np.argsort(-S[0], kind="stable")[:3].tolist()
    with pytest.raises(ValueError):
        evaluate.dot_topk_host(S, 3, pool=pool[:5])
    with pytest.raises(ValueError):
        evaluate.dot_topk_host(S[0], 3)


# ---------------------------------------------------------------------------------------------------------------------
# nrms.recommend on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(D.MODELS))
def test_recommend_matches_sorted_over_the_stock_scores(pre):
    from digat_amd import nrms
    m, dev, inp = D.model(pre), D.dev_set(), D.inputs()
    S = D.stock_scores(m, dev)
    hist, mask = inp["history_ids"], inp["history_mask"]
    assert not mask[1].any() and mask[2].sum() == 1, "user 1 has an empty history, user 2 a single item"
    users = np.arange(D.USERS)
    everything = np.arange(1, D.NEWS)
    for k in (1, 10):
        for exclude in (True, False):
            got = nrms.recommend(m, dev, users, k=k, exclude_history=exclude, batch_size=4)
            want = [D.brute_force(S[g], everything, D.banned_ids(hist[g], mask[g]) if exclude else set(), k) for g in users]
            D.check_rows(*got, want, k)
            if exclude:
                ids = got[0].numpy()
                assert all(not (set(ids[g].tolist()) & D.banned_ids(hist[g], mask[g])) for g in users)
    # the empty history excludes row 0 alone; a pool that names row 0 returns it only when the candidates are taken at their word
    pool = np.array([5, 0, 7, 5, 31], dtype=np.int64)                                     # a repeated id: two elements
    got = nrms.recommend(m, dev, np.array([1]), candidates=pool, k=4, exclude_history=True)
    D.check_rows(*got, [D.brute_force(S[1], pool, {0}, 4)], 4)
    assert 0 not in got[0].tolist()[0] and got[0].tolist()[0].count(5) == 2
    got = nrms.recommend(m, dev, np.array([1]), candidates=pool, k=5, exclude_history=False)
    D.check_rows(*got, [D.brute_force(S[1], pool, set(), 5)], 5)
    assert 0 in got[0].tolist()[0]


def test_recommend_pool_smaller_than_k_and_users_in_any_order():
    from digat_amd import nrms
    m, dev, inp = D.model("nrms"), D.dev_set(), D.inputs()
    S = D.stock_scores(m, dev)
    hist, mask = inp["history_ids"], inp["history_mask"]
    users = np.array([4, 0, 4, 8])
    pool = np.array([9, 3, 44, 17, 2, 60], dtype=np.int64)
    ids, scores, count = nrms.recommend(m, dev, users, candidates=pool, k=10)
    want = [D.brute_force(S[g], pool, D.banned_ids(hist[g], mask[g]), 10) for g in users]
    D.check_rows(ids, scores, count, want, 10)
    assert (count.numpy() < 10).all() and (ids[:, 6:] == -1).all() and torch.isneginf(scores[:, 6:]).all()
    assert torch.equal(ids[0], ids[2])
    empty = nrms.recommend(m, dev, users, candidates=np.zeros(0, dtype=np.int64), k=3)
    assert empty[2].tolist() == [0] * 4 and (empty[0] == -1).all() and torch.isneginf(empty[1]).all()
    nobody = nrms.recommend(m, dev, np.zeros(0, dtype=np.int64), k=3)
    assert tuple(nobody[0].shape) == (0, 3) and tuple(nobody[2].shape) == (0,)


def test_recommend_takes_people_who_are_no_rows_of_the_corpus():
    from digat_amd import nrms
    m, dev = D.model("sa"), D.dev_set()
    rng = np.random.default_rng(8)
    hist = rng.integers(1, D.NEWS, size=(3, D.HIST)).astype(np.int64)
    mask = np.arange(D.HIST)[None, :] < np.array([[D.HIST], [2], [0]])
    hist[~mask] = 0
    S = D.stock_scores(m, dev, hist, mask)
    got = nrms.recommend(m, dev, (hist, mask), k=6)
    D.check_rows(*got, [D.brute_force(S[g], np.arange(1, D.NEWS), D.banned_ids(hist[g], mask[g]), 6) for g in range(3)], 6)
    vec = nrms.user_vectors(m, dev, (hist, mask), batch_size=2)
    assert tuple(vec.shape) == (3, D.HEADS * D.DK)
    by_index = nrms.user_vectors(m, dev, np.array([2, 0]))
    assert torch.equal(by_index[1], nrms.user_vectors(m, dev, np.array([0]))[0])


def test_recommend_per_user_lists():
    from digat_amd import nrms
    m, dev, inp = D.model("sa"), D.dev_set(), D.inputs()
    S = D.stock_scores(m, dev)
    hist, mask = inp["history_ids"], inp["history_mask"]
    rng = np.random.default_rng(2)
    users = np.array([3, 1, 7, 0])
    lens = [12, 0, 3, 40]                                                                 # an empty list, one shorter than k
    lists = [rng.integers(0, D.NEWS, size=n).astype(np.int64) for n in lens]
    csr = (np.concatenate(lists), np.r_[0, np.cumsum(lens)])
    for exclude in (True, False):
        got = nrms.recommend(m, dev, users, candidates=csr, k=5, exclude_history=exclude)
        want = [D.brute_force(S[g], lists[j], D.banned_ids(hist[g], mask[g]) if exclude else set(), 5) for j, g in enumerate(users)]
        D.check_rows(*got, want, 5)
        assert got[2][1] == 0


def test_recommend_refuses_bad_arguments():
    from digat_amd import nrms
    m, dev = D.model("nrms"), D.dev_set()
    pool = np.arange(1, 20)
    two = np.array([0, 1])
    for k in (0, 129, -3):
        with pytest.raises(ValueError, match="k must be"):
            nrms.recommend(m, dev, two, pool, k)
    with pytest.raises(ValueError, match="max_history_num"):
        nrms.recommend(m, dev, (np.zeros((2, D.HIST + 1), dtype=np.int64), np.zeros((2, D.HIST + 1), dtype=bool)), pool, 3)
    with pytest.raises(ValueError, match="history_mask"):
        nrms.recommend(m, dev, (np.zeros((2, D.HIST), dtype=np.int64), np.zeros((3, D.HIST), dtype=bool)), pool, 3)
    with pytest.raises(ValueError, match="history ids"):
        nrms.recommend(m, dev, (np.full((2, D.HIST), D.NEWS, dtype=np.int64), np.ones((2, D.HIST), dtype=bool)), pool, 3)
    with pytest.raises(ValueError, match="impression indices"):
        nrms.recommend(m, dev, np.array([0, D.USERS]), pool, 3)
    with pytest.raises(ValueError, match="impression indices"):
        nrms.recommend(m, dev, np.array([-1]), pool, 3)
    with pytest.raises(ValueError, match="users must be"):
        nrms.recommend(m, dev, np.array([0.5, 1.0]), pool, 3)
    with pytest.raises(ValueError, match="last candidate start"):
        nrms.recommend(m, dev, two, (np.arange(1, 8), np.array([0, 3, 6])), 3)
    with pytest.raises(ValueError, match="users \\+ 1"):
        nrms.recommend(m, dev, two, (np.arange(1, 8), np.array([0, 7])), 3)
    with pytest.raises(ValueError, match="never decrease"):
        nrms.recommend(m, dev, two, (np.arange(1, 8), np.array([0, 9, 7])), 3)
    for bad in (np.array([1, D.NEWS]), np.array([-1, 2])):
        with pytest.raises(ValueError, match="candidate ids"):
            nrms.recommend(m, dev, two, bad, 3)
    with pytest.raises(ValueError, match="candidates must be"):
        nrms.recommend(m, dev, two, np.zeros((2, 2), dtype=np.int64), 3)
    long = types.SimpleNamespace(**vars(dev))
    long.history_ids = torch.zeros((2, 257), dtype=torch.int64)
    long.history_mask = torch.zeros((2, 257), dtype=torch.bool)
    with pytest.raises(ValueError, match="exclude_history"):
        nrms.recommend(m, long, two, pool, 3)


def test_candidates_csr_round_trips_into_util_recommend():
    from digat_amd import nrms, util
    ids = torch.tensor([[4, 9, 2], [7, -1, -1], [-1, -1, -1], [1, 3, -1]])
    count = torch.tensor([3, 1, 0, 2], dtype=torch.int32)
    flat, start = nrms.candidates_csr(ids, count)
    assert flat.tolist() == [4, 9, 2, 7, 1, 3] and flat.dtype == torch.int64
    assert start.tolist() == [0, 3, 4, 4, 6] and start.dtype == np.int64
    for g in range(4):
        assert flat[start[g]:start[g + 1]].tolist() == ids[g, :int(count[g])].tolist()
    got_ids, got_start = util.recommend_candidates((flat, start), users=4, news_num=10)
    assert got_ids.tolist() == flat.tolist() and got_start.tolist() == start.tolist()
    none = nrms.candidates_csr(torch.full((2, 3), -1), torch.zeros(2, dtype=torch.int32))
    assert none[0].numel() == 0 and none[1].tolist() == [0, 0, 0]
    util.recommend_candidates(none, users=2, news_num=10)
    with pytest.raises(ValueError):
        nrms.candidates_csr(ids, count[:3])
    with pytest.raises(ValueError):
        nrms.candidates_csr(ids, torch.tensor([4, 0, 0, 0]))
    # a whole result, fill included
    m, dev = D.model("nrms"), D.dev_set()
    res = nrms.recommend(m, dev, np.arange(D.USERS), candidates=np.array([9, 3, 44, 17]), k=6)
    flat, start = nrms.candidates_csr(res[0], res[2])
    assert (flat >= 0).all() and int(start[-1]) == int(res[2].sum())
    util.recommend_candidates((flat, start), users=D.USERS, news_num=D.NEWS)
