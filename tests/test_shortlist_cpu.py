"""CPU suite: long shortlists without a GPU — the four entries are declared, exported and bound; their workspace queries; the refusals,
which come before any launch; the host contracts (``shortlist_segments_host``, ``dot_shortlist_host``) on hand-written inputs;
``nrms.shortlist`` on CPU tensors against a brute-force ``sorted()`` over the stock scores."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dot_topk_common as D
import shortlist_common as SC
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_shortlist_segments_workspace_bytes", "digat_shortlist_segments", "digat_dot_shortlist_workspace_bytes", "digat_dot_shortlist")


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
    assert int(re.search(r"#define\s+DIGAT_SHORTLIST_MAX_K\s+(\d+)", header).group(1)) == evaluate.SHORTLIST_MAX_K == 1024
    assert evaluate.TOPK_MAX_K == 128 and SC.CHUNK == evaluate.TOPK_CHUNK
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_dot_topk.inc"') < hip.index('#include "digat_shortlist.inc"')       # it launches dot_chunk_kernel


def test_workspace_queries():
    from digat_amd import _lib
    L = _lib.lib()
    q, ch = L.digat_shortlist_segments_workspace_bytes, SC.CHUNK
    for rows, segments, m in ((1, 1, 1), (5 * ch + 3, 7, 1024), (100, 100, 129)):
        assert q(rows, segments, m) >= (rows // ch + segments) * m * 8
    for axis in ([q(r, 5, 300) for r in (0, 1, ch - 1, ch, ch + 1, 10 * ch)], [q(3 * ch, s, 300) for s in (1, 2, 100)],
                 [q(3 * ch, 5, m) for m in (1, 128, 129, 1023, 1024)]):
        assert all(a <= b for a, b in zip(axis, axis[1:])) and axis[0] > 0, axis
    assert q(-1, 5, 10) == 0 and q(10, 0, 10) == 0 and q(10, -1, 10) == 0 and q(10, 5, 0) == 0 and q(10, 5, 1025) == 0
    d = L.digat_dot_shortlist_workspace_bytes
    for P, m, slab in ((1, 1, 1), (65237, 1024, 256), (2 * ch + 1, 129, 100)):
        assert d(7, P, m, slab) >= slab * P * 4 + slab * -(-P // ch) * m * 8
    for axis in ([d(9, P, 300, 64) for P in (1, 1024, 1025, ch, ch + 1, 65237)], [d(9, 5000, m, 64) for m in (1, 129, 1024)],
                 [d(9, 5000, 300, s) for s in (1, 2, 64, 256, 1000)]):
        assert all(a <= b for a, b in zip(axis, axis[1:])) and axis[0] > 0, axis
    assert len({d(G, 65237, 1024, 256) for G in (0, 1, 64, 4096, 1 << 30)}) == 1, "the workspace does not grow with the users"
    assert d(9, 5000, 300, 0) == d(9, 5000, 300, -5) == d(9, 5000, 300, 256), "no slab named: 256"
    assert d(4096, 65237, 1024, 256) < 100 << 20 < 4096 * 65237 * 4
    assert d(-1, 10, 10, 4) == 0 and d(10, -1, 10, 4) == 0 and d(10, 10, 0, 4) == 0 and d(10, 10, 1025, 4) == 0


def test_segment_entry_refuses_bad_arguments_before_any_launch():
    from digat_amd import _lib
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    rows, segments = 3 * SC.CHUNK, 4
    need = L.digat_shortlist_segments_workspace_bytes(rows, segments, 300)
    assert need > 0

    def call(scores=p, start=p, rows=rows, segments=segments, ids=p, skip=p, skip_len=5, m=300, out_s=p, out_i=p, out_c=p, ws=p,
             ws_bytes=need):
        return L.digat_shortlist_segments(scores, start, rows, segments, ids, skip, skip_len, m, out_s, out_i, out_c, ws, ws_bytes, None)
    for m in (0, -1, 1025):
        assert call(m=m) == ARG, m
    for skip_len in (-1, 257):
        assert call(skip_len=skip_len) == ARG, skip_len
    assert call(ids=None) == ARG                                    # skip needs ids
    for name in ("scores", "start", "out_s", "out_i", "out_c", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(rows=-1) == ARG and call(segments=-1) == ARG
    assert call(ws=p + 4) == ARG                                    # 8-byte alignment
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(m=1024) == WORKSPACE                                # sized for m = 300
    assert call(m=1025, ws_bytes=0) == ARG                          # the list length is judged before the workspace
    assert call(rows=1 << 50, ws_bytes=1 << 62) == SHAPE
    assert call(segments=0) == OK and call(segments=0, ws=None, ws_bytes=0) == OK


def test_dot_entry_refuses_bad_arguments_before_any_launch():
    from digat_amd import _lib
    L = _lib.lib()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    G, N, P = 5, 30000, 20000
    need = L.digat_dot_shortlist_workspace_bytes(G, P, 300, 2)
    assert need > 0

    def call(users=p, news=p, pool=p, G=G, N=N, P=P, d=20, skip=p, skip_len=5, m=300, slab=2, out_s=p, out_i=p, out_c=p, ws=p, ws_bytes=need):
        return L.digat_dot_shortlist(users, news, pool, G, N, P, d, skip, skip_len, m, slab, out_s, out_i, out_c, ws, ws_bytes, None)
    for m in (0, -1, 1025):
        assert call(m=m) == ARG, m
    for skip_len in (-1, 257):
        assert call(skip_len=skip_len) == ARG, skip_len
    for name in ("users", "news", "out_s", "out_i", "out_c", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(G=-1) == ARG and call(N=-1) == ARG and call(P=-1) == ARG
    assert call(d=0) == ARG and call(d=-4) == ARG
    assert call(pool=None) == ARG                                   # no pool: P must be N
    assert call(ws=p + 4) == ARG
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(m=1024) == WORKSPACE and call(slab=3) == WORKSPACE  # sized for m = 300 and slabs of two users
    assert call(P=1 << 50, slab=1 << 20, ws_bytes=1 << 62) == SHAPE
    assert call(G=0) == OK and call(G=0, ws=None, ws_bytes=0) == OK
    assert call(G=0, m=1025) == ARG


def test_host_contract_on_hand_written_inputs():
    from digat_amd import evaluate
    nan, inf = np.nan, np.inf
    #           0    1     2    3     4     5    6    7     8    9    | 10   11
    x = np.array([1.0, nan, -0.0, inf, 0.0, -inf, 1.0, nan, 1.0, inf, 5.0, 4.0], dtype=np.float32)
    start = np.array([0, 10, 10, 12], dtype=np.int64)
    s, i, c = evaluate.shortlist_segments_host(x, start, 300)
    assert s.shape == (3, 300) and i.shape == (3, 300) and c.tolist() == [10, 0, 2]
    assert i[0, :10].tolist() == [3, 9, 0, 6, 8, 2, 4, 5, 1, 7]       # ties by position, -0.0 == +0.0, -inf before the NaNs
    assert SC.bits(s[0, :10]).tolist() == SC.bits(x[[3, 9, 0, 6, 8, 2, 4, 5, 1, 7]]).tolist()      # the zeros keep their signs
    assert (i[0, 10:] == -1).all() and np.isneginf(s[0, 10:]).all() and (i[1] == -1).all() and np.isneginf(s[1]).all()
    assert i[2, :2].tolist() == [0, 1] and s[2, :2].tolist() == [5.0, 4.0]
    # ids and a skip row that leaves fewer than m
    ids = np.array([7, 8, 9, 7, 3, 3, 2, 1, 7, 5, 11, 12], dtype=np.int64)
    skip = np.array([[7, 3, 100], [1, 1, 1], [12, 0, 0]], dtype=np.int64)
    s, i, c = evaluate.shortlist_segments_host(x, start, 129, ids=ids, skip=skip)
    assert c.tolist() == [5, 0, 1]
    assert i[0, :5].tolist() == [5, 2, 9, 8, 1] and i[2, 0] == 11     # inf (id 5), 1.0 (id 2), -0.0 (id 9), then the NaNs in order
    assert (i[0, 5:] == -1).all() and np.isneginf(s[0, 5:]).all()
    # a segment shorter than m next to one longer than m
    y = np.arange(40, dtype=np.float32)
    s, i, c = evaluate.shortlist_segments_host(y, np.array([0, 3, 40]), 10)
    assert c.tolist() == [3, 10] and i[0, :3].tolist() == [2, 1, 0] and i[1].tolist() == list(range(36, 26, -1))
    # the bound, and the old entry's
    assert evaluate.shortlist_segments_host(y, np.array([0, 40]), 1024)[2].tolist() == [40]
    for m in (0, 1025):
        with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
            evaluate.shortlist_segments_host(y, np.array([0, 40]), m)
    with pytest.raises(ValueError, match="k must be"):
        evaluate.topk_segments_host(y, np.array([0, 40]), 129)
    with pytest.raises(ValueError, match="skip needs ids"):
        evaluate.shortlist_segments_host(y, np.array([0, 40]), 5, skip=np.zeros((1, 2), dtype=np.int64))
    # the dot contract: G segments of length P over the pool's ids
    S = np.array([[1.0, 3.0, 3.0, nan], [0.0, -0.0, 2.0, 2.0]], dtype=np.float32)
    pool = np.array([40, 41, 41, 43], dtype=np.int64)
    s, i, c = evaluate.dot_shortlist_host(S, 200, pool=pool, skip=np.array([[40], [43]], dtype=np.int64))
    assert c.tolist() == [3, 3] and i[0, :3].tolist() == [41, 41, 43] and i[1, :3].tolist() == [41, 40, 41]
    assert evaluate.dot_shortlist_host(S, 3)[1].tolist() == [[1, 2, 0], [2, 3, 0]]
    with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
        evaluate.dot_shortlist_host(S, 1025)
    with pytest.raises(ValueError, match="k must be"):
        evaluate.dot_topk_host(S, 129)


def test_host_contract_is_topk_segments_host_up_to_128():
    from digat_amd import evaluate
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 400, size=12)
    lens[3] = 0
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    x = rng.integers(-4, 5, size=int(start[-1])).astype(np.float32)
    x[rng.integers(0, len(x), size=30)] = np.nan
    ids = rng.integers(0, 300, size=len(x)).astype(np.int64)
    skip = rng.integers(0, 300, size=(12, 20)).astype(np.int64)
    for m in range(1, 129):
        for kw in ({}, {"ids": ids}, {"ids": ids, "skip": skip}):
            SC.same(evaluate.shortlist_segments_host(x, start, m, **kw), evaluate.topk_segments_host(x, start, m, **kw), (m, sorted(kw)))
    wide = evaluate.shortlist_segments_host(x, start, 400, ids=ids, skip=skip)
    narrow = evaluate.topk_segments_host(x, start, 128, ids=ids, skip=skip)
    assert np.array_equal(wide[1][:, :128], narrow[1]) and np.array_equal(SC.bits(wide[0][:, :128]), SC.bits(narrow[0]))
    assert np.array_equal(np.minimum(wide[2], 128), narrow[2])


# ---------------------------------------------------------------------------------------------------------------------
# nrms.shortlist on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(D.MODELS))
def test_shortlist_matches_sorted_over_the_stock_scores(pre):
    from digat_amd import nrms
    m, dev, inp = D.model(pre), SC.dev_set(), SC.inputs()
    S = D.stock_scores(m, dev)
    hist, mask = inp["history_ids"], inp["history_mask"]
    users = np.arange(SC.USERS)
    everything = np.arange(1, SC.NEWS)
    for width in (300, 1024):                                       # 1024: more than the 511 news there are
        for exclude in (True, False):
            got = nrms.shortlist(m, dev, users, m=width, exclude_history=exclude, batch_size=4)
            want = [D.brute_force(S[g], everything, D.banned_ids(hist[g], mask[g]) if exclude else set(), width) for g in users]
            D.check_rows(*got, want, width)
    assert (nrms.shortlist(m, dev, users, m=1024)[2] < 1024).all()
    # up to 128 the lists are recommend's
    for a, b in zip(nrms.shortlist(m, dev, users, m=128), nrms.recommend(m, dev, users, k=128)):
        assert torch.equal(a, b)
    # per-user lists: an empty one, one shorter than m, one longer
    rng = np.random.default_rng(2)
    some = np.array([3, 1, 5, 0])
    lens = [12, 0, 150, 400]
    lists = [rng.integers(0, SC.NEWS, size=n).astype(np.int64) for n in lens]
    csr = (np.concatenate(lists), np.r_[0, np.cumsum(lens)])
    got = nrms.shortlist(m, dev, some, candidates=csr, m=140)
    want = [D.brute_force(S[g], lists[j], D.banned_ids(hist[g], mask[g]), 140) for j, g in enumerate(some)]
    D.check_rows(*got, want, 140)
    # the default width, and people who are no rows of the corpus
    ids, scores, count = nrms.shortlist(m, dev, (hist[:2], mask[:2]))
    assert tuple(ids.shape) == (2, 512) and count.tolist() == [len(everything) - len(D.banned_ids(hist[g], mask[g]) - {0}) for g in range(2)]


def test_shortlist_refuses_bad_arguments_and_feeds_candidates_csr():
    from digat_amd import evaluate, nrms, util
    m, dev = D.model("nrms"), SC.dev_set()
    two = np.array([0, 1])
    for width in (0, 1025, -3):
        with pytest.raises(ValueError, match="SHORTLIST_MAX_K"):
            nrms.shortlist(m, dev, two, m=width)
    with pytest.raises(ValueError, match="k must be"):
        nrms.recommend(m, dev, two, k=129)
    with pytest.raises(ValueError, match="k must be"):
        util.recommend_limits(129, 0)
    assert util.recommend_limits(129, 0, long_lists=True) == 129
    with pytest.raises(ValueError, match="impression indices"):
        nrms.shortlist(m, dev, np.array([0, SC.USERS]))
    ids, scores, count = nrms.shortlist(m, dev, np.arange(SC.USERS), m=600)
    assert tuple(ids.shape) == (SC.USERS, 600) and int(count.max()) < 600
    flat, start = nrms.candidates_csr(ids, count)
    assert int(start[-1]) == int(count.sum()) == len(flat) and (flat > 0).all()
    got_ids, got_start = util.recommend_candidates((flat, start), users=SC.USERS, news_num=SC.NEWS)
    assert got_ids.tolist() == flat.tolist() and got_start.tolist() == start.tolist()
    for g in range(SC.USERS):
        assert flat[start[g]:start[g + 1]].tolist() == ids[g, :int(count[g])].tolist()
    # a second stage's lists are held to the first stage's by list_ranks
    rank = evaluate.list_ranks(ids, count, ids[:, 5], np.arange(SC.USERS + 1))
    assert rank.tolist() == [5] * SC.USERS
