"""CPU suite: top-k recommendation without a GPU — the segmented top-k entry is declared, exported and refuses bad arguments
before any launch; its numpy restatement (``evaluate.topk_segments_host``, which the GPU suite holds the kernel to exactly)
follows the contract against a brute-force ``sorted()``; ``util.recommend``'s argument checks and row builder; the CLI flags."""
import ctypes as C
import math
import os
import re
import struct
import types

import numpy as np
import pytest
import torch

from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_topk_segments_workspace_bytes", "digat_topk_segments")


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
    assert int(re.search(r"#define\s+DIGAT_TOPK_CHUNK\s+(\d+)", header).group(1)) == evaluate.TOPK_CHUNK
    assert '#include "digat_topk.inc"' in open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()


def test_workspace_query_covers_every_chunk_slot():
    from digat_amd import _lib, evaluate
    L = _lib.lib()
    for rows, segs, k in ((0, 1, 1), (65238, 1, 10), (2 * evaluate.TOPK_CHUNK + 1, 3, 128), (16_700_928, 256, 100)):
        slots = rows // evaluate.TOPK_CHUNK + segs                 # the bound the grid is sized from
        assert L.digat_topk_segments_workspace_bytes(rows, segs, k) >= slots * k * 12


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    rows, segs = 100, 3
    need = L.digat_topk_segments_workspace_bytes(rows, segs, 10)
    assert need > 0

    def call(scores=p, start=p, rows=rows, segs=segs, ids=p, skip=p, skip_len=5, k=10, out_s=p, out_i=p, out_c=p, ws=p, ws_bytes=need):
        return L.digat_topk_segments(scores, start, rows, segs, ids, skip, skip_len, k, out_s, out_i, out_c, ws, ws_bytes, None)
    assert call(k=0) == ARG
    assert call(k=129) == ARG
    assert call(skip_len=257) == ARG
    assert call(skip_len=-1) == ARG
    assert call(ids=None) == ARG                                   # skip without ids
    assert call(scores=None) == ARG
    for name in ("start", "out_s", "out_i", "out_c", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(rows=-1) == ARG and call(segs=-1) == ARG
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(k=128) == WORKSPACE                                # sized for k = 10
    assert call(segs=0) == OK
    assert call(segs=0, rows=0, ws=None, ws_bytes=0) == OK


# ---------------------------------------------------------------------------------------------------------------------
# topk_segments_host against sorted() over Python tuples
# ---------------------------------------------------------------------------------------------------------------------
def brute_force(scores, start, k, ids, skip):
    """Per segment: elements whose id is not skipped, sorted by (NaN last, score descending, position ascending) as tuples."""
    out = []
    for s in range(len(start) - 1):
        a, b = int(start[s]), int(start[s + 1])
        banned = set() if skip is None else set(int(v) for v in skip[s])
        elems = []
        for pos in range(b - a):
            ident = pos if ids is None else int(ids[a + pos])
            if ids is not None and ident in banned:
                continue
            x = float(scores[a + pos])
            elems.append((1, 0.0, pos, ident) if math.isnan(x) else (0, -x, pos, ident))      # -(-0.0) == 0.0 == -(0.0): equal
        elems.sort()
        out.append([(a + e[2], e[3]) for e in elems[:k]])
    return out


def special_segment(rng, n):
    vals = np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5], dtype=np.float32)
    return vals[rng.integers(0, len(vals), size=n)]


def make_case(rng, segments=300, max_len=40):
    lens = rng.integers(0, max_len + 1, size=segments)
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    scores = (rng.integers(0, 4, size=int(start[-1])) * 0.25 - 0.5).astype(np.float32)         # four values
    for s in range(segments):
        a, b = start[s], start[s + 1]
        if s % 7 == 3:
            scores[a:b] = special_segment(rng, b - a)
        if s % 7 == 5 and b > a:
            scores[a:b][rng.integers(0, 2, size=b - a) == 1] = np.nan
            if b - a > 2:
                scores[a + 1] = np.float32(struct.unpack("f", struct.pack("I", 0xFFC00001))[0])   # a negative NaN with a payload
    return scores, start


def check_against_brute_force(scores, start, k, ids, skip):
    from digat_amd import evaluate
    got_s, got_i, got_c = evaluate.topk_segments_host(scores, start, k, ids=ids, skip=skip)
    want = brute_force(scores, start, k, ids, skip)
    assert got_s.shape == got_i.shape == (len(start) - 1, k) and got_s.dtype == np.float32 and got_i.dtype == np.int64
    assert got_c.dtype == np.int32
    for s, w in enumerate(want):
        assert got_c[s] == len(w), s
        assert list(got_i[s, :len(w)]) == [e[1] for e in w], s
        assert got_s[s, :len(w)].view(np.uint32).tolist() == scores[[e[0] for e in w]].view(np.uint32).tolist(), s    # original bits
        assert np.all(np.isneginf(got_s[s, len(w):])) and np.all(got_i[s, len(w):] == -1), s


@pytest.mark.parametrize("k", [1, 3, 10, 128])
def test_host_topk_matches_sorted_tuples(k):
    rng = np.random.default_rng(100 + k)
    scores, start = make_case(rng)
    assert np.isnan(scores).any() and np.isinf(scores).any() and (scores.view(np.uint32) == 0x80000000).any()
    check_against_brute_force(scores, start, k, None, None)


@pytest.mark.parametrize("k", [1, 5])
def test_host_topk_with_ids_and_skip_rows(k):
    rng = np.random.default_rng(200 + k)
    scores, start = make_case(rng, segments=200, max_len=30)
    S = len(start) - 1
    ids = rng.integers(0, 2 ** 40, size=len(scores)).astype(np.int64)
    ids[rng.integers(0, len(ids), size=len(ids) // 5)] = 7                      # repeated ids: distinct elements, skipped together
    skip = rng.integers(2 ** 41, 2 ** 42, size=(S, 6)).astype(np.int64)        # ids nobody has ...
    best_removed = fewer_than_k = everything = 0
    for s in range(S):
        a, b = int(start[s]), int(start[s + 1])
        if b == a:
            continue
        top = brute_force(scores, start, 1, ids, None)[s][0]
        if s % 3 == 0:                                                         # ... the best element's id
            skip[s, 2] = top[1]
            best_removed += 1
        elif s % 3 == 1 and b - a <= 6:                                        # ... every id of the segment
            skip[s, :b - a] = ids[a:b]
            everything += 1
        elif s % 3 == 2 and b - a > 1:                                         # ... all but at most k - 1 (when k > 1) or all but one
            keep = max(1, k - 1)
            drop = ids[a:b][:max(0, b - a - keep)][:6]
            skip[s, :len(drop)] = drop
            fewer_than_k += 1
    assert best_removed and fewer_than_k and everything
    got = None
    from digat_amd import evaluate
    got = evaluate.topk_segments_host(scores, start, k, ids=ids, skip=skip)
    for s in range(0, S, 3):
        a, b = int(start[s]), int(start[s + 1])
        if b > a:
            top = brute_force(scores, start, 1, ids, None)[s][0]
            assert top[1] not in got[1][s], s
    check_against_brute_force(scores, start, k, ids, skip)


def test_keys_order_as_the_contract_says():
    from digat_amd import evaluate
    x = np.array([np.nan, -np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32)
    key = evaluate.topk_keys(x).astype(np.int64)
    assert key[0] == 1 and key[4] == key[5]
    assert np.all(np.diff(np.delete(key, 4)) > 0)
    assert not (key == 0).any()                                    # 0 is "not an element" in the kernel


def test_host_topk_refuses_bad_arguments():
    from digat_amd import evaluate
    sc, st = np.zeros(4, dtype=np.float32), np.array([0, 4])
    for k in (0, 129):
        with pytest.raises(ValueError):
            evaluate.topk_segments_host(sc, st, k)
    with pytest.raises(ValueError):
        evaluate.topk_segments_host(sc, st, 2, skip=np.zeros((1, 3), dtype=np.int64))          # skip without ids
    with pytest.raises(ValueError):
        evaluate.topk_segments_host(sc, st, 2, ids=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        evaluate.topk_segments_host(sc, st, 2, ids=np.zeros(4, dtype=np.int64), skip=np.zeros((1, 257), dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# util.recommend: argument checks and the row builder, on host tensors
# ---------------------------------------------------------------------------------------------------------------------
def host_corpus(I=5, H=4, C=3, news_num=20, table=True):
    from digat_amd import util
    rng = np.random.default_rng(0)
    U = H + C
    return util.DeviceCorpus(
        news_embedding=torch.zeros(news_num, 8), news_node_ID=torch.zeros(news_num, 2, dtype=torch.int64),
        news_graph=torch.zeros(news_num, 2, 2, dtype=torch.bool), news_graph_mask=torch.zeros(news_num, 2, dtype=torch.bool),
        history=torch.from_numpy(rng.integers(0, news_num, size=(I, H))), user_graph=torch.zeros(I, U, U, dtype=torch.bool) if table else None,
        user_category_mask=torch.zeros(I, C + 1, dtype=torch.bool) if table else None,
        user_category_indices=torch.from_numpy(rng.integers(0, C + 1, size=(I, H))), row_impression=torch.zeros(0, dtype=torch.int64),
        row_candidate=torch.zeros(0, dtype=torch.int64), category_num=C)


def test_recommend_refuses_bad_arguments_before_it_touches_the_model():
    from digat_amd import util
    dc = host_corpus()
    model = types.SimpleNamespace()                    # no attribute may be needed to refuse
    pool = np.arange(1, 20)
    for k in (0, 129, -3):
        with pytest.raises(ValueError, match="k must be"):
            util.recommend(model, dc, np.array([0, 1]), pool, k)
    with pytest.raises(ValueError, match="max_history_num"):                                   # H mismatch
        util.recommend(model, dc, (np.zeros((2, 5), dtype=np.int64), np.zeros((2, 5), dtype=np.int64)), pool, 3)
    with pytest.raises(ValueError, match="history"):                                           # the pair's shapes differ
        util.recommend(model, dc, (np.zeros((2, 4), dtype=np.int64), np.zeros((3, 4), dtype=np.int64)), pool, 3)
    with pytest.raises(ValueError, match="impression indices"):
        util.recommend(model, dc, np.array([0, 5]), pool, 3)
    with pytest.raises(ValueError, match="last candidate start"):                              # a CSR whose last start is not R
        util.recommend(model, dc, np.array([0, 1]), (np.arange(1, 8), np.array([0, 3, 6])), 3)
    with pytest.raises(ValueError, match="users \\+ 1"):
        util.recommend(model, dc, np.array([0, 1]), (np.arange(1, 8), np.array([0, 7])), 3)
    with pytest.raises(ValueError, match="never decrease"):
        util.recommend(model, dc, np.array([0, 1]), (np.arange(1, 8), np.array([0, 9, 7])), 3)
    for bad in (np.array([1, 20]), np.array([-1, 2])):                                         # ids outside [0, news_num)
        with pytest.raises(ValueError, match="candidate ids"):
            util.recommend(model, dc, np.array([0, 1]), bad, 3)
    with pytest.raises(ValueError, match="candidates must be"):
        util.recommend(model, dc, np.array([0, 1]), np.zeros((2, 2), dtype=np.int64), 3)
    with pytest.raises(ValueError, match="max_rows"):
        util.recommend(model, dc, np.array([0, 1]), pool, 3, max_rows=0)


def test_recommend_users_takes_indices_or_arrays():
    from digat_amd import util
    dc = host_corpus()
    idx = np.array([3, 0, 3])
    hist, cat, graph, mask = util.recommend_users(dc, idx)
    assert torch.equal(hist, dc.history[[3, 0, 3]]) and torch.equal(cat, dc.user_category_indices[[3, 0, 3]])
    assert tuple(graph.shape) == (3, 7, 7) and tuple(mask.shape) == (3, 4)
    hist2, cat2, graph2, mask2 = util.recommend_users(dc, (hist.numpy(), cat.numpy()))
    assert torch.equal(hist2, hist) and torch.equal(cat2, cat) and graph2 is None and mask2 is None       # derived on the device
    derived = host_corpus(table=False)
    assert util.recommend_users(derived, idx)[2:] == (None, None)


def test_row_builder_shared_pool_and_csr():
    from digat_amd import util
    pool, _ = util.recommend_candidates(np.array([4, 9, 2]), users=5, news_num=20)
    imp, cand, seg = util.recommend_rows(1, 4, pool, None)
    assert imp.tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3] and cand.tolist() == [4, 9, 2] * 3 and seg.tolist() == [0, 3, 6, 9]
    assert imp.dtype == cand.dtype == seg.dtype == torch.int64
    ids, start = util.recommend_candidates((np.array([5, 6, 7, 8, 9, 10]), np.array([0, 2, 2, 5, 6])), users=4, news_num=20)
    imp, cand, seg = util.recommend_rows(0, 4, ids, start)
    assert imp.tolist() == [0, 0, 2, 2, 2, 3] and cand.tolist() == [5, 6, 7, 8, 9, 10] and seg.tolist() == [0, 2, 2, 5, 6]
    imp, cand, seg = util.recommend_rows(1, 3, ids, start)                                        # an empty user, then three pairs
    assert imp.tolist() == [2, 2, 2] and cand.tolist() == [7, 8, 9] and seg.tolist() == [0, 0, 3]
    imp, cand, seg = util.recommend_rows(2, 2, ids, start)
    assert imp.numel() == 0 and cand.numel() == 0 and seg.tolist() == [0]


def test_user_chunks_respect_max_rows():
    from digat_amd import util
    assert util.recommend_user_chunks(7, 10, None, 30) == [(0, 3), (3, 6), (6, 7)]
    assert util.recommend_user_chunks(3, 10, None, 5) == [(0, 1), (1, 2), (2, 3)]              # one user's pool exceeds it: one user
    assert util.recommend_user_chunks(0, 10, None, 5) == []
    start = np.array([0, 4, 4, 9, 30, 31])
    chunks = util.recommend_user_chunks(5, 31, start, 10)
    assert chunks == [(0, 3), (3, 4), (4, 5)]
    assert chunks[0][0] == 0 and chunks[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert util.RECOMMEND_MAX_ROWS * 20 == 80 << 20                                             # the bytes the docstring states


@pytest.mark.parametrize("with_skip", [False, True])
def test_select_driver_is_chunk_invariant_and_matches_the_host_selection(with_skip):
    """``util.recommend_select`` over host scores (routed to ``topk_segments_host``): whatever ``max_rows`` cuts the users into, the
    ids, score bits, counts and fills are those of one selection over all pairs at once."""
    from digat_amd import evaluate, util
    lens = [0, 1, 5, 0, 12, 3, 9]
    G, k = len(lens), 4
    rng = np.random.default_rng(5)
    ids = torch.from_numpy(rng.integers(0, 40, size=sum(lens)))
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    skip = torch.from_numpy(rng.integers(0, 40, size=(G, 6))) if with_skip else None
    seen = []

    def score(g0, g1, row_user, row_cand):                      # a fixed function of (user, candidate), three values: many ties
        seen.append((g0, g1, int(row_user.shape[0])))
        return ((row_user * 7 + row_cand) % 3).to(torch.float32) * 0.5 - 0.5
    row_user, row_cand, seg = util.recommend_rows(0, G, ids, start)
    want_s, want_i, want_c = evaluate.topk_segments_host(score(0, G, row_user, row_cand).numpy(), seg.numpy(), k, ids=row_cand.numpy(),
                                                         skip=None if skip is None else skip.numpy())
    assert want_c.tolist()[0] == 0 and want_c.tolist()[3] == 0 and (want_c < k).any() and (want_c == k).any()
    if with_skip:
        assert want_c.sum() < evaluate.topk_segments_host(np.zeros(sum(lens), dtype=np.float32), start, k)[2].sum()   # the rows bite
    for max_rows in (1, 4, 1000):
        del seen[:]
        got_i, got_s, got_c = util.recommend_select(G, k, ids, start, skip, max_rows, score)
        assert got_i.dtype == torch.int64 and got_s.dtype == torch.float32 and got_c.dtype == torch.int32
        assert np.array_equal(got_i.numpy(), want_i) and np.array_equal(got_c.numpy(), want_c), max_rows
        assert np.array_equal(got_s.numpy().view(np.uint32), want_s.view(np.uint32)), max_rows          # fills included
        assert all(r > 0 for _, _, r in seen), "an empty chunk was scored"
        assert all(r <= max_rows or g1 - g0 == 1 for g0, g1, r in seen) and (len(seen) == 1) == (max_rows == 1000)


def test_config_parses_the_recommend_mode():
    from digat_amd.config import Config
    c = Config(["--mode", "recommend", "--recommend_k", "5"])
    assert c.mode == "recommend" and c.recommend_k == 5 and c.recommend_output == ""
    assert Config([]).recommend_k == 10
