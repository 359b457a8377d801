"""CPU suite of exposure-capped top-k: the host contract (``evaluate.capped_select_host``, the round-wise form) against a
plain-Python deferred acceptance that makes ONE proposal at a time in a scrambled order (uniqueness: any schedule reaches the same
assignment) and against a brute-force search for a blocking pair (stability, feasibility) on every case the GPU suite compares
exactly (tests/capped_common.py: same generator, same seeds); the reductions and tie rules the contract states; ``util.recommend`` /
``nrms.recommend`` with ``exposure_cap=`` on CPU tensors; the library's refusals and symbols; the CLI flag."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import capped_common as K
import dot_topk_common as D
import test_calibrate_cpu as TC
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_capped_select_workspace_bytes", "digat_capped_prepare", "digat_capped_rounds", "digat_capped_emit")


def _keys(inputs, P):
    """``(elem [G,M] bool, ks, kp [G,M] int64)``: the element test and the two keys, written out once more."""
    from digat_amd import evaluate
    ids, scores, count, pr = inputs
    G, M = ids.shape
    ks = evaluate.topk_keys(scores).reshape(G, M).astype(np.int64)
    kp = ks if pr is None else evaluate.topk_keys(pr).reshape(G, M).astype(np.int64)
    cnt = np.full(G, M) if count is None else np.clip(np.asarray(count, dtype=np.int64), 0, M)
    elem = (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < P)
    elem &= ~np.isnan(scores) & ~np.isneginf(scores)
    if pr is not None:
        elem &= ~np.isnan(pr)
    return elem, ks, kp


def serial_deferred_acceptance(inputs, k, caps, P, rng):
    """Deferred acceptance, the lists proposing, one proposal at a time, the proposer drawn at random among the lists that hold
    fewer than k and have entries left to propose: ``held[g]`` = the set of slots list g ends up holding."""
    ids = inputs[0]
    elem, ks, kp = _keys(inputs, P)
    G, M = ids.shape
    pref = [sorted(np.flatnonzero(elem[g]).tolist(), key=lambda j: (-ks[g, j], j)) for g in range(G)]
    nxt, held = [0] * G, [set() for _ in range(G)]
    holders = {}                                                     # news -> [(item's order of the pair, g, slot)], best first
    active = [g for g in range(G) if pref[g]]
    while active:
        at = int(rng.integers(len(active)))
        g = active[at]
        j = pref[g][nxt[g]]
        nxt[g] += 1
        news = int(ids[g, j])
        if caps[news] > 0:
            h = holders.setdefault(news, [])
            h.append(((-kp[g, j], g, j), g, j))
            held[g].add(j)
            if len(h) > caps[news]:
                h.sort()
                _, g2, j2 = h.pop()
                held[g2].discard(j2)
                if g2 != g and g2 not in active and nxt[g2] < len(pref[g2]):
                    active.append(g2)
        if len(held[g]) >= k or nxt[g] >= len(pref[g]):
            active.remove(g)
    return held


def check_result(inputs, capv, k, P, got):
    """Feasibility, the outputs' form, and no blocking pair, by brute force over every pair of the call."""
    from digat_amd import evaluate
    ids, scores, count, pr = inputs
    out_i, out_s, out_c, out_p, rounds = got
    G, M = ids.shape
    elem, ks, kp = _keys(inputs, P)
    caps = evaluate.capped_caps_host(capv, P).astype(np.int64)
    assert out_i.dtype == np.int64 and out_s.dtype == np.float32 and out_c.dtype == np.int32 and out_p.dtype == np.int32
    assert out_i.shape == out_s.shape == out_p.shape == (G, k) and out_c.shape == (G,) and rounds >= 1
    filled = np.arange(k)[None, :] < out_c[:, None]
    assert (out_i[~filled] == -1).all() and np.isneginf(out_s[~filled]).all() and (out_p[~filled] == -1).all()
    assert (out_p[filled] >= 0).all() and (out_p[filled] < M).all()
    gi, qi = np.nonzero(filled)
    sl = out_p[gi, qi]
    assert np.array_equal(out_i[gi, qi], ids[gi, sl]) and np.array_equal(K.bits(out_s[gi, qi]), K.bits(scores[gi, sl]))
    held = np.zeros((G, M), dtype=bool)
    held[gi, sl] = True
    assert held.sum() == filled.sum(), "no slot twice"
    assert not (held & ~elem).any(), "only elements are held"
    lval = ks * 2048 + (2047 - np.arange(M)[None, :])                # a list's order of its entries: larger first
    row = np.where(filled, lval[np.arange(G)[:, None], np.clip(out_p, 0, M - 1)], -1)
    assert (row[:, 1:] < row[:, :-1])[filled[:, 1:]].all(), "held entries in the list's order"
    ival = kp * (G * M) + (G * M - 1 - np.arange(G * M).reshape(G, M))           # an item's order of its pairs: larger first
    n_item = np.bincount(ids[held], minlength=P)
    assert (n_item <= np.maximum(caps, 0)).all(), "no news beyond its capacity"
    assert (held.sum(axis=1) <= k).all()
    worst_l = np.where(held, lval, np.iinfo(np.int64).max).min(axis=1)
    list_wants = elem & ~held & ((held.sum(axis=1)[:, None] < k) | (lval > worst_l[:, None]))
    worst_i = np.full(P, np.iinfo(np.int64).max)
    np.minimum.at(worst_i, ids[held], ival[held])
    safe = np.where(elem, ids, 0)
    item_wants = elem & (caps[safe] > 0) & ((n_item[safe] < caps[safe]) | (ival > worst_i[safe]))
    assert not (list_wants & item_wants).any(), ("a blocking pair", np.argwhere(list_wants & item_wants)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# capped_select_host: uniqueness and stability
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priority", [False, True])
@pytest.mark.parametrize("cap", K.CAPS)
@pytest.mark.parametrize("G,M,k,P", K.CASES)
def test_every_shared_case_is_stable_and_feasible(G, M, k, P, cap, priority):
    inputs, capv, want = K.case(G, M, k, P, cap, priority)
    check_result(inputs, capv, k, P, want)


@pytest.mark.parametrize("priority", [False, True])
@pytest.mark.parametrize("cap", K.CAPS)
@pytest.mark.parametrize("G,M,k,P", [c for c in K.CASES if c[0] <= 65 and c[1] <= 257])
def test_twin_is_the_serial_deferred_acceptance_in_any_proposal_order(G, M, k, P, cap, priority):
    from digat_amd import evaluate
    inputs, capv, want = K.case(G, M, k, P, cap, priority)
    caps = evaluate.capped_caps_host(capv, P)
    for scramble in (0, 1):
        held = serial_deferred_acceptance(inputs, k, caps, P, np.random.default_rng(scramble))
        for g in range(G):
            assert held[g] == set(want[3][g, :want[2][g]].tolist()), (g, scramble)


def test_small_random_calls_against_the_serial_loop_and_brute_force():
    from digat_amd import evaluate
    seen_short = seen_full = 0
    for seed in range(40):
        rng = np.random.default_rng(900 + seed)
        G, M, k, P = int(rng.integers(1, 9)), int(rng.integers(1, 13)), int(rng.integers(1, 5)), int(rng.integers(1, 10))
        inputs = K.make_lists(seed, G, M, P, priority=bool(seed % 2))
        capv = K.make_cap(seed, "array" if seed % 3 == 0 else int(rng.integers(0, 4)), P)
        got = evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], k, capv, P, priority=inputs[3])
        check_result(inputs, capv, k, P, got)
        held = serial_deferred_acceptance(inputs, k, evaluate.capped_caps_host(capv, P), P, rng)
        assert [set(got[3][g, :got[2][g]].tolist()) for g in range(G)] == held, seed
        seen_short += int((got[2] < k).any())
        seen_full += int((got[2] == k).any())
    assert seen_short >= 10 and seen_full >= 10


# ---------------------------------------------------------------------------------------------------------------------
# reductions and tie rules
# ---------------------------------------------------------------------------------------------------------------------
def _elements_topk(inputs, P, k, drop=None):
    """``shortlist_segments_host``'s top-k of every list's elements (without news ``drop``): ``(scores, ids, count)``."""
    from digat_amd import evaluate
    ids, scores = inputs[0], inputs[1]
    elem, _, _ = _keys(inputs, P)
    if drop is not None:
        elem = elem & (ids != drop)
    start = np.concatenate([[0], np.cumsum(elem.sum(axis=1))]).astype(np.int64)
    return evaluate.shortlist_segments_host(scores[elem], start, k, ids=ids[elem])


@pytest.mark.parametrize("G,M,k,P", [(3, 63, 10, 40), (65, 64, 10, 50), (33, 257, 10, 300), (65, 1024, 128, 1500)])
def test_a_cap_of_G_is_the_plain_topk_and_a_cap_of_zero_blocks_a_news(G, M, k, P):
    from digat_amd import evaluate
    inputs = K.make_lists(K.seed_of(G, M, k, P), G, M, P)
    for cap in (G, G + 5, np.full(P, G, dtype=np.int32)):
        i, s, c, p, rounds = evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], k, cap, P)
        ws, wi, wc = _elements_topk(inputs, P, k)
        assert rounds == 1 and np.array_equal(i, wi) and np.array_equal(K.bits(s), K.bits(ws)) and np.array_equal(c, wc)
    assert int(c[1]) == 0 and (i[1] == -1).all(), "the empty list"
    block = np.full(P, G, dtype=np.int32)
    block[1] = 0                                                     # the news every list names in slot 0
    i, s, c, p, rounds = evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], k, block, P)
    ws, wi, wc = _elements_topk(inputs, P, k, drop=1)
    assert not (i == 1).any() and np.array_equal(i, wi) and np.array_equal(K.bits(s), K.bits(ws)) and np.array_equal(c, wc)
    nothing = evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], k, 0, P)
    assert (nothing[2] == 0).all() and (nothing[0] == -1).all() and np.isneginf(nothing[1]).all() and (nothing[3] == -1).all()
    empty = evaluate.capped_select_host(inputs[0], inputs[1], np.zeros(G, dtype=np.int32), k, 1, P)
    assert (empty[2] == 0).all() and empty[4] == 1


def test_tie_rules_and_priority():
    from digat_amd import evaluate
    f32 = lambda x: np.array(x, dtype=np.float32)
    i64 = lambda x: np.array(x, dtype=np.int64)
    # equal scores go by slot; -0 equals +0
    i, s, c, p, _ = evaluate.capped_select_host(i64([[5, 6, 7, 8]]), f32([[1, 1, 1, 2]]), None, 3, 9, 10)
    assert i.tolist() == [[8, 5, 6]] and p.tolist() == [[3, 0, 1]]
    i, *_ = evaluate.capped_select_host(i64([[5, 6]]), f32([[-0.0, 0.0]]), None, 1, 9, 10)
    assert i.tolist() == [[5]]
    # equal priorities go by g
    ids, sc = i64([[4], [4], [4]]), f32([[1], [1], [1]])
    assert evaluate.capped_select_host(ids, sc, None, 1, 1, 5)[2].tolist() == [1, 0, 0]
    assert evaluate.capped_select_host(ids, sc, None, 1, 2, 5)[2].tolist() == [1, 1, 0]
    # a higher score takes a contested news; the loser moves on
    ids, sc = i64([[4, 5], [4, 6]]), f32([[2, 1], [3, 1]])
    i, s, c, p, rounds = evaluate.capped_select_host(ids, sc, None, 1, 1, 7)
    assert i.tolist() == [[5], [4]] and s.tolist() == [[1.0], [3.0]] and rounds == 2
    # a given priority changes who keeps it — never the feasibility
    i, s, c, p, rounds = evaluate.capped_select_host(ids, sc, None, 1, 1, 7, priority=f32([[9, 0], [1, 0]]))
    assert i.tolist() == [[4], [6]] and s.tolist() == [[2.0], [1.0]]
    # a NaN priority is no element; -inf priority is one, the last its item takes
    i, *_ = evaluate.capped_select_host(ids, sc, None, 1, 1, 7, priority=f32([[np.nan, 0], [-np.inf, 0]]))
    assert i.tolist() == [[5], [4]]
    # a list that names one news twice holds two pairs, and both count against the capacity
    i, s, c, p, _ = evaluate.capped_select_host(i64([[4, 4, 5]]), f32([[1, 2, 0]]), None, 3, 2, 7)
    assert i.tolist() == [[4, 4, 5]] and p.tolist() == [[1, 0, 2]]
    i, s, c, p, _ = evaluate.capped_select_host(i64([[4, 4, 5]]), f32([[1, 2, 0]]), None, 3, 1, 7)
    assert i.tolist() == [[4, 5, -1]] and p.tolist() == [[1, 2, -1]], "by priority = score the better pair stays"
    # ... at equal priorities the item goes by slot, whatever the list's own order of the two
    i, s, c, p, _ = evaluate.capped_select_host(i64([[4, 4, 5]]), f32([[1, 2, 0]]), None, 3, 1, 7, priority=f32([[7, 7, 7]]))
    assert p.tolist() == [[0, 2, -1]] and s.tolist()[0][:2] == [1.0, 0.0]


def test_host_refuses_bad_arguments():
    from digat_amd import evaluate
    ids, scores, count, _ = K.make_lists(0, 4, 20, 30)
    call = lambda **kw: evaluate.capped_select_host(**{**dict(ids=ids, scores=scores, count=count, k=5, cap=2, pool=30), **kw})
    call()
    for bad, match in ((dict(k=0), "k must be"), (dict(k=129), "k must be"), (dict(cap=-1), "cap must"), (dict(cap=1.5), "cap must"),
                       (dict(cap=np.zeros(29, np.int32)), "cap must"), (dict(cap=np.zeros(30, np.float32)), "cap must"),
                       (dict(pool=-1), "pool must"), (dict(pool=2 ** 31), "pool must"), (dict(scores=scores[:, :5]), r"\[G, M\]"),
                       (dict(count=count[:2]), "count must"), (dict(priority=scores[:2]), "priority must"), (dict(max_rounds=0), "max_rounds"),
                       (dict(ids=np.zeros((4, 1025), np.int64), scores=np.zeros((4, 1025), np.float32)), r"\[G, M\]")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    inputs, capv, want = K.case(33, 257, 10, 300, 1)
    assert want[4] > 2
    with pytest.raises(RuntimeError, match="max_rounds"):
        evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], 10, capv, 300, max_rounds=want[4] - 1)
    assert evaluate.CAP_MAX_LIST == evaluate.SHORTLIST_MAX_K == 1024 and evaluate.CAP_MAX_K == 128
    assert evaluate.CAP_ROUNDS_PER_SYNC == 4 and evaluate.CAP_MAX_ROUNDS == 1024


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
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
    assert int(re.search(r"#define\s+DIGAT_CAPPED_MAX_LIST\s+(\d+)", header).group(1)) == 1024
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    for before in ("digat_topk.inc", "digat_shortlist.inc", "digat_mmr.inc"):                    # topk_key, short_bitonic, sel_count
        assert hip.index('#include "%s"' % before) < hip.index('#include "digat_capped.inc"')
    # words (8), order (2), rejected and demand (1 each) per pair, every block rounded up to 256 bytes
    up = lambda x: (x + 255) // 256 * 256
    for G, M in ((1, 1), (65, 65), (300, 1024), (4096, 1024)):
        assert L.digat_capped_select_workspace_bytes(G, M) == up(G * M * 8) + up(G * M * 2) + 2 * up(G * M)
    assert L.digat_capped_select_workspace_bytes(0, 64) == 0


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 4096)()                     # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    need = L.digat_capped_select_workspace_bytes(3, 16)

    def prepare(ids=p, scores=p, priority=p, count=p, G=3, M=16, P=100, ws=p, nbytes=need):
        return L.digat_capped_prepare(ids, scores, priority, count, G, M, P, ws, nbytes, None)

    def rounds(G=3, M=16, k=10, perm=p, begin=p, cap=p, live=p, n_seg=2, counter=p, n=4, ws=p, nbytes=need):
        return L.digat_capped_rounds(G, M, k, perm, begin, cap, live, n_seg, counter, n, ws, nbytes, None)

    def emit(ids=p, scores=p, G=3, M=16, k=10, out_i=p, out_s=p, out_c=p, out_p=p, ws=p, nbytes=need):
        return L.digat_capped_emit(ids, scores, G, M, k, out_i, out_s, out_c, out_p, ws, nbytes, None)

    for name in ("ids", "scores", "ws"):
        assert prepare(**{name: None}) == ARG, name
    assert prepare(G=-1) == ARG and prepare(P=-1) == ARG and prepare(ws=p + 4) == ARG
    assert prepare(P=1 << 31) == SHAPE and prepare(G=1 << 31) == SHAPE and prepare(G=1 << 22, M=1024) == SHAPE
    for M in (0, -1, 1025):
        assert prepare(M=M) == SHAPE and rounds(M=M) == SHAPE and emit(M=M) == SHAPE, M
    assert prepare(nbytes=need - 1) == WORKSPACE and rounds(nbytes=need - 1) == WORKSPACE and emit(nbytes=need - 1) == WORKSPACE
    assert prepare(G=0, ws=None, nbytes=0) == OK and rounds(G=0, ws=None, nbytes=0) == OK and emit(G=0, ws=None, nbytes=0) == OK
    for name in ("perm", "begin", "cap", "live", "counter", "ws"):
        assert rounds(**{name: None}) == ARG, name
    assert rounds(n_seg=-1) == ARG and rounds(n=-1) == ARG and rounds(G=-1) == ARG
    for k in (0, -1, 129):
        assert rounds(k=k) == SHAPE and emit(k=k) == SHAPE, k
    for name in ("ids", "scores", "out_i", "out_s", "out_c", "out_p", "ws"):
        assert emit(**{name: None}) == ARG, name


# ---------------------------------------------------------------------------------------------------------------------
# recommend(exposure_cap=) on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def popular_scoring(monkeypatch):
    """``TC.fake_scoring`` with a popularity term all users share, on a grid of 1/8: the users contend for the same few news and
    exact ties between users are met."""
    from digat_amd import util

    def score_rows(model, view, start, end, batch_size, *a, **kw):
        cand, user = view.row_candidate.to(torch.float32), view.row_impression.to(torch.float32)
        return torch.round((2 * torch.cos(cand * 0.7) + 0.5 * torch.sin(user * 37 + cand * 11)) * 8) / 8
    monkeypatch.setattr(util, "score_rows", score_rows)
    monkeypatch.setattr(util, "refresh_news_side", lambda model, dc, batch_size: None)


def test_util_recommend_with_exposure_cap_is_the_selection_then_the_twin(monkeypatch):
    from digat_amd import evaluate, util
    popular_scoring(monkeypatch)
    dc, model = TC.host_corpus(), types.SimpleNamespace()
    users, pool, k, N = np.array([0, 3, 4, 1, 2, 5]), np.arange(1, 300), 5, 300
    plain = util.recommend(model, dc, users, pool, k)
    again = util.recommend(model, dc, users, pool, k, exposure_cap=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), "exposure_cap=None is the call without the keyword"
    per_news = np.random.default_rng(4).integers(0, 3, size=N).astype(np.int32)
    for cap, shortlist in ((1, None), (2, 200), (1, 8), (len(users), None), (per_news, None), (torch.from_numpy(per_news), 30)):
        wide = shortlist or min(1024, 8 * k)
        i, s, c = util.recommend_lists(model, dc, users, pool, wide)
        capv = cap.numpy() if torch.is_tensor(cap) else cap
        want = evaluate.capped_select_host(i.numpy(), s.numpy(), c.numpy(), k, capv, N)
        got = util.recommend(model, dc, users, pool, k, exposure_cap=cap, shortlist=shortlist)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
        K.same(tuple(got) + (want[3], want[4]), want, (shortlist,))
        stage = util.cap_exposure(i, s, c, k, cap, N)
        K.same(stage, want, "cap_exposure")
        shown = np.bincount(got[0].numpy()[got[0].numpy() >= 0], minlength=N)
        assert (shown <= evaluate.capped_caps_host(capv, N)).all()
        if np.ndim(capv) == 0 and capv == len(users):
            assert all(torch.equal(a, b) for a, b in zip(got, plain)), "a cap of G: the plain list"
        if np.ndim(capv) == 0 and capv == 1 and shortlist is None:
            assert shown.max() == 1 and np.bincount(plain[0].numpy().reshape(-1)).max() > 1, "the cap binds on this corpus"
        # the users in several chunks: the stage still sees all lists together
        for kw in (dict(batch_size=2), dict(max_rows=700), dict(batch_size=3, max_rows=300)):
            chunked = util.recommend(model, dc, users, pool, k, exposure_cap=cap, shortlist=shortlist, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, chunked)), kw
    # a priority of the caller's, through the stage
    i, s, c = util.recommend_lists(model, dc, users, pool, 40)
    pr = torch.from_numpy(np.random.default_rng(1).standard_normal((len(users), 40)).astype(np.float32))
    K.same(util.cap_exposure(i, s, c, k, 1, N, priority=pr), evaluate.capped_select_host(i.numpy(), s.numpy(), c.numpy(), k, 1, N, pr.numpy()), "priority")
    # every refusal, before anything is scored
    def never(*a, **kw):
        raise AssertionError("scored before the refusal")
    monkeypatch.setattr(util, "score_rows", never)
    for bad in (dict(diversity=0.3), dict(calibration=0.3), dict(rerank=(0.2, 0.2)), dict(sample=1.0), dict(max_per_category=2),
                dict(category=np.zeros(N, np.int32)), dict(calibration_target=np.zeros((6, 4), np.float32)), dict(shortlist=4),
                dict(shortlist=1025)):
        with pytest.raises(ValueError):
            util.recommend(model, dc, users, pool, k, exposure_cap=2, **bad)
    for cap in (-1, 1.5, np.zeros(N - 1, np.int32), np.zeros(N, np.float32), torch.zeros(N)):
        with pytest.raises(ValueError, match="exposure_cap|cap must"):
            util.recommend(model, dc, users, pool, k, exposure_cap=cap)
    with pytest.raises(ValueError, match="k must be"):
        util.recommend(model, dc, users, pool, 129, exposure_cap=2)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_recommend_with_exposure_cap_is_the_selection_then_the_twin(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), D.dev_set()
    users, k = np.arange(D.USERS), 4
    plain = nrms.recommend(m, dev, users, k=k)
    again = nrms.recommend(m, dev, users, k=k, exposure_cap=None)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    for cap, shortlist in ((1, None), (2, 60), (D.USERS, None)):
        i, s, c = nrms.recommend(m, dev, users, k=shortlist or 8 * k)
        want = evaluate.capped_select_host(i.numpy(), s.numpy(), c.numpy(), k, cap, D.NEWS)
        got = nrms.recommend(m, dev, users, k=k, exposure_cap=cap, shortlist=shortlist)
        K.same(tuple(got) + (want[3], want[4]), want, (pre, cap, shortlist))
        if cap == D.USERS:
            assert all(torch.equal(a, b) for a, b in zip(got, plain))
    for bad in (dict(diversity=0.3), dict(calibration=0.3), dict(rerank=(0.1, 0.1)), dict(sample=1.0), dict(max_per_category=1),
                dict(index=object()), dict(refine=64)):
        with pytest.raises(ValueError):
            nrms.recommend(m, dev, users, k=k, exposure_cap=1, **bad)


# ---------------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_config_parses_the_exposure_cap_flag(capsys):
    from digat_amd.config import Config
    c = Config(["--mode", "recommend"])
    assert not hasattr(c, "recommend_exposure_cap") and not hasattr(c, "recommend_shortlist"), "off: no attribute"
    c = Config(["--mode", "recommend", "--recommend_exposure_cap", "13"])
    assert c.recommend_exposure_cap == 13 and c.recommend_shortlist == 0
    assert not hasattr(c, "recommend_diversity") and not hasattr(c, "recommend_max_per_category") and not hasattr(c, "recommend_calibration")
    c = Config(["--mode", "recommend", "--recommend_exposure_cap", "0", "--recommend_shortlist", "1024"])
    assert c.recommend_exposure_cap == 0 and c.recommend_shortlist == 1024
    c = Config(["--mode", "recommend", "--recommend_calibration", "0.5"])
    assert not hasattr(c, "recommend_exposure_cap")
    for bad, text in ((["--recommend_exposure_cap", "-1"], "must not be negative"),
                      (["--recommend_exposure_cap", "3", "--recommend_diversity", "0.3"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_calibration", "0.3"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_sample", "1.0"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_rerank", "0.2,0.2"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_report", "0,0.1"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_max_per_category", "2"], "does not combine"),
                      (["--recommend_exposure_cap", "3", "--recommend_shortlist", "-1"], "must not be negative")):
        with pytest.raises(SystemExit):
            Config(["--mode", "recommend"] + bad)
        assert text in capsys.readouterr().err, bad


def test_recommend_lines_passes_the_cap_on(monkeypatch):
    from digat_amd import main
    popular_scoring(monkeypatch)
    dc, model = TC.host_corpus(), types.SimpleNamespace()
    lines = main.recommend_lines(model, dc, 5, 64, exposure_cap=1)
    plain = main.recommend_lines(model, dc, 5, 64)
    shown = [int(v) for line in lines for v in line.split("[")[1].rstrip("]").split(",") if v]
    assert len(lines) == len(plain) == 6 and len(shown) == len(set(shown)) == 30 and lines != plain
