"""CPU suite: retrieval training without a GPU — the full-pool softmax entries are declared, exported and refuse bad arguments before
any launch; their workspace holds nothing the size of the score matrix; the host contracts ``evaluate.pool_softmax_host`` / ``pool_softmax_grad_host`` against
float64 ``torch.autograd`` on the stock composition; the CPU path of ``evaluate.pool_softmax``; ``nrms.retrieval_loss`` and
``nrms.fit_retriever`` on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dot_rank_common as R
import dot_topk_common as D
import pool_softmax_common as PS
from conftest import REPO

OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
NEW = ("digat_pool_softmax_workspace_bytes", "digat_pool_softmax_fwd", "digat_pool_softmax_bwd")


def test_new_symbols_are_declared_exported_and_bound():
    from digat_amd import _lib, build, evaluate
    build.build(verbose=False)
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/digat_hip.h"
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.digat_version() == _lib.ABI_VERSION == 4, "new exports only: the ABI version stays"
    hip = open(os.path.join(REPO, "digat_amd", "csrc", "digat_kernels.hip")).read()
    assert hip.index('#include "digat_dot_rank.inc"') < hip.index('#include "digat_pool_softmax.inc"')      # it uses rank_tile_starts
    inc = open(os.path.join(REPO, "digat_amd", "csrc", "digat_pool_softmax.inc")).read()
    assert "atomicAdd" not in inc, "no floating-point atomics: every sum has a fixed order"
    assert re.search(r"#define\s+PSM_MAX_D\s+(\d+)", inc).group(1) == str(evaluate.POOL_SOFTMAX_MAX_D)


def _formula(G, P, T, d):
    """include/digat_hip.h: every region rounded up to 256 bytes."""
    from digat_amd import evaluate
    up = lambda n: -(-n // 256) * 256
    tiles, chunks = -(-G // evaluate.DOT_TOPK_USERS), -(-P // evaluate.DOT_TOPK_CHUNK)
    return (3 * up(4 * T) + up(8 * T) + up(8 * G * chunks) + up(4 * G) + up(4 * tiles) + up(256 * d * min(tiles * chunks, 256 + tiles)))


def test_workspace_query_has_no_score_matrix_in_it():
    from digat_amd import _lib, evaluate
    q = _lib.lib().digat_pool_softmax_workspace_bytes
    ch = evaluate.DOT_TOPK_CHUNK
    assert q(-1, 10, 10, 8) == 0 and q(10, -1, 10, 8) == 0 and q(10, 10, -1, 8) == 0 and q(10, 10, 10, 0) == 0 and q(10, 10, 10, -3) == 0
    for shape in ((1, 1, 1, 1), (64, 65237, 64, 400), (4096, 65237, 5 * 4096, 400), (3, 2 * ch + 1, 6147, 36), (100000, 70000, 100000, 512)):
        assert q(*shape) == _formula(*shape), shape
    users_axis = [q(u, 5000, 100, 64) for u in (0, 1, 63, 64, 65, 200, 4096, 16384, 16385, 20000, 1 << 20)]
    pool_axis = [q(100, p, 100, 64) for p in (0, 1, ch - 1, ch, ch + 1, 2 * ch + 1, 65237, 1 << 24)]
    target_axis = [q(100, 5000, t, 64) for t in (0, 1, 63, 64, 65, 1000, 1 << 20)]
    d_axis = [q(100, 5000, 100, d) for d in (1, 5, 64, 65, 400, 512, 513, 4096)]
    for axis in (users_axis, pool_axis, target_axis, d_axis):
        assert all(a <= b for a, b in zip(axis, axis[1:])), axis
    big = q(4096, 65237, 4096, 400)
    assert big < 64 << 20 and 16 * big < 4096 * 65237 * 4, "a sixteenth of the matrix it replaces"
    # nothing the size of the matrix: per (user, position) there is 8 / 2048 of a byte, the pair of a user's chunk
    assert q(1 << 20, 1 << 24, 1 << 20, 400) < (1 << 20) * (1 << 24) * 4 // 512


def test_bad_arguments_are_refused_before_any_launch():
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    buf = (C.c_int64 * 64)()                       # host memory: every call below must return before it would launch
    p = C.addressof(buf)
    G, N, P, T, d = 5, 300, 100, 12, 20
    need = L.digat_pool_softmax_workspace_bytes(G, P, T, d)
    assert need > 0

    def fwd(users=p, news=p, pool=p, G=G, N=N, P=P, d=d, skip=p, skip_len=5, pos=p, start=p, T=T, loss=p, lse=p, score=p, ws=p, ws_bytes=need):
        return L.digat_pool_softmax_fwd(users, news, pool, G, N, P, d, skip, skip_len, pos, start, T, 1.0, loss, lse, score, ws, ws_bytes, None)

    def bwd(users=p, news=p, pool=p, G=G, N=N, P=P, d=d, skip=p, skip_len=5, pos=p, start=p, T=T, lse=p, gl=p, du=p, dr=p, ws=p, ws_bytes=need):
        return L.digat_pool_softmax_bwd(users, news, pool, G, N, P, d, skip, skip_len, pos, start, T, 1.0, lse, gl, du, dr, ws, ws_bytes, None)
    for call, own in ((fwd, ("loss", "lse", "score")), (bwd, ("lse", "gl", "du", "dr"))):
        for name in ("users", "news", "pos", "start", "ws") + own:
            assert call(**{name: None}) == ARG, (call.__name__, name)
        assert call(G=-1) == ARG and call(N=-1) == ARG and call(P=-1) == ARG and call(T=-1) == ARG
        assert call(d=0) == ARG and call(d=-4) == ARG
        for skip_len in (-1, 257):
            assert call(skip_len=skip_len) == ARG, skip_len
        assert call(pool=None) == ARG                                   # no pool: P must be N
        assert call(ws=p + 4) == ARG                                    # 8-byte alignment
        assert call(ws_bytes=need - 1) == WORKSPACE
        assert call(T=1 << 20) == WORKSPACE                             # sized for 12 targets
        assert call(G=1 << 40, P=1 << 40, ws_bytes=1 << 62) == SHAPE
        assert call(T=1 << 31, ws_bytes=1 << 62) == SHAPE
        assert call(G=0, T=0, P=0, N=0, ws=None, ws_bytes=0) == OK      # nobody, nothing: no workspace, no launch
    assert bwd(d=516, ws_bytes=1 << 62) == SHAPE and bwd(d=512, ws_bytes=need - 1) == WORKSPACE, "the backward takes d <= 512"
    assert fwd(d=516, ws_bytes=need) == WORKSPACE, "the forward takes any d (here: it gets as far as the workspace check)"


def _host_cases():
    """(users, news, pool, skip, pos, start, scale, news_num): with and without a pool, with repeats and ids outside the table, skip
    rows, users with 0 / 1 / several targets, a repeated target, a target inside the skip row, a user with no element."""
    rng = np.random.default_rng(17)
    G, d = 6, 7
    out = []
    for pooled, skipped, scale in ((False, False, 1.0), (True, False, 0.5), (False, True, 2.0), (True, True, 1.3)):
        P = 23
        N = 40 if pooled else P
        users = rng.standard_normal((G, d))
        news = rng.standard_normal((N, d))
        pool = None
        if pooled:
            pool = rng.integers(0, N, size=P).astype(np.int64)
            pool[3] = pool[11]                                      # a repeated id
            pool[5], pool[7] = N + 2, -4                            # ids that are no rows
        ids = np.arange(P, dtype=np.int64) if pool is None else pool
        skip = None
        if skipped:
            skip = np.stack([ids[rng.integers(0, P, size=9)] for _ in range(G)])
            skip[4, :] = -1
            skip[4, :min(9, P)] = ids[:9]
            skip = np.concatenate([skip, np.full((G, P), -1, dtype=np.int64)], axis=1)
            skip[4, 9:9 + P] = ids                                  # user 4: every id skipped — no element
        pos = np.array([2, 2, 9,            # user 0: a repeated target
                        0,                  # user 1: one
                        # user 2: none
                        5, 7, -1, P, 22,    # user 3: ids outside the table (with a pool), positions outside the pool
                        1, 3,               # user 4
                        4, 4, 4, 10],       # user 5: three times the same
                       dtype=np.int64)
        start = np.array([0, 3, 4, 4, 9, 11, 15], dtype=np.int64)
        if skipped:
            hit = np.flatnonzero(ids == skip[0, 0])
            pos[2] = hit[0]                                         # user 0: a target inside its skip row
        out.append((users, news, pool, skip, pos, start, scale, N))
    return out


@pytest.mark.parametrize("n", range(4))
def test_host_functions_match_float64_autograd(n):
    from digat_amd import evaluate
    users, news, pool, skip, pos, start, scale, N = _host_cases()[n]
    rng = np.random.default_rng(n)
    gl = rng.standard_normal(len(pos))
    w_loss, w_lse, w_ranked, w_dU, w_dR = PS.stock_fp64(users, news, pos, start, pool, skip, scale, gl)
    ids = np.arange(len(news)) if pool is None else pool
    ok = (ids >= 0) & (ids < N)
    rows = np.zeros((len(ids), users.shape[1]))
    rows[ok] = news[ids[ok]]
    S = users @ rows.T
    loss, lse, ranked = evaluate.pool_softmax_host(S, pos, start, pool=pool, skip=skip, news_num=N, scale=scale)
    dU, dR = evaluate.pool_softmax_grad_host(users, rows, S, pos, start, pool=pool, skip=skip, news_num=N, scale=scale, grad_loss=gl)
    assert loss.dtype == lse.dtype == dU.dtype == dR.dtype == np.float64 and ranked.dtype == bool
    assert np.array_equal(ranked, w_ranked)
    assert not ranked[[6, 7]].any() and ranked.any() and (loss[~ranked] == 0).all()
    if pool is not None:
        assert not ranked[4] and not ranked[5], "ids outside the table are no elements"
        assert (dR[5] == 0).all() and (dR[7] == 0).all()
    else:
        assert ranked[[0, 1, 3]].all() if skip is None else True
    if skip is not None:
        assert not ranked[2] and np.isneginf(lse[4]) and not ranked[9:11].any() and (dU[4] == 0).all()
    assert np.array_equal(np.isneginf(lse), np.isneginf(w_lse))
    fin = np.isfinite(w_lse)
    for got, want, what in ((lse[fin], w_lse[fin], "lse"), (loss, w_loss, "loss"), (dU, w_dU, "d_users"), (dR, w_dR, "d_rows")):
        scale_ = max(float(np.abs(want).max()), 1e-300)
        assert np.abs(got - want).max() <= 1e-12 * scale_, (what, float(np.abs(got - want).max()), scale_)
    assert (dU[2] == 0).all(), "a user without a target contributes exactly zero"
    # grad_loss None is ones; the grad_loss of a target that is not ranked is ignored
    ones = evaluate.pool_softmax_grad_host(users, rows, S, pos, start, pool=pool, skip=skip, news_num=N, scale=scale)
    g1 = np.ones(len(pos))
    g1[~ranked] = 1e9
    same = evaluate.pool_softmax_grad_host(users, rows, S, pos, start, pool=pool, skip=skip, news_num=N, scale=scale, grad_loss=g1)
    assert np.array_equal(ones[0], same[0]) and np.array_equal(ones[1], same[1])
    with pytest.raises(ValueError, match="target_start"):
        evaluate.pool_softmax_host(S, pos, start[:-1])
    with pytest.raises(ValueError, match="scores must be"):
        evaluate.pool_softmax_host(S[0], pos, start)


@pytest.mark.parametrize("n", range(4))
def test_cpu_path_of_pool_softmax_agrees_with_the_host_and_is_differentiable(n):
    from digat_amd import evaluate
    users, news, pool, skip, pos, start, scale, N = _host_cases()[n]
    if pool is not None:
        pool = np.clip(pool, 0, N - 1)                              # the Python entry refuses ids outside the table
        if skip is not None:
            skip = np.where(np.isin(skip, pool) | (skip < 0), skip, -1)
    rng = np.random.default_rng(n)
    gl = rng.standard_normal(len(pos)).astype(np.float32)
    U = torch.tensor(users, dtype=torch.float32, requires_grad=True)
    V = torch.tensor(news, dtype=torch.float32, requires_grad=True)
    tp = lambda x: None if x is None else torch.from_numpy(x)
    loss, lse, score = evaluate.pool_softmax(U, V, pos, start, pool=tp(pool), skip=tp(skip), scale=scale)
    assert loss.requires_grad and not lse.requires_grad and not score.requires_grad
    (loss * torch.from_numpy(gl)).sum().backward()
    rows = news if pool is None else news[pool]
    S = (U.detach().double() @ torch.tensor(rows).float().double().t()).numpy()
    w_loss, w_lse, ranked = evaluate.pool_softmax_host(S, pos, start, pool=pool, skip=skip, scale=scale)
    w_dU, w_dR = evaluate.pool_softmax_grad_host(U.detach().numpy(), V.detach().numpy()[np.arange(len(news)) if pool is None else pool], S,
                                                 pos, start, pool=pool, skip=skip, scale=scale, grad_loss=gl)
    w_dV = np.zeros(news.shape)
    np.add.at(w_dV, np.arange(len(news)) if pool is None else pool, w_dR)
    assert np.array_equal(np.isnan(score.numpy()), ~ranked)
    np.testing.assert_allclose(score.numpy()[ranked], S[np.repeat(np.arange(len(users)), np.diff(start))[ranked], pos[ranked]], rtol=1e-5, atol=1e-5)
    fin = np.isfinite(w_lse)
    assert np.array_equal(np.isneginf(lse.numpy()), ~fin)
    np.testing.assert_allclose(lse.numpy()[fin], w_lse[fin], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss.detach().numpy(), w_loss, rtol=1e-5, atol=1e-5)
    assert np.isfinite(U.grad.numpy()).all() and np.isfinite(V.grad.numpy()).all()
    np.testing.assert_allclose(U.grad.numpy(), w_dU, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(V.grad.numpy(), w_dV, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError, match="target_pos"):
        evaluate.pool_softmax(U, V, pos.astype(np.float32), start, pool=tp(pool))
    with pytest.raises(ValueError, match="target_start"):
        evaluate.pool_softmax(U, V, pos, start[1:], pool=tp(pool))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_retrieval_loss_is_the_host_contract_on_the_stock_scores(pre):
    from digat_amd import evaluate, nrms
    m, dev = D.model(pre), R.dev_with_rows()
    inp = D.inputs()
    got = nrms.retrieval_loss(m, dev, scale=0.8)
    S = D.stock_scores(m, D.dev_set())                              # [users, news]
    pool = np.arange(1, D.NEWS, dtype=np.int64)
    tid = inp["candidate_ids"].reshape(-1)
    start = np.arange(D.USERS + 1, dtype=np.int64) * R.CANDS
    skip = np.where(inp["history_mask"] != 0, inp["history_ids"], 0)
    w_loss, w_lse, ranked = evaluate.pool_softmax_host(S[:, 1:], tid - 1, start, pool=pool, skip=skip, scale=0.8)
    assert got["targets"] == len(tid) and got["users"] == D.USERS and got["not_ranked"] == int((~ranked).sum()) > 0
    # the stock scores are float32 and depend in their last bits on how the encoders were batched: equal to their resolution
    for batched in (got, nrms.retrieval_loss(m, dev, batch_size=4, scale=0.8)):
        np.testing.assert_allclose(batched["loss"], w_loss, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(batched["lse"], w_lse, rtol=1e-6, atol=1e-6)
        assert (batched["loss"][~ranked] == 0).all() and batched["not_ranked"] == got["not_ranked"]
        assert batched["nll"] == float(batched["loss"][ranked].mean())
    rank = nrms.retrieval_metrics(m, dev)["rank"]
    assert np.array_equal(rank >= 0, ranked), "ranked here exactly where retrieval_metrics ranks"
    some = nrms.retrieval_loss(m, dev, users=np.array([2, 5]), targets=(np.array([3, 4, 9]), np.array([0, 1, 3])), candidates=np.arange(1, 40))
    assert some["targets"] == 3 and some["users"] == 2 and some["loss"].shape == (3,) and some["lse"].shape == (2,)
    with pytest.raises(ValueError, match="one pool"):
        nrms.retrieval_loss(m, dev, users=np.array([2, 5]), targets=(np.array([3, 4, 9]), np.array([0, 1, 3])),
                            candidates=(np.array([3, 4, 9, 1]), np.array([0, 2, 4])))


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_fit_retriever_lowers_the_retrieval_loss_and_is_reproducible(pre):
    from digat_amd import nrms
    dev = R.dev_with_rows()
    before = nrms.retrieval_loss(D.model(pre), dev)["nll"]
    runs = []
    for _ in range(2):
        m = D.model(pre)
        losses = nrms.fit_retriever(m, dev, steps=6, batch_users=D.USERS, lr=2e-3, seed=5)
        assert m.training and len(losses) == 6 and all(np.isfinite(losses))
        runs.append((losses, nrms.retrieval_loss(m, dev)["nll"]))
    assert runs[0] == runs[1], "one seed, one result"
    print(pre, "retrieval loss before", before, "after", runs[0][1], "per step", runs[0][0])
    assert runs[0][1] < before
    assert abs(runs[0][0][0] - before) <= 1e-4 * abs(before), "dropout 0: the first step's loss is the loss before"
    # a sampled pool never holds row 0, holds the batch's targets, and another seed draws other steps
    other = nrms.fit_retriever(D.model(pre), dev, steps=3, batch_users=4, pool_size=20, seed=6)
    again = nrms.fit_retriever(D.model(pre), dev, steps=3, batch_users=4, pool_size=20, seed=6)
    third = nrms.fit_retriever(D.model(pre), dev, steps=3, batch_users=4, pool_size=20, seed=7)
    assert other == again and other != third
