"""GPU suite: the fused full-pool softmax loss (``digat_pool_softmax_fwd`` / ``_bwd``, ``evaluate.pool_softmax``) and
``nrms.retrieval_step`` / ``retrieval_loss`` on it.  What is a matter of bits — the targets' scores, which targets are ranked, that two
calls and two groupings of the users agree — is held exactly; ``lse`` and ``loss`` to the float64 host contract on the kernel's own
scores (``digat_dot_scores``) at the bound the kernel file derives; the gradients at the training tolerance 2e-4."""
import functools

import numpy as np
import pytest
import torch

import dot_rank_common as R
import dot_topk_common as D
import nrms_common as NC
import pool_softmax_common as C
from nrms_common import close

pytestmark = pytest.mark.gpu

# G in {1, 64, 65, 130}, P in {1, 63, 65, 2047, 2049, 4100}, d in {1, 5, 32, 36, 400, 512}
SWEEP = ((1, 1, 1), (1, 63, 5), (64, 65, 32), (65, 63, 36), (65, 2047, 5), (130, 2049, 32), (1, 4100, 400), (64, 2049, 400),
         (130, 65, 512), (65, 4100, 36), (1, 2047, 512), (130, 1, 1))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def test_the_sweep_covers_what_it_should():
    from digat_amd import evaluate
    ch, sub, tile = evaluate.DOT_TOPK_CHUNK, evaluate.DOT_TOPK_SUB, evaluate.DOT_TOPK_USERS
    assert {g for g, _, _ in SWEEP} == {1, tile, tile + 1, 2 * tile + 2}
    assert {p for _, p, _ in SWEEP} == {1, sub - 1, sub + 1, ch - 1, ch + 1, 2 * ch + 4}
    assert {d for _, _, d in SWEEP} == {1, 5, 32, 36, 400, evaluate.POOL_SOFTMAX_MAX_D}


def _run(users, news, pos, start, pool, skip, scale, gl):
    """One forward and backward on the device: ``(loss, lse, score, d_users, d_news)`` as numpy."""
    from digat_amd import evaluate
    U, V = _t(users).requires_grad_(True), _t(news).requires_grad_(True)
    loss, lse, score = evaluate.pool_softmax(U, V, _t(pos), start, pool=_t(pool), skip=_t(skip), scale=scale)
    assert loss.dtype == lse.dtype == score.dtype == torch.float32
    assert loss.shape == score.shape == (len(pos),) and lse.shape == (len(users),)
    assert loss.requires_grad and not lse.requires_grad and not score.requires_grad
    (loss * _t(gl)).sum().backward()
    return tuple(t.detach().cpu().numpy() for t in (loss, lse, score, U.grad, V.grad))


def _close_grad(got, want, cancelled, what):
    """The training tolerance, ``close(rtol=2e-4, atol=0)``: relative to the gradient's own size.  Where the exact gradient is
    IDENTICALLY zero — a pool of one element: its softmax is 1 and cancels the targets whatever the vectors are — it has no size of
    its own; it is the difference of two equal sums, c x row and the sum of grad_loss x row, and is held at the same rtol to their
    size ``cancelled`` (no fp32 evaluation, stock PyTorch's included, cancels sums of rounded terms to exactly zero)."""
    if np.abs(want).max() > 0:
        close(torch.from_numpy(got), want, what, rtol=2e-4, atol=0.0)
    else:
        assert np.isfinite(got).all() and np.abs(got).max() <= 2e-4 * cancelled, (what, float(np.abs(got).max()), cancelled)


def _check(users, news, pos, start, pool, skip, scale, rng, what):
    """The whole contract of one call against the host functions on ``dot_scores``."""
    from digat_amd import evaluate
    gl = rng.standard_normal(len(pos)).astype(np.float32)
    loss, lse, score, dU, dV = _run(users, news, pos, start, pool, skip, scale, gl)
    S = evaluate.dot_scores(_t(users), _t(news), pool=_t(pool)).cpu().numpy()
    rank = evaluate.dot_rank(_t(users), _t(news), _t(pos), start, pool=_t(pool), skip=_t(skip))[0].cpu().numpy()
    w_loss, w_lse, ranked = evaluate.pool_softmax_host(S, pos, start, pool=pool, skip=skip, scale=scale)
    owner = np.repeat(np.arange(len(users)), np.diff(start))
    # bits
    assert np.array_equal(ranked, rank >= 0), what
    assert np.array_equal(np.isnan(score), rank < 0), (what, "NaN exactly where dot_rank gives -1")
    assert np.array_equal(_bits(score[ranked]), _bits(S[owner[ranked], pos[ranked]])), (what, "score bits")
    assert (loss[~ranked] == 0).all(), what
    # lse and loss at the derived bound, which is inside the project's output tolerance
    none = np.isneginf(w_lse)
    assert np.array_equal(np.isneginf(lse), none), what
    x = scale * S.astype(np.float64)
    x_max = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(users))
    P = S.shape[1]
    if (~none).any():
        b_lse = evaluate.pool_softmax_bound(P, w_lse[~none], x_max[~none])
        err = np.abs(lse[~none] - w_lse[~none])
        print(what, "lse: worst error over bound", float((err / b_lse).max()), "largest bound", float(b_lse.max()))
        tol = 2e-6 + 1e-5 * np.maximum(np.abs(w_lse[~none]), 0.05 * np.abs(w_lse[~none]).max())
        assert (b_lse <= tol).all(), (what, "the bound is looser than the output tolerance")
        assert (err <= b_lse).all(), (what, float((err / b_lse).max()))
        close(torch.from_numpy(lse[~none]), w_lse[~none], f"{what} lse")
    if ranked.any():
        g = owner[ranked]
        b_loss = evaluate.pool_softmax_bound(P, w_lse[g], x_max[g], x[g, pos[ranked]], w_loss[ranked])
        err = np.abs(loss[ranked] - w_loss[ranked])
        print(what, "loss: worst error over bound", float((err / b_loss).max()), "largest bound", float(b_loss.max()))
        assert (err <= b_loss).all(), (what, float((err / b_loss).max()))
    # gradients at the training tolerance
    w_dU, w_dR = evaluate.pool_softmax_grad_host(users, C.rows_of(news, pool), S, pos, start, pool=pool, skip=skip, scale=scale, grad_loss=gl)
    w_dV = w_dR
    if pool is not None:
        w_dV = np.zeros((len(news), users.shape[1]))
        np.add.at(w_dV, pool, w_dR)
    per_user = np.bincount(owner, weights=np.abs(gl) * ranked, minlength=len(users)).max() if len(pos) else 0.0
    _close_grad(dU, w_dU, abs(scale) * per_user * np.abs(news).max(), f"{what} d_users")
    _close_grad(dV, w_dV, abs(scale) * per_user * np.abs(users).max(), f"{what} d_news")
    return loss, lse, score, dU, dV


@pytest.mark.parametrize("G,P,d", SWEEP)
def test_loss_and_gradients_against_the_host_contract(G, P, d):
    from digat_amd import evaluate
    rng = np.random.default_rng(1000 * G + P + d)
    n = SWEEP.index((G, P, d))
    for pool in (False, True):
        for skip in (False, True):
            users, news, pl, sk = C.case(rng, G, P, d, pool, skip)
            users *= np.float32(1.5 / np.sqrt(d))                  # scores of a few units: a softmax that is neither flat nor one-hot
            pos, start = C.targets(rng, G, P, sk, pl, evaluate.DOT_TOPK_CHUNK, rot=n)
            _check(users, news, pos, start, pl, sk, 1.0 if n % 2 else 0.7, rng, (G, P, d, pool, skip))
            n += 1


def test_targets_that_are_no_elements_and_users_without_any():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(9)
    G, N, d = 4, 500, 20
    u = rng.standard_normal((G, d)).astype(np.float32)
    v = rng.standard_normal((N, d)).astype(np.float32)
    few = rng.permutation(N)[:40].astype(np.int64)
    P = len(few)
    skip = rng.integers(0, N, size=(G, 64)).astype(np.int64)
    skip[0], skip[0, 7] = few[4], few[17]                           # user 0: positions 4 and 17 skipped, nothing else
    skip[1, :40], skip[1, 40:] = few, few[0]                        # user 1: every id skipped: no element, lse -inf
    pos = np.r_[np.array([3, 4, 5, -1, 16, 17, 18, P, 0, P - 1, -(1 << 40), 1 << 40, 3, 3]), np.arange(P), np.array([4, 17, 2, 9, 5])].astype(np.int64)
    start = np.array([0, 14, 14 + P, 14 + P + 5, 14 + P + 5], dtype=np.int64)      # user 3 has no target
    loss, lse, score, dU, dV = _check(u, v, pos, start, few, skip, 1.0, rng, "skipped, out of range")
    assert np.isneginf(lse[1]) and np.isfinite(lse[[0, 2, 3]]).all()
    assert np.isnan(score[[1, 3, 5, 7, 10, 11]]).all() and np.isnan(score[14:14 + P]).all()
    assert (dU[1] == 0).all() and (dU[3] == 0).all(), "a user without a ranked target contributes exactly zero"
    assert np.isfinite(dU).all() and np.isfinite(dV).all()
    # pool ids outside [0, N): the Python entry refuses them, the C entry treats them as no element and writes every byte
    pool = few.copy()
    pool[5], pool[9] = N, -3
    with pytest.raises(ValueError, match="pool ids"):
        evaluate.pool_softmax(_t(u), _t(v), _t(pos), start, pool=_t(pool))
    L = _lib.lib()
    U, V, PL, SK, TP, ST = _t(u), _t(v), _t(pool), _t(skip), _t(pos), _t(start)
    T = len(pos)
    need = int(L.digat_pool_softmax_workspace_bytes(G, P, T, d))
    ws = _lib.workspace(need, _dev(), "pool_softmax")
    ws.fill_(0xFF)
    f = dict(dtype=torch.float32, device=_dev())
    o_loss, o_lse, o_sc = torch.full((T + 8,), 77.0, **f), torch.full((G + 8,), 77.0, **f), torch.full((T + 8,), 77.0, **f)
    head = (U.data_ptr(), V.data_ptr(), PL.data_ptr(), G, N, P, d, SK.data_ptr(), 64, TP.data_ptr(), ST.data_ptr(), T, 1.0)
    _lib.check(L.digat_pool_softmax_fwd(*head, o_loss.data_ptr(), o_lse.data_ptr(), o_sc.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()),
               "digat_pool_softmax_fwd")
    S2 = evaluate.dot_scores(U, V, pool=_t(few)).cpu().numpy()      # the scores of positions 5 and 9 are never read
    w_loss, w_lse, ranked = evaluate.pool_softmax_host(S2, pos, start, pool=pool, skip=skip, news_num=N)
    assert not ranked[2] and not ranked[14 + P + 3] and not ranked[14 + P + 4]
    assert (o_loss[T:] == 77).all() and (o_lse[G:] == 77).all() and (o_sc[T:] == 77).all(), "nothing is written beyond the arrays"
    assert np.array_equal(np.isnan(o_sc[:T].cpu().numpy()), ~ranked)
    fin = np.isfinite(w_lse)
    close(o_lse[:G][torch.from_numpy(fin).to(_dev())], w_lse[fin], "lse with ids outside the table")
    close(o_loss[:T], w_loss, "loss with ids outside the table")
    gl = torch.ones(T, **f)
    dU2, dR2 = torch.full((G + 1, d), 77.0, **f), torch.full((P + 1, d), 77.0, **f)
    _lib.check(L.digat_pool_softmax_bwd(*head, o_lse.data_ptr(), gl.data_ptr(), dU2.data_ptr(), dR2.data_ptr(), ws.data_ptr(), need,
                                        _lib.stream_ptr()), "digat_pool_softmax_bwd")
    rows = np.zeros((P, d))
    ok = (pool >= 0) & (pool < N)
    rows[ok] = v[pool[ok]]
    w_dU, w_dR = evaluate.pool_softmax_grad_host(u, rows, S2, pos, start, pool=pool, skip=skip, news_num=N)
    assert (dU2[G:] == 77).all() and (dR2[P:] == 77).all()
    close(dU2[:G], w_dU, "d_users with ids outside the table", rtol=2e-4, atol=0.0)
    close(dR2[:P], w_dR, "d_rows with ids outside the table", rtol=2e-4, atol=0.0)
    assert (dR2[5] == 0).all() and (dR2[9] == 0).all()
    # malformed offsets: wrong numbers at most, every byte written, nothing outside
    bad = _t(np.array([5, 1 << 40, -7, 3, T], dtype=np.int64))
    head_bad = head[:10] + (bad.data_ptr(),) + head[11:]
    o_loss.fill_(77.0)
    o_sc.fill_(77.0)
    _lib.check(L.digat_pool_softmax_fwd(*head_bad, o_loss.data_ptr(), o_lse.data_ptr(), o_sc.data_ptr(), ws.data_ptr(), need,
                                        _lib.stream_ptr()), "digat_pool_softmax_fwd")
    torch.cuda.synchronize()
    assert (o_loss[:T] != 77).all() and (o_sc[:T] != 77).all() and (o_loss[T:] == 77).all() and (o_sc[T:] == 77).all()


def test_two_calls_and_a_tile_alone_give_the_same_bits():
    from digat_amd import evaluate
    rng = np.random.default_rng(31)
    G, P, d = 130, 2049, 36
    users, news, pl, sk = C.case(rng, G, P, d, True, False)
    pl = rng.permutation(len(news))[:P].astype(np.int64)            # no repeated id: the gradient of the news is d_rows, row for row
    sk = np.stack([pl[rng.integers(0, P, size=50)] for _ in range(G)])
    pos, start = C.targets(rng, G, P, sk, pl, evaluate.DOT_TOPK_CHUNK, per_user=(1, 5, 0, 7))
    gl = rng.standard_normal(len(pos)).astype(np.float32)
    first = _run(users, news, pos, start, pl, sk, 0.3, gl)
    again = _run(users, news, pos, start, pl, sk, 0.3, gl)
    for a, b, name in zip(first, again, ("loss", "lse", "target_score", "d_users", "d_news")):
        assert np.array_equal(_bits(a), _bits(b)), name
    # the second tile of users alone: the same lse and loss bits (the gradient of the news is another sum and is not compared)
    g0, g1 = 64, 128
    t0, t1 = int(start[g0]), int(start[g1])
    alone = _run(users[g0:g1], news, pos[t0:t1], start[g0:g1 + 1] - t0, pl, sk[g0:g1], 0.3, gl[t0:t1])
    assert np.array_equal(_bits(alone[0]), _bits(first[0][t0:t1])) and np.array_equal(_bits(alone[1]), _bits(first[1][g0:g1]))
    # one user alone, moved to the front of a tile: still the same bits
    g = 69                                                          # five targets
    t0, t1 = int(start[g]), int(start[g + 1])
    one = _run(users[g:g + 1], news, pos[t0:t1], np.array([0, t1 - t0]), pl, sk[g:g + 1], 0.3, gl[t0:t1])
    assert np.array_equal(_bits(one[0]), _bits(first[0][t0:t1])) and np.array_equal(_bits(one[1]), _bits(first[1][g:g + 1]))


def test_scores_of_three_hundred_stay_finite():
    """x reaches +-300: exp(x) overflows fp32 (and exp(-x) underflows) unless the maximum is subtracted."""
    from digat_amd import evaluate
    rng = np.random.default_rng(77)
    G, P, d = 65, 2049, 32
    users, news, pl, sk = C.case(rng, G, P, d, True, True)
    S = users.astype(np.float64) @ news[pl].astype(np.float64).T
    scale = float(300.0 / np.abs(S).max())
    pos, start = C.targets(rng, G, P, sk, pl, evaluate.DOT_TOPK_CHUNK, per_user=(1, 5))
    loss, lse, score, dU, dV = _check(users, news, pos, start, pl, sk, scale, rng, "range")
    assert np.abs(lse).max() > 200 and np.isfinite(loss).all() and np.isfinite(dU).all() and np.isfinite(dV).all()


def test_wide_vectors_forward_only():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    G, P, d = 3, 130, evaluate.POOL_SOFTMAX_MAX_D + 4
    users, news, pl, sk = C.case(rng, G, P, d, True, True)
    users *= np.float32(1.5 / np.sqrt(d))
    pos, start = C.targets(rng, G, P, sk, pl, evaluate.DOT_TOPK_CHUNK, per_user=(5,))
    U, V = _t(users).requires_grad_(True), _t(news)
    loss, lse, score = evaluate.pool_softmax(U, V, _t(pos), start, pool=_t(pl), skip=_t(sk))
    S = evaluate.dot_scores(_t(users), V, pool=_t(pl)).cpu().numpy()
    w_loss, w_lse, ranked = evaluate.pool_softmax_host(S, pos, start, pool=pl, skip=sk)
    close(lse, w_lse, "wide lse")
    close(loss, w_loss, "wide loss")
    with pytest.raises(ValueError, match=str(evaluate.POOL_SOFTMAX_MAX_D)):
        loss.sum().backward()


def test_refusals_and_empty_calls():
    from digat_amd import evaluate
    rng = np.random.default_rng(13)
    G, P, d = 5, 70, 8
    users, news, pl, sk = C.case(rng, G, P, d, True, True)
    pos, start = C.targets(rng, G, P, sk, pl, evaluate.DOT_TOPK_CHUNK, per_user=(2,))
    U, V, PL, SK, TP = _t(users), _t(news), _t(pl), _t(sk), _t(pos)
    with pytest.raises(ValueError, match="target_start"):
        evaluate.pool_softmax(U, V, TP, start[:-1], pool=PL)
    with pytest.raises(ValueError, match="target_pos"):
        evaluate.pool_softmax(U, V, TP.float(), start, pool=PL)
    with pytest.raises(ValueError, match="share d"):
        evaluate.pool_softmax(U, V[:, :5], TP, start)
    with pytest.raises(ValueError, match="skip must be"):
        evaluate.pool_softmax(U, V, TP, start, pool=PL, skip=SK[:2])
    # no target at all: lse is still computed, the gradients are zero
    Ug = U.clone().requires_grad_(True)
    loss, lse, score = evaluate.pool_softmax(Ug, V, TP[:0], np.zeros(G + 1, dtype=np.int64), pool=PL, skip=SK)
    S = evaluate.dot_scores(U, V, pool=PL).cpu().numpy()
    close(lse, evaluate.pool_softmax_host(S, pos[:0], np.zeros(G + 1, dtype=np.int64), pool=pl, skip=sk)[1], "lse without targets")
    loss.sum().backward()
    assert loss.shape == (0,) and (Ug.grad == 0).all()
    # an empty pool: nothing is an element
    none = evaluate.pool_softmax(U, V, TP, start, pool=PL[:0])
    assert (none[0] == 0).all() and torch.isneginf(none[1]).all() and torch.isnan(none[2]).all()


STEP_FIXTURE = "nrms_train_tiny.npz"      # on nrms_train_default.npz the stock fp32 step itself is 4.9 tolerances from its fp64 twin


def _train_set(name, device="cpu"):
    """The training fixture's impressions with the first candidate of each clicked, as the fixture's own click loss has it.  Its user
    encoder's attention is sharpened (``user_qk_gain``) so that fp32 holds every gradient to the training tolerance — the stock fp32
    step itself misses 2e-4 on the pooling parameters of ``dot_topk_common``'s model, whose gradients there are differences of nearly
    equal numbers."""
    dev = NC.dev_set(name, device)
    U, K = NC.case(name)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U


@functools.lru_cache(maxsize=None)
def _step_reference(name, pre, exclude):
    """The retrieval step on a float64 CPU copy through forward_stock and the stock composition: (loss, {parameter: gradient})."""
    from digat_amd import nrms
    m = C.double_twin(NC.model(name, pre))
    m.train()
    dev, U = _train_set(name)
    loss = nrms.retrieval_step(m, dev, np.arange(U), exclude_history=exclude)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("pre", list(NC.MODELS))
@pytest.mark.parametrize("exclude", [True, False])
def test_nrms_retrieval_step_on_the_device(exclude, pre):
    from digat_amd import nrms
    name = STEP_FIXTURE
    want_loss, want = _step_reference(name, pre, exclude)
    m = NC.model(name, pre, _dev())
    m.train()
    dev, U = _train_set(name, _dev())
    loss = nrms.retrieval_step(m, dev, np.arange(U), exclude_history=exclude)
    loss.backward()
    close(loss, np.float64(want_loss), f"{pre} retrieval loss", rtol=2e-5, atol=1e-5)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, want[k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)


@pytest.mark.parametrize("pre", list(D.MODELS))
def test_nrms_retrieval_loss_on_the_device(pre):
    from digat_amd import nrms
    got = nrms.retrieval_loss(D.model(pre, _dev()), R.dev_with_rows(_dev()), batch_size=4)
    cpu = nrms.retrieval_loss(D.model(pre), R.dev_with_rows())
    assert got["targets"] == cpu["targets"] == D.USERS * R.CANDS and got["not_ranked"] == cpu["not_ranked"] > 0
    assert abs(got["nll"] - cpu["nll"]) <= 2e-5 * abs(cpu["nll"]) + 1e-5
    close(torch.from_numpy(got["loss"]), cpu["loss"], f"{pre} loss per target", rtol=2e-5, atol=1e-5)
    close(torch.from_numpy(got["lse"]), cpu["lse"], f"{pre} lse", rtol=2e-5, atol=1e-5)
