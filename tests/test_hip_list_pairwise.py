"""GPU suite: the fused pairwise nDCG loss (``digat_list_pairwise_fwd`` / ``_scores_fwd`` / ``_bwd``, ``evaluate.list_pairwise`` and
``pairwise_scores``) and ``nrms.rank_step`` on it.  What is a matter of bits — the scores, ``valid``, the zeros, that two calls, a
list alone or in a batch, the autograd function and the C entry, the fused entry and the scores entry agree — is held exactly;
``loss``, ``ndcg`` and ``lambda`` to the float64 host contract on the kernel's own scores (``digat_dot_scores`` gathered at the
list's ids) at the bound the kernel file derives; the gradients at the training tolerance 2e-4."""
import functools

import numpy as np
import pytest
import torch

import list_pairwise_common as LP
import list_softmax_common as LC
import nrms_common as NC
import pool_softmax_common as PC
from nrms_common import close

pytestmark = pytest.mark.gpu

# G in {1, 3, 65}, M in {1, 2, 63, 65, 255, 257, 1024}, d in {1, 5, 36, 400, 512}; 65 lists only up to M = 257 (the twin is O(M^2) a list)
SWEEP = ((1, 1, 1), (3, 2, 5), (65, 63, 36), (1, 255, 400), (3, 257, 512), (65, 65, 5), (3, 1024, 400), (65, 255, 1), (1, 1024, 512),
         (65, 257, 36), (3, 65, 400), (1, 63, 5))
SLAB = 256      # csrc/digat_list_softmax.inc: LSM_SLAB, the slots one thread of the workgroup owns one of


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def test_the_sweep_covers_what_it_should():
    from digat_amd import evaluate
    assert {g for g, _, _ in SWEEP} == {1, 3, 65}
    assert {m for _, m, _ in SWEEP} == {1, 2, 63, 65, SLAB - 1, SLAB + 1, evaluate.SHORTLIST_MAX_K}      # an element, a pair, a wave, a slab edge
    assert {d for _, _, d in SWEEP} == {1, 5, 36, 400, evaluate.LIST_SOFTMAX_MAX_D}
    assert all(m <= SLAB + 1 for g, m, _ in SWEEP if g == 65) and len(SWEEP) == 12
    assert {(n + s) % len(LP.KINDS) for n, (g, _, _) in enumerate(SWEEP) for s in range(g)} == set(range(len(LP.KINDS))), "every kind of gains"


def _raw_forward(users, rows, ids, count, gain, D, scale):
    """The two C entries themselves, into buffers with a guard behind them: ``(loss, ndcg, valid, scores, lambda)`` of the fused entry,
    and the scores entry's outputs on those scores asserted to hold the same bits."""
    from digat_amd import _lib
    G, M = ids.shape
    f = dict(dtype=torch.float32, device=_dev())
    U, R, I, Cn, Gn, Dt = _t(users), _t(rows), _t(ids), _t(count), _t(gain), _t(D)
    L = _lib.lib()

    def buffers():
        return (torch.full((G + 4,), 77.0, **f), torch.full((G + 4,), 77.0, **f), torch.full((G + 4,), 77, dtype=torch.int32, device=_dev()),
                torch.full((G * M + 4,), 77.0, **f), torch.full((G * M + 4,), 77.0, **f))
    loss, ndcg, valid, sc, lam = buffers()
    _lib.check(L.digat_list_pairwise_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), Gn.data_ptr(), Dt.data_ptr(), G, len(rows), M,
                                         users.shape[1], scale, loss.data_ptr(), ndcg.data_ptr(), valid.data_ptr(), sc.data_ptr(),
                                         lam.data_ptr(), _lib.stream_ptr()), "digat_list_pairwise_fwd")
    for b in (loss, ndcg, valid):
        assert (b[G:] == 77).all(), "nothing beyond the arrays"
    assert (sc[G * M:] == 77).all() and (lam[G * M:] == 77).all(), "nothing beyond the arrays"
    loss2, ndcg2, valid2, _, lam2 = buffers()
    _lib.check(L.digat_list_pairwise_scores_fwd(sc.data_ptr(), _lib.ptr(Cn), Gn.data_ptr(), Dt.data_ptr(), G, M, scale, loss2.data_ptr(),
                                                ndcg2.data_ptr(), valid2.data_ptr(), lam2.data_ptr(), _lib.stream_ptr()),
               "digat_list_pairwise_scores_fwd")
    for a, b in ((loss, loss2), (ndcg, ndcg2), (lam, lam2)):
        assert np.array_equal(_bits(a), _bits(b)), "the fused entry and the scores entry on its scores: the same bits, guards included"
    assert torch.equal(valid, valid2)
    return loss[:G].cpu().numpy(), ndcg[:G].cpu().numpy(), valid[:G].cpu().numpy(), sc[:G * M].view(G, M).cpu().numpy(), \
        lam[:G * M].view(G, M).cpu().numpy()


def _run(users, rows, ids, count, gain, D, scale, gl):
    """One forward and backward through autograd on the device: ``(loss, ndcg, scores, d_users, d_rows)`` as numpy."""
    from digat_amd import evaluate
    U, R = _t(users).requires_grad_(True), _t(rows).requires_grad_(True)
    loss, ndcg, scores = evaluate.list_pairwise(U, R, _t(ids), _t(count), _t(gain), scale=scale, discount=D)
    assert loss.dtype == ndcg.dtype == scores.dtype == torch.float32
    assert loss.shape == ndcg.shape == (len(users),) and scores.shape == ids.shape
    assert loss.requires_grad and not ndcg.requires_grad and not scores.requires_grad
    (loss * _t(gl)).sum().backward()
    return tuple(t.detach().cpu().numpy() for t in (loss, ndcg, scores, U.grad, R.grad))


def _close_grad(got, want, cancelled, what):
    """tests/test_hip_list_softmax.py's rule: ``close(rtol=2e-4, atol=0)`` relative to the gradient's own size; where the exact gradient
    is identically zero, the same rtol to the size ``cancelled`` of the sums it is the difference of."""
    if np.abs(want).max() > 0:
        close(torch.from_numpy(got), want, what, rtol=2e-4, atol=0.0)
    else:
        assert np.isfinite(got).all() and np.abs(got).max() <= 2e-4 * cancelled, (what, float(np.abs(got).max()), cancelled)


def _gathered(users, rows, ids):
    from digat_amd import evaluate
    S = evaluate.dot_scores(_t(users), _t(rows)).cpu().numpy()
    ok = (ids >= 0) & (ids < len(rows))
    return np.where(ok, S[np.arange(len(ids))[:, None], np.where(ok, ids, 0)], np.float32(0))


def _over_bound(got, want, bound, what, name):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max()) if err.size else 0.0
    print(what, f"{name}: worst error over bound", worst)
    assert (err <= bound).all(), (what, name, worst)


def _check(users, rows, ids, count, gain, scale, k, rng, what):
    """The whole contract of one call against the host functions on ``dot_scores``.  ``scale`` is a float32 number."""
    from digat_amd import evaluate
    assert float(np.float32(scale)) == scale
    G, M = ids.shape
    P = len(rows)
    D = evaluate.ndcg_discount(M, k)
    gl = rng.standard_normal(G).astype(np.float32)
    loss, ndcg, scores, dU, dR = _run(users, rows, ids, count, gain, D, scale, gl)
    r_loss, r_ndcg, r_valid, r_scores, lam = _raw_forward(users, rows, ids, count, gain, D, scale)
    for a, b, name in ((loss, r_loss, "loss"), (ndcg, r_ndcg, "ndcg"), (scores, r_scores, "scores")):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, "the autograd function and the C entry")
    S = _gathered(users, rows, ids)
    elem = LP.elements(ids, count, P)
    w_loss, w_ndcg, w_valid, w_lam, n, A = evaluate.list_pairwise_host(S, ids, count, gain, P, scale, D, parts=True)
    # bits and zeros
    assert np.array_equal(np.isnan(scores), ~elem), (what, "NaN exactly where the slot is no element")
    assert np.array_equal(_bits(scores[elem]), _bits(S[elem])), (what, "score bits")
    assert np.array_equal(r_valid, w_valid.astype(np.int32)), (what, "valid")
    assert (loss[~w_valid] == 0).all() and (ndcg[~w_valid] == 0).all() and (lam[~w_valid] == 0).all(), what
    with np.errstate(invalid="ignore"):
        lab = elem & np.isfinite(gain) & (gain >= 0)
    assert (lam[~lab] == 0).all() and (w_lam[~lab] == 0).all(), (what, "lambda is 0 where the slot is no labelled element")
    assert (loss[w_loss == 0] == 0).all(), (what, "a list without a live pair has loss 0")
    # loss, ndcg and lambda at the derived bound
    _over_bound(loss, w_loss, evaluate.list_pairwise_bound(n, w_loss), what, "loss")
    _over_bound(ndcg, w_ndcg, evaluate.list_pairwise_bound(n, w_ndcg), what, "ndcg")
    _over_bound(lam, w_lam, evaluate.list_pairwise_bound(n[:, None], w_lam, A), what, "lambda")
    # gradients at the training tolerance
    w_dU, w_dR = evaluate.list_pairwise_grad_host(users, rows, S, ids, count, gain, scale, D, gl)
    _close_grad(dU, w_dU, LC.cancelled(gl, scale, rows), f"{what} d_users")
    _close_grad(dR, w_dR, LC.cancelled(gl, scale, users), f"{what} d_rows")
    named = np.zeros(P, dtype=bool)
    named[ids[elem]] = True
    assert (dR[~named] == 0).all() and (dU[~w_valid] == 0).all(), (what, "exactly zero where nothing contributes")
    return loss, ndcg, scores, lam, dU, dR


@pytest.mark.parametrize("G,M,d", SWEEP)
def test_loss_and_gradients_against_the_host_contract(G, M, d):
    rng = np.random.default_rng(1000 * G + M + d)
    n = SWEEP.index((G, M, d))
    for counted in (True, False):
        users, rows, ids, count, gain, kind = LP.case(rng, G, M, d, shift=n)
        _check(users, rows, ids, count if counted else None, gain, 1.0 if n % 2 else 0.5, 0 if (n // 2) % 2 else 10, rng, (G, M, d, counted))
        n += 1


def test_two_calls_and_a_list_alone_give_the_same_bits():
    from digat_amd import evaluate
    rng = np.random.default_rng(31)
    G, M, d = 65, 300, 36
    users, rows, ids, count, gain, _ = LP.case(rng, G, M, d)
    D = evaluate.ndcg_discount(M, 10)
    gl = rng.standard_normal(G).astype(np.float32)
    first = _run(users, rows, ids, count, gain, D, 0.5, gl)
    again = _run(users, rows, ids, count, gain, D, 0.5, gl)
    names = ("loss", "ndcg", "scores", "d_users", "d_rows")
    for a, b, name in zip(first, again, names):
        assert np.array_equal(_bits(a), _bits(b)), name
    lam = _raw_forward(users, rows, ids, count, gain, D, 0.5)[4]
    # a list alone: the same bits as inside the batch of 65 (the gradient of the rows is another sum and is not compared)
    for g in (2, 7, 64):
        one = _run(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], gain[g:g + 1], D, 0.5, gl[g:g + 1])
        for k in range(4):
            assert np.array_equal(_bits(one[k][0]), _bits(first[k][g])), (g, names[k])
        assert np.array_equal(_bits(_raw_forward(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], gain[g:g + 1], D, 0.5)[4][0]), _bits(lam[g]))


def test_scores_of_three_hundred_stay_finite():
    """x reaches +-300 and differences 600: exp overflows unless sp and sg are taken in their stable forms."""
    rng = np.random.default_rng(77)
    G, M, d = 6, 300, 32
    users, rows, ids, count, gain, _ = LP.case(rng, G, M, d, bad=0.05)
    count[:] = M
    S = users.astype(np.float64) @ rows.astype(np.float64).T
    users *= np.float32(300.0 / np.abs(S).max())
    loss, ndcg, scores, lam, dU, dR = _check(users, rows, ids, count, gain, 1.0, 0, rng, "range")
    assert np.nanmax(np.abs(scores)) > 150 and loss.max() > 0
    assert np.isfinite(loss).all() and np.isfinite(lam).all() and np.isfinite(dU).all() and np.isfinite(dR).all()


def test_pairwise_scores_under_autograd():
    from digat_amd import evaluate
    rng = np.random.default_rng(9)
    G, M = 9, 270
    _, _, ids, count, gain, _ = LP.case(rng, G, M, 4)
    S = (2.0 * rng.standard_normal((G, M))).astype(np.float32)
    S[:, 1] = S[:, 0]                                               # a tie in every list
    S[rng.random((G, M)) < 0.1] = np.nan                            # no element
    D = evaluate.ndcg_discount(M, 10)
    gl = rng.standard_normal(G).astype(np.float32)
    St = _t(S).requires_grad_(True)
    loss, ndcg = evaluate.pairwise_scores(St, _t(count), _t(gain), scale=0.5, discount=D)
    assert loss.requires_grad and not ndcg.requires_grad and loss.dtype == ndcg.dtype == torch.float32
    (loss * _t(gl)).sum().backward()
    w_loss, w_ndcg, w_valid, w_lam, n, A = evaluate.list_pairwise_host(S, None, count, gain, 0, 0.5, D, parts=True)
    assert w_valid.sum() >= 4
    _over_bound(loss.detach().cpu().numpy(), w_loss, evaluate.list_pairwise_bound(n, w_loss), "scores", "loss")
    _over_bound(ndcg.cpu().numpy(), w_ndcg, evaluate.list_pairwise_bound(n, w_ndcg), "scores", "ndcg")
    # the raw entry's lambda: the gradient is grad_loss lambda, bit for bit
    from digat_amd import _lib
    f = dict(dtype=torch.float32, device=_dev())
    o, lam = torch.empty((2, G), **f), torch.empty((G, M), **f)
    valid = torch.empty(G, dtype=torch.int32, device=_dev())
    Cn, Gn, Dt = _t(count), _t(gain), _t(D)
    _lib.check(_lib.lib().digat_list_pairwise_scores_fwd(St.data_ptr(), Cn.data_ptr(), Gn.data_ptr(), Dt.data_ptr(), G, M, 0.5, o[0].data_ptr(),
                                                         o[1].data_ptr(), valid.data_ptr(), lam.data_ptr(), _lib.stream_ptr()), "scores_fwd")
    _over_bound(lam.cpu().numpy(), w_lam, evaluate.list_pairwise_bound(n[:, None], w_lam, A), "scores", "lambda")
    assert np.array_equal(_bits(St.grad), _bits(_t(gl)[:, None] * lam)), "scores.grad == grad_loss[:, None] * lambda"
    assert np.array_equal(_bits(loss.detach()), _bits(o[0])) and np.array_equal(valid.cpu().numpy(), w_valid.astype(np.int32))
    assert (St.grad[_t(np.isnan(S))] == 0).all()


def test_refusals_and_empty_calls():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(13)
    G, M, d = 4, 9, 8
    users, rows, ids, count, gain, _ = LP.case(rng, G, M, d)
    P = len(rows)
    D = evaluate.ndcg_discount(M)
    U, R, I, Cn, Gn, Dt = _t(users), _t(rows), _t(ids), _t(count), _t(gain), _t(D)
    L = _lib.lib()
    f = dict(dtype=torch.float32, device=_dev())
    o = torch.full((5, G * M), 77.0, **f)
    valid = torch.full((G,), 77, dtype=torch.int32, device=_dev())

    def fwd(G=G, M=M, d=d, gain=Gn.data_ptr(), disc=Dt.data_ptr()):
        return L.digat_list_pairwise_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), gain, disc, G, P, M, d, 1.0, o[0].data_ptr(),
                                         o[1].data_ptr(), valid.data_ptr(), o[2].data_ptr(), o[3].data_ptr(), _lib.stream_ptr())

    def sfwd(G=G, M=M, disc=Dt.data_ptr()):
        return L.digat_list_pairwise_scores_fwd(o[4].data_ptr(), Cn.data_ptr(), Gn.data_ptr(), disc, G, M, 1.0, o[0].data_ptr(), o[1].data_ptr(),
                                                valid.data_ptr(), o[3].data_ptr(), _lib.stream_ptr())
    assert fwd(M=0) == 2 and fwd(M=1025) == 2 and fwd(d=513) == 2 and fwd(d=0) == 2 and fwd(gain=None) == 1 and fwd(disc=None) == 1 and fwd(G=-1) == 1
    assert sfwd(M=0) == 2 and sfwd(M=1025) == 2 and sfwd(disc=None) == 1
    assert fwd(G=0) == 0 and sfwd(G=0) == 0
    ws_need = int(L.digat_list_pairwise_workspace_bytes(G, M))
    assert ws_need == 256 and int(L.digat_list_pairwise_workspace_bytes(-1, M)) == 0
    ws = _lib.workspace(ws_need, _dev(), "list_pairwise")
    GL = torch.ones(G, **f)
    d_users = torch.full((G, d), 77.0, **f)

    def bwd(need=ws_need, d_rows=None, keys=None, E=0, M=M):
        return L.digat_list_pairwise_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, o[3].data_ptr(), GL.data_ptr(), keys, E,
                                         d_users.data_ptr(), d_rows, ws.data_ptr(), need, _lib.stream_ptr())
    assert bwd(need=ws_need - 1) == 3 and bwd(M=1025) == 2 and bwd(d_rows=o[4].data_ptr(), E=3) == 1 and bwd(d_rows=o[4].data_ptr(), E=-1) == 1
    torch.cuda.synchronize()
    assert (o == 77).all() and (valid == 77).all() and (d_users == 77).all(), "a refused or empty call launches nothing"
    with pytest.raises(ValueError, match="one device"):
        evaluate.list_pairwise(U, R, I.cpu(), Cn, Gn)
    with pytest.raises(ValueError, match="float64"):
        evaluate.list_pairwise(U, R, I, Cn, Gn, discount=D.astype(np.float32))
    # no list at all, and an empty table: no launch, zero gradients
    Ug = U.clone().requires_grad_(True)
    loss, ndcg, scores = evaluate.list_pairwise(Ug[:0], R, I[:0], Cn[:0], Gn[:0])
    assert loss.shape == ndcg.shape == (0,) and scores.shape == (0, M)
    loss.sum().backward()
    assert (Ug.grad == 0).all()
    none = evaluate.list_pairwise(U, R[:0], I, Cn, Gn)
    assert (none[0] == 0).all() and (none[1] == 0).all() and torch.isnan(none[2]).all()
    assert evaluate.pairwise_scores(torch.zeros((0, M), **f), None, Gn[:0])[0].shape == (0,)
    # the raw entries on an empty table: every byte written, nothing an element
    assert L.digat_list_pairwise_fwd(U.data_ptr(), None, I.data_ptr(), Cn.data_ptr(), Gn.data_ptr(), Dt.data_ptr(), G, 0, M, d, 1.0, o[0].data_ptr(),
                                     o[1].data_ptr(), valid.data_ptr(), o[2].data_ptr(), o[3].data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (o[0, :G] == 0).all() and (o[1, :G] == 0).all() and (valid == 0).all() and torch.isnan(o[2]).all() and (o[3] == 0).all()
    # a NULL d_rows: one launch, no keys; users without a gradient, rows with one, and the other way round
    lam = _raw_forward(users, rows, ids, count, gain, D, 1.0)[4]
    LM = _t(lam)
    assert L.digat_list_pairwise_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, LM.data_ptr(), GL.data_ptr(), None, 0,
                                     d_users.data_ptr(), None, ws.data_ptr(), ws_need, _lib.stream_ptr()) == 0
    Rg = R.clone().requires_grad_(True)
    evaluate.list_pairwise(U, Rg, I, Cn, Gn)[0].sum().backward()
    Ug = U.clone().requires_grad_(True)
    evaluate.list_pairwise(Ug, R, I, Cn, Gn)[0].sum().backward()
    assert np.array_equal(_bits(d_users), _bits(Ug.grad))
    S = _gathered(users, rows, ids)
    w_dU, w_dR = evaluate.list_pairwise_grad_host(users, rows, S, ids, count, gain)
    close(Ug.grad, w_dU, "d_users alone", rtol=2e-4, atol=0.0)
    close(Rg.grad, w_dR, "d_rows alone", rtol=2e-4, atol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# nrms.rank_step against the float64 CPU twin
# ---------------------------------------------------------------------------------------------------------------------
STEP_FIXTURE = "nrms_train_tiny.npz"      # test_hip_list_softmax.py's


def _train_set(device="cpu"):
    dev = NC.dev_set(STEP_FIXTURE, device)
    U, K = NC.case(STEP_FIXTURE)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U


@functools.lru_cache(maxsize=None)
def _lists():
    """Per user a list of 12 news with repeats across users, a count below M, an id outside the corpus, graded gains, an unlabelled
    slot and a list without a positive gain."""
    dev, U = _train_set()
    N = int(dev.title_text.shape[0])
    rng = np.random.default_rng(17)
    M = 12
    ids = rng.integers(1, N, size=(U, M)).astype(np.int64)
    gain = rng.integers(0, 4, size=(U, M)).astype(np.float32)
    count = np.full(U, M, dtype=np.int32)
    count[1] = M - 3
    ids[0, 4], ids[2, 0] = N + 2, -1
    gain[0, 1], gain[3, :] = np.nan, 0.0
    return np.arange(U), ids, gain, count


@functools.lru_cache(maxsize=None)
def _step_reference(pre):
    from digat_amd import nrms
    m = PC.double_twin(NC.model(STEP_FIXTURE, pre))
    m.train()
    dev, U = _train_set()
    loss = nrms.rank_step(m, dev, *_lists()[:3], _lists()[3], scale=1.0, k=5)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_nrms_rank_step_on_the_device(pre):
    from digat_amd import nrms
    want_loss, want = _step_reference(pre)
    m = NC.model(STEP_FIXTURE, pre, _dev())
    m.train()
    dev, U = _train_set(_dev())
    loss = nrms.rank_step(m, dev, *_lists()[:3], _lists()[3], scale=1.0, k=5)
    loss.backward()
    print(pre, "rank loss", float(loss.detach()), "float64 twin", want_loss)
    close(loss, np.float64(want_loss), f"{pre} rank loss", rtol=2e-5, atol=1e-5)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, want[k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)
