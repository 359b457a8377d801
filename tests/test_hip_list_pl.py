"""GPU suite: the differentiable Plackett-Luce slate likelihood (``digat_list_pl_fwd`` / ``_bwd``, ``digat_pl_scores_bwd``,
``evaluate.list_pl`` and ``pl_scores``) and ``nrms.policy_step`` / ``fit_policy`` on it.  What is a matter of bits — the scores, the
forward against ``pl_log_prob`` at ``scale = 1``, the zeros of the coefficient, that two calls, a list alone or in a batch, the
autograd function and the C entry, ``list_pl``'s coefficient and ``pl_scores``' gradient agree — is held exactly; ``logp`` and
``step_logp`` to the float64 host twin inside ``pl_bound``, the coefficient inside ``list_pl_bound`` (the worst ratio printed), the
gradients at the training tolerance 2e-4."""
import functools

import numpy as np
import pytest
import torch

import list_pl_common as LPL
import list_softmax_common as LC
import nrms_common as NC
import pool_softmax_common as PC
from nrms_common import close

pytestmark = pytest.mark.gpu

# (G, M, d, k, S): G in {1, 3, 65}, M in {1, 2, 63, 65, 255, 257, 1024}, d in {1, 5, 36, 400, 512}, k in {1, 10, 128}, S in {1, 3};
# 65 lists only up to M = 257
SWEEP = ((1, 1, 1, 1, 1), (3, 2, 5, 10, 3), (65, 63, 36, 10, 1), (1, 255, 400, 128, 3), (3, 257, 512, 10, 1), (65, 65, 5, 128, 3),
         (3, 1024, 400, 128, 1), (65, 255, 1, 1, 3), (1, 1024, 512, 10, 3), (65, 257, 36, 128, 1), (3, 65, 400, 1, 3), (1, 63, 5, 10, 1))
SLAB = 256      # csrc/digat_list_softmax.inc: LSM_SLAB


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _bits(x):
    a = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_the_sweep_covers_what_it_should():
    from digat_amd import evaluate
    assert {c[0] for c in SWEEP} == {1, 3, 65}
    assert {c[1] for c in SWEEP} == {1, 2, 63, 65, SLAB - 1, SLAB + 1, evaluate.SHORTLIST_MAX_K}
    assert {c[2] for c in SWEEP} == {1, 5, 36, 400, evaluate.LIST_SOFTMAX_MAX_D}
    assert {c[3] for c in SWEEP} == {1, 10, evaluate.PL_MAX_K} and {c[4] for c in SWEEP} == {1, 3}
    assert all(c[1] <= SLAB + 1 for c in SWEEP if c[0] == 65) and len(SWEEP) == 12
    kinds = {(g + s + n) % len(LPL.SLATE_KINDS) for n, c in enumerate(SWEEP) for g in range(c[0]) for s in range(c[4])}
    assert kinds == set(range(len(LPL.SLATE_KINDS))), "every kind of slate"


def _raw(users, rows, ids, count, picks, inv_t, gl):
    """The C entries themselves, into buffers with a guard behind them: ``(logp, step, scores, coef, d_users, d_rows)`` of
    ``digat_list_pl_fwd`` / ``digat_list_pl_bwd`` (the coefficient read from the workspace), with ``digat_pl_scores_bwd`` on those
    scores asserted to give the same coefficients."""
    from digat_amd import _lib, evaluate
    G, M = ids.shape
    S, k = picks.shape[1:]
    P, d = rows.shape
    dev = _dev()
    f = dict(dtype=torch.float32, device=dev)
    U, R, I, Cn, Pk, Gl = _t(users), _t(rows), _t(ids), _t(count), _t(picks.astype(np.int32)), _t(gl.astype(np.float64))
    L = _lib.lib()
    logp = torch.full((G * S + 4,), 77.0, dtype=torch.float64, device=dev)
    step, scores = torch.full((G * S * k + 4,), 77.0, **f), torch.full((G * M + 4,), 77.0, **f)
    _lib.check(L.digat_list_pl_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), G, P, M, d, Pk.data_ptr(), S, k, inv_t,
                                   logp.data_ptr(), step.data_ptr(), scores.data_ptr(), _lib.stream_ptr()), "digat_list_pl_fwd")
    assert (logp[G * S:] == 77).all() and (step[G * S * k:] == 77).all() and (scores[G * M:] == 77).all(), "nothing beyond the arrays"
    need = int(L.digat_list_pl_workspace_bytes(G, M))
    assert need >= G * M * 4
    ws = torch.full((need // 4 + 4,), 77.0, **f)
    elem = evaluate.list_elements(I, Cn, P).view(-1)
    keys = torch.sort(I.view(-1)[elem] * (G * M) + torch.arange(G * M, device=dev)[elem]).values.contiguous()
    d_users, d_rows = torch.full((G * d + 4,), 77.0, **f), torch.full((P * d + 4,), 77.0, **f)
    _lib.check(L.digat_list_pl_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), G, P, M, d, scores.data_ptr(), Pk.data_ptr(), S, k,
                                   inv_t, Gl.data_ptr(), _lib.ptr(keys) if keys.numel() else None, int(keys.numel()), d_users.data_ptr(),
                                   d_rows.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_list_pl_bwd")
    assert (ws[need // 4:] == 77).all() and (d_users[G * d:] == 77).all() and (d_rows[P * d:] == 77).all(), "nothing beyond the arrays"
    coef = ws[:G * M].view(G, M)
    grad = torch.full((G * M + 4,), 77.0, **f)
    _lib.check(L.digat_pl_scores_bwd(scores.data_ptr(), _lib.ptr(Cn), G, M, k, inv_t, S, Pk.data_ptr(), Gl.data_ptr(), grad.data_ptr(),
                                     _lib.stream_ptr()), "digat_pl_scores_bwd")
    assert (grad[G * M:] == 77).all()
    assert torch.equal(grad[:G * M].view(G, M), coef), "list_pl's coefficient is pl_scores' gradient on the same scores"
    return tuple(t.cpu().numpy() for t in (logp[:G * S].view(G, S), step[:G * S * k].view(G, S, k), scores[:G * M].view(G, M), coef,
                                           d_users[:G * d].view(G, d), d_rows[:P * d].view(P, d)))


def _run(users, rows, ids, count, picks, scale, T, gl):
    """One forward and backward through autograd on the device: ``(logp, step, scores, d_users, d_rows)`` as numpy."""
    from digat_amd import evaluate
    U, R = _t(users).requires_grad_(True), _t(rows).requires_grad_(True)
    logp, step, scores = evaluate.list_pl(U, R, _t(ids), _t(count), _t(picks), scale=scale, temperature=T)
    assert logp.dtype == torch.float64 and step.dtype == scores.dtype == torch.float32
    assert logp.shape == picks.shape[:2] and step.shape == picks.shape and scores.shape == ids.shape
    assert logp.requires_grad and not step.requires_grad and not scores.requires_grad
    (logp * _t(gl)).sum().backward()
    return tuple(t.detach().cpu().numpy() for t in (logp, step, scores, U.grad, R.grad))


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


WORST = {"coef": 0.0}


def _over_bound(got, want, bound, what, name):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    worst = float((err / bound).max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(what, f"{name}: worst error over bound", worst, "so far", WORST[name])
    assert (err <= bound).all(), (what, name, worst)


def _check(users, rows, ids, count, picks, gl, scale, T, what):
    """The whole contract of one call against the host functions on ``dot_scores``."""
    from digat_amd import evaluate
    G, M = ids.shape
    S, k = picks.shape[1:]
    P = len(rows)
    inv_t = evaluate._pl_inv_t(scale, T)
    logp, step, scores, dU, dR = _run(users, rows, ids, count, picks, scale, T, gl)
    r_logp, r_step, r_scores, coef, r_dU, r_dR = _raw(users, rows, ids, count, picks, inv_t, gl)
    for a, b, name in ((logp, r_logp, "logp"), (step, r_step, "step"), (scores, r_scores, "scores"), (dU, r_dU, "d_users"), (dR, r_dR, "d_rows")):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, "the autograd function and the C entry")
    Sg = _gathered(users, rows, ids)
    elem = LPL.elements(ids, count, P)
    live = elem & np.isfinite(Sg)
    # bits and zeros
    assert np.array_equal(np.isnan(scores) & ~elem, ~elem), (what, "NaN where the slot is no element")
    assert np.array_equal(np.isnan(scores[elem]), np.isnan(Sg[elem])), (what, "an overflowed chain is a NaN on both sides")
    number = elem & ~np.isnan(Sg)
    assert np.array_equal(_bits(scores[number]), _bits(Sg[number].astype(np.float32))), (what, "score bits")
    assert (_bits(coef)[~live] == 0).all(), (what, "the coefficient is exactly 0 where the slot is not live")
    sc_t, cn_t, pk_t = _t(scores), _t(count), _t(picks)
    if scale == 1.0:
        p_logp, p_step = evaluate.pl_log_prob(sc_t, cn_t, pk_t, T)
        assert np.array_equal(_bits(logp), _bits(p_logp)) and np.array_equal(_bits(step), _bits(p_step)), (what, "pl_log_prob's bits")
        X = sc_t.clone().requires_grad_(True)
        s_logp, s_step = evaluate.pl_scores(X, cn_t, pk_t, T)
        assert np.array_equal(_bits(s_logp), _bits(p_logp)) and np.array_equal(_bits(s_step), _bits(p_step)), (what, "pl_scores' forward")
        assert s_logp.requires_grad and not s_step.requires_grad
        (s_logp * _t(gl)).sum().backward()
        assert np.array_equal(X.grad.cpu().numpy(), coef), (what, "pl_scores' gradient is list_pl's coefficient")
        X64 = sc_t.double().requires_grad_(True)                   # another floating dtype: converted, the gradient in that dtype
        (evaluate.pl_scores(X64, cn_t, pk_t, T)[0] * _t(gl)).sum().backward()
        assert X64.grad.dtype == torch.float64 and np.array_equal(X64.grad.cpu().numpy(), coef.astype(np.float64)), (what, "float64 scores")
    # the host twin
    w_logp, w_step, w_coef, parts = evaluate.list_pl_host(Sg, ids, count, picks, P, scale, T, grad_logp=gl, parts=True)
    n = parts["live"].astype(np.float64)
    assert np.array_equal(n, live.sum(axis=1))
    _over_bound(step, w_step.astype(np.float64), evaluate.pl_bound(n[:, None, None], parts["logZ"], parts["step"], float32=True), what, "step_logp")
    _over_bound(logp, w_logp, evaluate.pl_bound(n[:, None, None], parts["logZ"], parts["step"], total=True), what, "logp")
    assert (logp[parts["length"] == 0] == 0).all() and (w_coef[~live] == 0).all()
    _over_bound(coef, w_coef, evaluate.list_pl_bound(n, k, S, w_coef, parts["absolute"]), what, "coef")
    # gradients at the training tolerance
    w_dU, w_dR = evaluate.list_pl_grad_host(users, rows, Sg, ids, count, picks, scale, T, gl)
    tame = np.abs(rows) < 1e30
    _close_grad(dU, w_dU, LC.cancelled(gl, inv_t, np.where(tame, rows, 0)), f"{what} d_users")
    _close_grad(dR, w_dR, LC.cancelled(gl, inv_t, users), f"{what} d_rows")
    named = np.zeros(P, dtype=bool)
    named[ids[live]] = True
    assert (dR[~named] == 0).all(), (what, "exactly zero where nothing contributes")
    return logp, step, scores, coef, dU, dR


@pytest.mark.parametrize("G,M,d,k,S", SWEEP)
def test_likelihood_and_gradients_against_the_host_contract(G, M, d, k, S):
    rng = np.random.default_rng(1000 * G + M + d + k)
    n = SWEEP.index((G, M, d, k, S))
    users, rows, ids, count, picks, gl, kind = LPL.case(rng, G, M, d, k, S, shift=n)
    scale, T = (1.0, 0.5) if n % 2 else (0.75, 1.5)
    _check(users, rows, ids, count if n % 3 else None, picks, gl, scale, T, (G, M, d, k, S))


def test_two_calls_and_a_list_alone_give_the_same_bits():
    from digat_amd import evaluate
    rng = np.random.default_rng(31)
    G, M, d, k, S = 65, 300, 36, 10, 3
    users, rows, ids, count, picks, gl, _ = LPL.case(rng, G, M, d, k, S)
    inv_t = evaluate._pl_inv_t(0.5, 0.25)
    first = _run(users, rows, ids, count, picks, 0.5, 0.25, gl)
    again = _run(users, rows, ids, count, picks, 0.5, 0.25, gl)
    names = ("logp", "step", "scores", "d_users", "d_rows")
    for a, b, name in zip(first, again, names):
        assert np.array_equal(_bits(a), _bits(b)), name
    coef = _raw(users, rows, ids, count, picks, inv_t, gl)[3]
    # a list alone: the same bits as inside the batch of 65 (the gradient of the rows is another sum and is not compared)
    for g in (2, 7, 64):
        one = _run(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], picks[g:g + 1], 0.5, 0.25, gl[g:g + 1])
        for i in range(4):
            assert np.array_equal(_bits(one[i][0]), _bits(first[i][g])), (g, names[i])
        alone = _raw(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], picks[g:g + 1], inv_t, gl[g:g + 1])[3]
        assert np.array_equal(_bits(alone[0]), _bits(coef[g])), (g, "coef")


def test_refusals_and_empty_calls():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(13)
    G, M, d, k, S = 4, 9, 8, 3, 2
    users, rows, ids, count, picks, gl, _ = LPL.case(rng, G, M, d, k, S)
    P = len(rows)
    U, R, I, Cn, Pk, Gl = _t(users), _t(rows), _t(ids), _t(count), _t(picks), _t(gl)
    L = _lib.lib()
    f = dict(dtype=torch.float32, device=_dev())
    o = torch.full((4, G * M * 4), 77.0, **f)
    lp = torch.full((G * S,), 77.0, dtype=torch.float64, device=_dev())
    ws_need = int(L.digat_list_pl_workspace_bytes(G, M))
    assert ws_need == 256 and int(L.digat_list_pl_workspace_bytes(-1, M)) == 0
    ws = torch.full((ws_need // 4,), 77.0, **f)

    def fwd(G=G, M=M, d=d, k=k, S=S, inv_t=1.0, picks=Pk.data_ptr(), logp=lp.data_ptr()):
        return L.digat_list_pl_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, picks, S, k, inv_t, logp, o[0].data_ptr(),
                                   o[1].data_ptr(), _lib.stream_ptr())

    def sbwd(G=G, M=M, k=k, S=S, inv_t=1.0, gl=Gl.data_ptr()):
        return L.digat_pl_scores_bwd(o[2].data_ptr(), Cn.data_ptr(), G, M, k, inv_t, S, Pk.data_ptr(), gl, o[1].data_ptr(), _lib.stream_ptr())

    def bwd(need=ws_need, d_rows=None, E=0, M=M, k=k):
        return L.digat_list_pl_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, o[2].data_ptr(), Pk.data_ptr(), S, k, 1.0,
                                   Gl.data_ptr(), None, E, o[3].data_ptr(), d_rows, ws.data_ptr(), need, _lib.stream_ptr())
    assert fwd(M=0) == 2 and fwd(M=1025) == 2 and fwd(d=513) == 2 and fwd(d=0) == 2 and fwd(k=0) == 2 and fwd(k=129) == 2 and fwd(S=0) == 2
    assert fwd(picks=None) == 1 and fwd(logp=None) == 1 and fwd(G=-1) == 1 and fwd(inv_t=0.0) == 1 and fwd(inv_t=float("nan")) == 1
    assert fwd(inv_t=float("inf")) == 1 and fwd(logp=lp.data_ptr() + 4) == 1
    assert sbwd(M=1025) == 2 and sbwd(k=129) == 2 and sbwd(S=0) == 2 and sbwd(gl=None) == 1 and sbwd(inv_t=-1.0) == 1
    assert bwd(need=ws_need - 1) == 3 and bwd(M=1025) == 2 and bwd(k=0) == 2 and bwd(d_rows=o[1].data_ptr(), E=3) == 1
    assert bwd(d_rows=o[1].data_ptr(), E=-1) == 1
    assert fwd(G=0) == 0 and sbwd(G=0) == 0
    torch.cuda.synchronize()
    assert (o == 77).all() and (lp == 77).all() and (ws == 77).all(), "a refused or empty call launches nothing"
    with pytest.raises(ValueError, match="one device"):
        evaluate.list_pl(U, R, I.cpu(), Cn, Pk)
    with pytest.raises(ValueError, match="integer positions"):
        evaluate.list_pl(U, R, I, Cn, Pk.float())
    # no list at all, and an empty table: no launch, zero gradients
    Ug = U.clone().requires_grad_(True)
    logp, step, scores = evaluate.list_pl(Ug[:0], R, I[:0], Cn[:0], Pk[:0])
    assert logp.shape == (0, S) and step.shape == (0, S, k) and scores.shape == (0, M)
    logp.sum().backward()
    assert (Ug.grad == 0).all()
    Ug = U.clone().requires_grad_(True)
    none = evaluate.list_pl(Ug, R[:0], I, Cn, Pk)
    assert (none[0] == 0).all() and (none[1] == 0).all() and torch.isnan(none[2]).all()
    none[0].sum().backward()
    assert (Ug.grad == 0).all()
    assert evaluate.pl_scores(torch.zeros((0, M), **f), None, Pk[:0], 1.0)[0].shape == (0, S)
    # the raw entry on an empty table: every byte written, nothing live
    assert L.digat_list_pl_fwd(U.data_ptr(), None, I.data_ptr(), Cn.data_ptr(), G, 0, M, d, Pk.data_ptr(), S, k, 1.0, lp.data_ptr(),
                               o[0].data_ptr(), o[1].data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (lp == 0).all() and (o[0, :G * S * k] == 0).all() and torch.isnan(o[1, :G * M]).all() and (o[1, G * M:] == 77).all()
    # users without a gradient, rows with one, and the other way round: the same numbers as together
    both = _run(users, rows, ids, count, picks, 1.0, 1.0, gl)
    Rg = R.clone().requires_grad_(True)
    (evaluate.list_pl(U, Rg, I, Cn, Pk)[0] * Gl).sum().backward()
    Ug = U.clone().requires_grad_(True)
    (evaluate.list_pl(Ug, R, I, Cn, Pk)[0] * Gl).sum().backward()
    assert np.array_equal(_bits(Ug.grad), _bits(both[3])) and np.array_equal(_bits(Rg.grad), _bits(both[4]))


# ---------------------------------------------------------------------------------------------------------------------
# nrms.policy_step against the float64 CPU twin; fit_policy twice
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_reference(pre):
    from digat_amd import nrms
    m = PC.double_twin(NC.model(LPL.STEP_FIXTURE, pre))
    m.train()
    dev, U = LPL.train_set()
    users, ids, gain, count, slates, weight = LPL.policy_lists()
    loss, logp = nrms.policy_step(m, dev, users, ids, slates, weight, count, scale=2.0, temperature=0.5)
    loss.backward()
    return float(loss.detach()), logp.numpy().copy(), {k: p.grad.numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_nrms_policy_step_on_the_device(pre):
    from digat_amd import nrms
    want_loss, want_logp, want = _step_reference(pre)
    m = NC.model(LPL.STEP_FIXTURE, pre, _dev())
    m.train()
    dev, U = LPL.train_set(_dev())
    users, ids, gain, count, slates, weight = LPL.policy_lists()
    loss, logp = nrms.policy_step(m, dev, users, ids, slates, weight, count, scale=2.0, temperature=0.5)
    loss.backward()
    print(pre, "policy loss", float(loss.detach()), "float64 twin", want_loss)
    assert logp.dtype == torch.float64 and not logp.requires_grad and (logp[:, 2] == 0).all()
    close(logp, want_logp, f"{pre} logp", rtol=2e-5, atol=1e-5)
    close(loss, np.float64(want_loss), f"{pre} policy loss", rtol=2e-5, atol=1e-5)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, want[k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)


def test_fit_policy_twice_gives_the_same_losses():
    from digat_amd import nrms
    dev, U = LPL.train_set(_dev())
    users, ids, gain, count, _, _ = LPL.policy_lists()

    def run():
        torch.manual_seed(5)
        m = NC.model(LPL.STEP_FIXTURE, "nrms", _dev())
        return nrms.fit_policy(m, dev, (users, ids, gain, count), steps=4, k=3, samples=4, temperature=0.7, batch_users=3, lr=1e-3, seed=11,
                               scale=1.5)
    losses, rewards = run()
    assert len(losses) == 4 and np.isfinite(losses).all() and all(0.0 <= r <= 1.0 for r in rewards)
    assert run() == (losses, rewards), "bit for bit"
