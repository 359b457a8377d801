"""GPU suite: the PL-Rank policy gradient (``digat_list_plrank_fwd`` / ``_bwd``, ``digat_plrank_scores_fwd`` / ``_bwd``,
``evaluate.list_plrank`` and ``plrank_scores``) and ``nrms.plrank_step`` / ``fit_policy(estimator="plrank")`` on it.  What is a matter
of bits — the scores, the drawn slates against ``pl_sample``, a call split by ``first_sample``, two calls, a list alone or in a batch,
the autograd functions and the C entries, ``list_plrank``'s coefficient and ``plrank_scores``' gradient, the zeros of the coefficient
— is held exactly; ``slate_value``, ``value`` and the coefficient to the float64 host twin inside ``plrank_bound`` (the worst ratio
printed), the gradients at the training tolerance 2e-4; and the estimator's mean over every ordered slate to the exact gradient."""
import functools

import numpy as np
import pytest
import torch

import list_pl_common as LPL
import nrms_common as NC
import plrank_common as PR
import pool_softmax_common as PC
from nrms_common import close
from test_hip_list_pl import SWEEP, _bits, _close_grad, _dev, _gathered, _t

pytestmark = pytest.mark.gpu

WORST = {}


def _over_bound(got, want, bound, what, name):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(what, f"{name}: worst error over bound", worst, "so far", WORST[name])
    assert (err <= bound).all() and worst <= 1.0, (what, name, worst)


def _raw(users, rows, ids, count, gain, theta, lw, picks, S, k, inv_t, seed, first, streams, gv):
    """The C entries themselves, into buffers with a guard behind them: ``(value, slate_value, picks, scores, coef, d_users, d_rows)``
    of ``digat_list_plrank_fwd`` / ``_bwd`` (the coefficient read from the workspace), with ``digat_plrank_scores_fwd`` and
    ``digat_plrank_scores_bwd`` on those scores asserted to give the same bits.  ``picks`` None: the slates are drawn."""
    from digat_amd import _lib, evaluate
    G, M = ids.shape
    P, d = rows.shape
    dev = _dev()
    f = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    U, R, I, Cn, Gn, Th, Lw, St, Gv = (_t(x) for x in (users, rows, ids, count, gain, theta, lw, streams, gv))
    Pk = None if picks is None else _t(picks.astype(np.int32))
    L = _lib.lib()

    def outputs():
        return (torch.full((G * S * k + 4,), 77, dtype=torch.int32, device=dev), torch.full((G * S + 4,), 77.0, **f64),
                torch.full((G + 4,), 77.0, **f64))
    out_p, sv, value = outputs()
    scores = torch.full((G * M + 4,), 77.0, **f)
    _lib.check(L.digat_list_plrank_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), G, P, M, d, Gn.data_ptr(), Th.data_ptr(), _lib.ptr(Lw),
                                       _lib.ptr(Pk), S, k, inv_t, seed, first, _lib.ptr(St), out_p.data_ptr(), sv.data_ptr(), value.data_ptr(),
                                       scores.data_ptr(), _lib.stream_ptr()), "digat_list_plrank_fwd")
    assert (out_p[G * S * k:] == 77).all() and (sv[G * S:] == 77).all() and (value[G:] == 77).all() and (scores[G * M:] == 77).all()
    if Pk is not None:
        assert (out_p == 77).all(), "given slates are not written back"
    used = out_p[:G * S * k].view(G, S, k).contiguous() if Pk is None else Pk
    out_p2, sv2, value2 = outputs()
    _lib.check(L.digat_plrank_scores_fwd(scores.data_ptr(), _lib.ptr(Cn), G, M, Gn.data_ptr(), Th.data_ptr(), _lib.ptr(Lw), _lib.ptr(Pk), S, k, inv_t,
                                         seed, first, _lib.ptr(St), out_p2.data_ptr(), sv2.data_ptr(), value2.data_ptr(), _lib.stream_ptr()),
               "digat_plrank_scores_fwd")
    assert torch.equal(out_p2, out_p) and torch.equal(sv2, sv) and torch.equal(value2, value), "the forward from given scores: the same bits"
    need = int(L.digat_list_plrank_workspace_bytes(G, M))
    assert need >= G * M * 4
    ws = torch.full((need // 4 + 4,), 77.0, **f)
    elem = evaluate.list_elements(I, Cn, P).view(-1)
    keys = torch.sort(I.view(-1)[elem] * (G * M) + torch.arange(G * M, device=dev)[elem]).values.contiguous()
    d_users, d_rows = torch.full((G * d + 4,), 77.0, **f), torch.full((P * d + 4,), 77.0, **f)
    _lib.check(L.digat_list_plrank_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), _lib.ptr(Cn), G, P, M, d, scores.data_ptr(), Gn.data_ptr(),
                                       Th.data_ptr(), _lib.ptr(Lw), used.data_ptr(), S, k, inv_t, Gv.data_ptr(),
                                       _lib.ptr(keys) if keys.numel() else None, int(keys.numel()), d_users.data_ptr(), d_rows.data_ptr(),
                                       ws.data_ptr(), need, _lib.stream_ptr()), "digat_list_plrank_bwd")
    assert (ws[need // 4:] == 77).all() and (d_users[G * d:] == 77).all() and (d_rows[P * d:] == 77).all(), "nothing beyond the arrays"
    coef = ws[:G * M].view(G, M)
    grad = torch.full((G * M + 4,), 77.0, **f)
    _lib.check(L.digat_plrank_scores_bwd(scores.data_ptr(), _lib.ptr(Cn), G, M, Gn.data_ptr(), Th.data_ptr(), _lib.ptr(Lw), used.data_ptr(), S, k,
                                         inv_t, Gv.data_ptr(), grad.data_ptr(), _lib.stream_ptr()), "digat_plrank_scores_bwd")
    assert (grad[G * M:] == 77).all()
    assert torch.equal(grad[:G * M].view(G, M), coef), "list_plrank's coefficient is plrank_scores' gradient on the same scores"
    return tuple(t.cpu().numpy() for t in (value[:G], sv[:G * S].view(G, S), used, scores[:G * M].view(G, M), coef,
                                           d_users[:G * d].view(G, d), d_rows[:P * d].view(P, d)))


def _run(users, rows, ids, count, gain, theta, lw, picks, S, k, scale, T, seed, first, streams, gv):
    """One forward and backward through autograd on the device: ``(value, slate_value, picks, scores, d_users, d_rows)`` as numpy."""
    from digat_amd import evaluate
    U, R = _t(users).requires_grad_(True), _t(rows).requires_grad_(True)
    value, sv, pk, scores = evaluate.list_plrank(U, R, _t(ids), _t(count), _t(gain), k, S, theta, lw, scale, T, seed, first, _t(streams), _t(picks))
    G, M = ids.shape
    assert value.dtype == sv.dtype == torch.float64 and pk.dtype == torch.int32 and scores.dtype == torch.float32
    assert value.shape == (G,) and sv.shape == (G, S) and pk.shape == (G, S, k) and scores.shape == (G, M)
    assert value.requires_grad and not sv.requires_grad and not pk.requires_grad and not scores.requires_grad
    (value * _t(gv)).sum().backward()
    return tuple(t.detach().cpu().numpy() for t in (value, sv, pk, scores, U.grad, R.grad))


def _check(users, rows, ids, count, gain, theta, lw, picks, S, k, scale, T, seed, first, streams, gv, what):
    """The whole contract of one call against the host functions, fed the device's scores and picks."""
    from digat_amd import evaluate
    G, M = ids.shape
    P = len(rows)
    inv_t = evaluate._pl_inv_t(scale, T)
    th = evaluate.ndcg_discount(k) if theta is None else theta
    value, sv, pk, scores, dU, dR = _run(users, rows, ids, count, gain, theta, lw, picks, S, k, scale, T, seed, first, streams, gv)
    raw = _raw(users, rows, ids, count, gain, th, lw, picks, S, k, inv_t, seed, first, streams, gv)
    r_value, r_sv, r_pk, r_scores, coef, r_dU, r_dR = raw
    for a, b, name in ((value, r_value, "value"), (sv, r_sv, "slate_value"), (scores, r_scores, "scores"), (dU, r_dU, "d_users"), (dR, r_dR, "d_rows")):
        assert np.array_equal(_bits(a), _bits(b)), (what, name, "the autograd function and the C entry")
    # drawn slates: the C entry's; given slates come back as int32, a position outside the list held at -1 or PL_MAX_LIST (the same cut)
    assert np.array_equal(pk, r_pk if picks is None else np.clip(picks, -1, evaluate.PL_MAX_LIST)), (what, "picks")
    Sg = _gathered(users, rows, ids)
    elem = LPL.elements(ids, count, P)
    live = elem & np.isfinite(Sg)
    assert np.array_equal(np.isnan(scores) & ~elem, ~elem), (what, "NaN where the slot is no element")
    number = elem & ~np.isnan(Sg)
    assert np.array_equal(np.isnan(scores[elem]), np.isnan(Sg[elem])) and np.array_equal(_bits(scores[number]), _bits(Sg[number].astype(np.float32)))
    assert (_bits(coef)[~live] == 0).all(), (what, "the coefficient is exactly 0 where the slot is not live")
    sc_t, cn_t = _t(scores), _t(count)
    if picks is None:
        n_live = live.sum(axis=1)
        assert ((pk >= 0).sum(axis=2) == np.minimum(n_live, k)[:, None]).all(), (what, "min(k, live) entries, -1 behind them")
        if scale == 1.0:
            want = evaluate.pl_sample(sc_t, cn_t, k, T, seed, S, first, _t(streams))[0]
            assert np.array_equal(pk, want.cpu().numpy()), (what, "pl_sample's picks on the returned scores")
    if scale == 1.0:
        X = sc_t.clone().requires_grad_(True)
        s_value, s_sv, s_pk = evaluate.plrank_scores(X, cn_t, _t(gain), k, S, theta, lw, T, seed, first, _t(streams), _t(picks))
        assert np.array_equal(_bits(s_value), _bits(value)) and np.array_equal(_bits(s_sv), _bits(sv)) and np.array_equal(s_pk.cpu().numpy(), pk)
        assert s_value.requires_grad and not s_sv.requires_grad
        (s_value * _t(gv)).sum().backward()
        assert np.array_equal(X.grad.cpu().numpy(), coef), (what, "plrank_scores' gradient is list_plrank's coefficient")
    # the host twin on the device's scores and picks
    w_value, w_sv, w_coef, parts = evaluate.plrank_host(scores, ids, count, pk, gain, P, theta, lw, scale, T, grad_value=gv, parts=True)
    n = parts["live"].astype(np.float64)
    assert np.array_equal(n, live.sum(axis=1)) and (w_coef[~live] == 0).all() and (sv[parts["length"] == 0] == 0).all()
    _over_bound(sv, w_sv, evaluate.plrank_bound(n, k, S, value=w_sv), what, "slate_value")
    _over_bound(value, w_value, evaluate.plrank_bound(n, k, S, value=w_value), what, "value")
    _over_bound(coef, w_coef, evaluate.plrank_bound(n, k, S, w_coef, parts["absolute"]), what, "coef")
    w_dU, w_dR = evaluate.plrank_grad_host(users, rows, scores, ids, count, pk, gain, theta, lw, scale, T, gv)
    tame = np.abs(rows) < 1e30
    size = float(parts["absolute"].max())
    _close_grad(dU, w_dU, size * float(np.abs(np.where(tame, rows, 0)).max()), f"{what} d_users")
    _close_grad(dR, w_dR, size * float(np.abs(users).max()), f"{what} d_rows")
    named = np.zeros(P, dtype=bool)
    named[ids[live]] = True
    assert (dR[~named] == 0).all(), (what, "exactly zero where nothing contributes")
    return value, sv, pk, scores, coef, dU, dR


def _inputs(rng, G, M, d, k, S, n):
    users, rows, ids, count, picks, _, kind = LPL.case(rng, G, M, d, k, S, shift=n)
    gain, _ = PR.odd_gains(rng, G, M)
    lw = None if n % 2 else rng.random(G) + 0.5
    streams = rng.integers(0, 1 << 31, size=G).astype(np.int64) if n % 3 else None
    theta = np.ones(k) if n % 4 == 1 else None                       # precision@k's weights now and then
    gv = rng.standard_normal(G)
    gv[rng.random(G) < 1.0 / 6.0] = 0.0
    return users, rows, ids, count, gain, theta, lw, picks, streams, gv


@pytest.mark.parametrize("G,M,d,k,S", SWEEP)
def test_drawn_slates_values_and_gradients_against_the_host_contract(G, M, d, k, S):
    rng = np.random.default_rng(1000 * G + M + d + k)
    n = SWEEP.index((G, M, d, k, S))
    users, rows, ids, count, gain, theta, lw, _, streams, gv = _inputs(rng, G, M, d, k, S, n)
    scale, T = (1.0, 0.5) if n % 2 else (0.75, 1.5)
    _check(users, rows, ids, count if n % 3 else None, gain, theta, lw, None, S, k, scale, T, 17 + n, 5 * n, streams, gv, (G, M, d, k, S))


@pytest.mark.parametrize("G,M,d,k,S", [(12, 65, 36, 10, 3), (6, 257, 5, 128, 3), (7, 9, 4, 4, 6)])
def test_given_slates_of_every_kind(G, M, d, k, S):
    rng = np.random.default_rng(G + M)
    users, rows, ids, count, gain, theta, lw, picks, streams, gv = _inputs(rng, G, M, d, k, S, 0)
    kinds = {(g + s) % len(LPL.SLATE_KINDS) for g in range(G) for s in range(S)}
    assert kinds == set(range(len(LPL.SLATE_KINDS))), "every kind of slate"
    for scale, T in ((1.0, 0.5), (0.75, 1.5)):
        _check(users, rows, ids, count, gain, theta, lw, picks, S, k, scale, T, 0, 0, None, gv, (G, M, d, k, S, "given"))


def test_a_split_call_two_calls_and_a_list_alone_give_the_same_bits():
    from digat_amd import evaluate
    rng = np.random.default_rng(31)
    G, M, d, k, S = 65, 300, 36, 10, 3
    users, rows, ids, count, gain, theta, lw, _, streams, gv = _inputs(rng, G, M, d, k, S, 4)
    inv_t = evaluate._pl_inv_t(0.5, 0.25)
    th = evaluate.ndcg_discount(k)
    args = (gain, theta, lw, None, S, k, 0.5, 0.25, 3, 40, streams, gv)
    first = _run(users, rows, ids, count, *args)
    again = _run(users, rows, ids, count, *args)
    names = ("value", "slate_value", "picks", "scores", "d_users", "d_rows")
    for a, b, name in zip(first, again, names):
        assert np.array_equal(a, b, equal_nan=True) and (a.dtype.kind != "f" or np.array_equal(_bits(a), _bits(b))), name
    # a call split by first_sample: every slate and its value
    for s in range(S):
        part = _run(users, rows, ids, count, gain, theta, lw, None, 1, k, 0.5, 0.25, 3, 40 + s, streams, gv)
        assert np.array_equal(part[2][:, 0], first[2][:, s]) and np.array_equal(_bits(part[1][:, 0]), _bits(first[1][:, s])), s
    coef = _raw(users, rows, ids, count, gain, th, lw, None, S, k, inv_t, 3, 40, streams, gv)[4]
    # a list alone: the same bits as inside the batch of 65 (the gradient of the rows is another sum and is not compared)
    for g in (2, 7, 64):
        one_lw = None if lw is None else lw[g:g + 1]
        one = _run(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], gain[g:g + 1], theta, one_lw, None, S, k, 0.5, 0.25, 3, 40,
                   streams[g:g + 1], gv[g:g + 1])
        for i in range(5):
            assert np.array_equal(one[i][0], first[i][g], equal_nan=True), (g, names[i])
        alone = _raw(users[g:g + 1], rows, ids[g:g + 1], count[g:g + 1], gain[g:g + 1], th, one_lw, None, S, k, inv_t, 3, 40, streams[g:g + 1],
                     gv[g:g + 1])[4]
        assert np.array_equal(_bits(alone[0]), _bits(coef[g])), (g, "coef")


@pytest.mark.parametrize("M,k,seed", [(5, 3, 0), (5, 3, 1)])
def test_the_device_estimator_is_unbiased_over_every_ordered_slate(M, k, seed):
    """No random test: Y copies of one list, one slate each — the Y ordered slates of k of M — given as picks; the mean of the device's
    coefficient under the policy's exact probabilities against the exact gradient of the expected metric, within the same mean of
    ``plrank_bound`` (the enumeration's own float64 error, below 1e-15, on top)."""
    from digat_amd import evaluate
    scores, rho, theta = PR.fixture(M, k, seed)
    slates, pi, R, grad, _ = PR.enumeration(M, k, seed)
    Y = len(slates)
    assert Y == 60
    sc = np.tile(scores, (Y, 1))
    gn = np.tile(rho, (Y, 1))
    X = _t(sc).requires_grad_(True)
    value, sv, pk = evaluate.plrank_scores(X, None, _t(gn), k, 1, theta, None, 1.0, picks=_t(slates[:, None, :]))
    value.sum().backward()
    coef = X.grad.cpu().numpy().astype(np.float64)
    assert np.abs(sv.cpu().numpy()[:, 0] - R).max() <= 1e-14
    w_coef, parts = evaluate.plrank_host(sc, None, None, slates[:, None, :], gn, 0, theta, grad_value=np.ones(Y), parts=True)[2:]
    bound = evaluate.plrank_bound(parts["live"], k, 1, w_coef, parts["absolute"])
    err = np.abs((pi[:, None] * coef).sum(axis=0) - grad)
    allowed = (pi[:, None] * bound).sum(axis=0) + 1e-15
    print((M, k, seed), "|mean of the device's coefficient - exact gradient|", err, "allowed", allowed)
    assert (err <= allowed).all()


def test_refusals_and_empty_calls():
    from digat_amd import _lib, evaluate
    rng = np.random.default_rng(13)
    G, M, d, k, S = 4, 9, 8, 3, 2
    users, rows, ids, count, gain, _, _, picks, _, gv = _inputs(rng, G, M, d, k, S, 0)
    P = len(rows)
    U, R, I, Cn, Gn, Pk, Gv, Th = (_t(x) for x in (users, rows, ids, count, gain, picks, gv, evaluate.ndcg_discount(k)))
    L = _lib.lib()
    f = dict(dtype=torch.float32, device=_dev())
    o = torch.full((4, G * M * 4), 77.0, **f)
    o64 = torch.full((2, G * S + 1), 77.0, dtype=torch.float64, device=_dev())
    op = torch.full((G * S * k,), 77, dtype=torch.int32, device=_dev())
    ws_need = int(L.digat_list_plrank_workspace_bytes(G, M))
    assert ws_need == int(L.digat_list_pl_workspace_bytes(G, M)) and int(L.digat_list_plrank_workspace_bytes(-1, M)) == 0
    ws = torch.full((ws_need // 4,), 77.0, **f)

    def fwd(G=G, M=M, d=d, k=k, S=S, inv_t=1.0, picks=None, out_picks=op.data_ptr(), gain=Gn.data_ptr(), theta=Th.data_ptr(), first=0,
            value=o64[1].data_ptr()):
        return L.digat_list_plrank_fwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, gain, theta, None, picks, S, k, inv_t, 1,
                                       first, None, out_picks, o64[0].data_ptr(), value, o[0].data_ptr(), _lib.stream_ptr())

    def sfwd(G=G, M=M, k=k, S=S, picks=None, out_picks=op.data_ptr(), first=0):
        return L.digat_plrank_scores_fwd(o[2].data_ptr(), Cn.data_ptr(), G, M, Gn.data_ptr(), Th.data_ptr(), None, picks, S, k, 1.0, 1, first, None,
                                         out_picks, o64[0].data_ptr(), o64[1].data_ptr(), _lib.stream_ptr())

    def sbwd(G=G, M=M, k=k, S=S, inv_t=1.0, gv=Gv.data_ptr(), picks=Pk.data_ptr()):
        return L.digat_plrank_scores_bwd(o[2].data_ptr(), Cn.data_ptr(), G, M, Gn.data_ptr(), Th.data_ptr(), None, picks, S, k, inv_t, gv,
                                         o[1].data_ptr(), _lib.stream_ptr())

    def bwd(need=ws_need, d_rows=None, E=0, M=M, k=k):
        return L.digat_list_plrank_bwd(U.data_ptr(), R.data_ptr(), I.data_ptr(), Cn.data_ptr(), G, P, M, d, o[2].data_ptr(), Gn.data_ptr(), Th.data_ptr(),
                                       None, Pk.data_ptr(), S, k, 1.0, Gv.data_ptr(), None, E, o[3].data_ptr(), d_rows, ws.data_ptr(), need,
                                       _lib.stream_ptr())
    top = evaluate.PL_MAX_SAMPLE
    assert fwd(M=0) == 2 and fwd(M=1025) == 2 and fwd(d=513) == 2 and fwd(d=0) == 2 and fwd(k=0) == 2 and fwd(k=129) == 2 and fwd(S=0) == 2
    assert fwd(first=-1) == 2 and fwd(first=top - 1) == 2 and fwd(first=top + 1) == 2
    assert fwd(out_picks=None) == 1 and fwd(gain=None) == 1 and fwd(theta=None) == 1 and fwd(G=-1) == 1 and fwd(inv_t=0.0) == 1
    assert fwd(inv_t=float("nan")) == 1 and fwd(inv_t=float("inf")) == 1 and fwd(value=o64[1].data_ptr() + 4) == 1 and fwd(value=None) == 1
    assert sfwd(M=1025) == 2 and sfwd(k=129) == 2 and sfwd(S=0) == 2 and sfwd(out_picks=None) == 1 and sfwd(first=top) == 2
    assert sbwd(M=1025) == 2 and sbwd(k=129) == 2 and sbwd(S=0) == 2 and sbwd(gv=None) == 1 and sbwd(inv_t=-1.0) == 1 and sbwd(picks=None) == 1
    assert bwd(need=ws_need - 1) == 3 and bwd(M=1025) == 2 and bwd(k=0) == 2 and bwd(d_rows=o[1].data_ptr(), E=3) == 1
    assert bwd(d_rows=o[1].data_ptr(), E=-1) == 1
    assert fwd(G=0) == 0 and sfwd(G=0) == 0 and sbwd(G=0) == 0
    torch.cuda.synchronize()
    assert (o == 77).all() and (o64 == 77).all() and (op == 77).all() and (ws == 77).all(), "a refused or empty call launches nothing"
    with pytest.raises(ValueError, match="one device"):
        evaluate.list_plrank(U, R, I.cpu(), Cn, Gn, k)
    with pytest.raises(ValueError, match="integer positions"):
        evaluate.list_plrank(U, R, I, Cn, Gn, k, picks=Pk.float())
    # no list at all, and an empty table: no launch, zero gradients
    Ug = U.clone().requires_grad_(True)
    value, sv, pk, scores = evaluate.list_plrank(Ug[:0], R, I[:0], Cn[:0], Gn[:0], k, S)
    assert value.shape == (0,) and sv.shape == (0, S) and pk.shape == (0, S, k) and scores.shape == (0, M)
    value.sum().backward()
    assert (Ug.grad == 0).all()
    Ug = U.clone().requires_grad_(True)
    none = evaluate.list_plrank(Ug, R[:0], I, Cn, Gn, k, S)
    assert (none[0] == 0).all() and (none[1] == 0).all() and (none[2] == -1).all() and torch.isnan(none[3]).all()
    none[0].sum().backward()
    assert (Ug.grad == 0).all()
    assert evaluate.plrank_scores(torch.zeros((0, M), **f), None, Gn[:0], k, S)[1].shape == (0, S)
    # users without a gradient, rows with one, and the other way round: the same numbers as together
    both = _run(users, rows, ids, count, gain, None, None, None, S, k, 1.0, 1.0, 1, 0, None, gv)
    Rg = R.clone().requires_grad_(True)
    (evaluate.list_plrank(U, Rg, I, Cn, Gn, k, S, seed=1)[0] * Gv).sum().backward()
    Ug = U.clone().requires_grad_(True)
    (evaluate.list_plrank(Ug, R, I, Cn, Gn, k, S, seed=1)[0] * Gv).sum().backward()
    assert np.array_equal(_bits(Ug.grad), _bits(both[4])) and np.array_equal(_bits(Rg.grad), _bits(both[5]))


# ---------------------------------------------------------------------------------------------------------------------
# nrms.plrank_step against the float64 CPU twin, in eval mode; fit_policy(estimator="plrank") twice
# ---------------------------------------------------------------------------------------------------------------------
STEP = dict(k=3, samples=4, scale=1.0, temperature=0.5, seed=6, first_sample=12)


def _step(m, dev, monkeypatch):
    """One ``plrank_step`` in eval mode: ``(loss with its graph, reward, what evaluate.list_plrank returned)``."""
    from digat_amd import evaluate, nrms
    users, ids, gain, count, _, _ = LPL.policy_lists()
    seen = []
    real = evaluate.list_plrank
    monkeypatch.setattr(evaluate, "list_plrank", lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1])
    m.eval()
    loss, reward = nrms.plrank_step(m, dev, users, ids, gain, count, **STEP)
    monkeypatch.setattr(evaluate, "list_plrank", real)
    return loss, reward, seen[0]


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_nrms_plrank_step_on_the_device(pre, monkeypatch):
    from digat_amd import evaluate, nrms
    users, ids, gain, count, _, _ = LPL.policy_lists()
    ref = PC.double_twin(NC.model(LPL.STEP_FIXTURE, pre))
    want_loss, want_reward, (w_value, w_sv, w_picks, _) = _step(ref, LPL.train_set()[0], monkeypatch)
    want_loss.backward()
    m = NC.model(LPL.STEP_FIXTURE, pre, _dev())
    dev, U = LPL.train_set(_dev())
    loss, reward, (value, sv, picks, scores) = _step(m, dev, monkeypatch)
    loss.backward()
    print(pre, "plrank loss", float(loss.detach()), "float64 twin", float(want_loss.detach()), "reward", float(reward))
    # the slates are pl_sample's on the scores of the graph-free pass, with the impressions as streams (eval mode: the same scores up to
    # the last bits — the encoders' training kernels are not their inference kernels — which move no key past its neighbour here)
    free, cnt = nrms._list_scores(m, dev, users, ids, count.astype(np.int64))
    assert torch.equal(torch.isnan(free), torch.isnan(scores))
    close(torch.nan_to_num(scores), torch.nan_to_num(free).cpu().numpy(), f"{pre} scores of the one pass", rtol=1e-5, atol=1e-6)
    drawn = evaluate.pl_sample(free, cnt, STEP["k"], STEP["temperature"], STEP["seed"], STEP["samples"], STEP["first_sample"],
                               torch.from_numpy(users).to(_dev()))[0]
    assert torch.equal(picks, drawn), "pl_sample on _list_scores"
    assert np.array_equal(picks.cpu().numpy(), w_picks.numpy()), "the float64 twin drew the same slates"
    assert value.dtype == torch.float64 and value.requires_grad and not sv.requires_grad
    close(sv, w_sv.numpy(), f"{pre} slate_value", rtol=1e-12, atol=0.0)
    close(loss, np.float64(want_loss.detach()), f"{pre} plrank loss", rtol=1e-12, atol=1e-12)
    assert abs(float(reward) - float(want_reward)) <= 1e-12 and 0.0 < float(reward) <= 1.0
    grads = {k: p.grad.numpy().copy() for k, p in ref.named_parameters()}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, grads[k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)


def test_fit_policy_with_the_plrank_estimator_twice_gives_the_same_losses():
    from digat_amd import nrms
    dev, U = LPL.train_set(_dev())
    users, ids, gain, count, _, _ = LPL.policy_lists()

    def run():
        torch.manual_seed(5)
        m = NC.model(LPL.STEP_FIXTURE, "nrms", _dev())
        return nrms.fit_policy(m, dev, (users, ids, gain, count), steps=4, k=3, samples=4, temperature=0.7, batch_users=3, lr=1e-3, seed=11,
                               scale=1.5, estimator="plrank")
    losses, rewards = run()
    assert len(losses) == 4 and np.isfinite(losses).all() and all(0.0 <= r <= 1.0 for r in rewards)
    assert run() == (losses, rewards), "bit for bit"
