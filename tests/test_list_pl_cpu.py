"""CPU suite: the contract of the differentiable Plackett-Luce slate likelihood (``evaluate.list_pl`` / ``pl_scores``).  The host twin's
coefficient is held to central finite differences of ``pl_log_prob_host`` and to float64 autograd of a slate-at-a-time likelihood
written without ``evaluate``'s helpers; ``list_pl_grad_host`` and the CPU-tensor path of ``list_pl`` / ``pl_scores`` to each other at
1e-10 on inputs whose inner products are exact in float32; ListMLE to its textbook form; the refusals; and ``nrms.policy_step``,
``fit_policy`` and ``fit_from_logs`` on CPU tensors for NRMS and NRMS-SA."""
import numpy as np
import pytest
import torch

import list_pl_common as LPL
import nrms_common as NC
import pool_softmax_common as PC


def _exact_case(rng, G, M, d, k, S, **kw):
    """``list_pl_common.case`` without planted rows, users and rows on a grid of 1/8 with few channels: every inner product is a
    multiple of 1/64 below 2^10 — the same number in float32 and in float64."""
    users, rows, ids, count, picks, weight, kind = LPL.case(rng, G, M, d, k, S, plant=False, **kw)
    users = (np.round(users * 8.0) / 8.0).astype(np.float32)
    rows = (np.round(np.clip(rows, -3, 3) * 8.0) / 8.0).astype(np.float32)
    return users, rows, ids, count, picks, weight, kind


def _scores(users, rows, ids):
    ok = (ids >= 0) & (ids < len(rows))
    S = users.astype(np.float64) @ rows.astype(np.float64).T
    return np.where(ok, S[np.arange(len(ids))[:, None], np.where(ok, ids, 0)], 0.0).astype(np.float32)


def test_the_generator_makes_every_kind_of_slate():
    rng = np.random.default_rng(0)
    users, rows, ids, count, picks, weight, kind = LPL.case(rng, 9, 9, 4, 4, 3)
    assert set(kind.reshape(-1)) == set(range(len(LPL.SLATE_KINDS)))
    assert (weight == 0).any() and (weight > 0).any() and (weight < 0).any()
    assert (count == 0).any() and (ids < 0).any() and (ids >= len(rows)).any() and (ids[:, 0] == ids[:, 1]).any()
    from digat_amd import evaluate
    with np.errstate(all="ignore"):                                 # the float32 chain, channel by channel
        prod = (users[:, None, :] * rows[np.clip(ids, 0, len(rows) - 1)]).astype(np.float32)
        chain = np.zeros(ids.shape, dtype=np.float32)
        for c in range(users.shape[1]):
            chain = chain + prod[:, :, c]
    assert np.isfinite(rows).all() and np.isfinite(users).all()
    assert np.isposinf(chain).any() and np.isneginf(chain).any() and np.isnan(chain).any(), "planted through finite rows"
    lens = evaluate.pl_log_prob_host(np.where(LPL.elements(ids, count, len(rows)), chain, np.float32(np.nan)), count, picks, 1.0,
                                     parts=True)[2]["length"]
    assert (lens == 0).any() and (lens == 4).any() and ((lens > 0) & (lens < 4)).any()


@pytest.mark.parametrize("M,k,S", [(9, 4, 3), (5, 3, 2), (1, 1, 1), (2, 4, 2)])
def test_host_coefficient_against_finite_differences(M, k, S):
    """``pl_log_prob_host`` reads float32 scores: they sit on a grid of 2^-12 and move by h = 2^-8, so every perturbed score is exact.
    The central difference is off by h^2 / 6 |f'''| with |f'''| <= 8 k inv_t^3 at most: 2^-16 / 6 * 8 * 4 * 8 < 7e-4 at inv_t = 2; the
    tolerance is 1e-3 of max(1, |coef|)."""
    from digat_amd import evaluate
    rng = np.random.default_rng(100 * M + k)
    G = 6
    scores = (np.round(rng.standard_normal((G, M)) * 2.0 * 4096.0) / 4096.0).astype(np.float32)
    scores[0, 0] = np.nan
    count = rng.integers(0, M + 1, size=G).astype(np.int32)
    count[:2] = M
    ids = np.zeros((G, M), dtype=np.int64)
    picks, _ = LPL.slates(rng, ids, count, 1, k, S)
    gl = LPL.weights(rng, G, S)
    T, scale = 0.5, 1.0
    coef = evaluate.list_pl_host(scores, None, count, picks, 0, scale, T, grad_logp=gl)[2]
    h = 2.0 ** -8
    for g in range(G):
        for j in range(M):
            if not (j < count[g] and np.isfinite(scores[g, j])):
                assert coef[g, j] == 0
                continue
            up, dn = scores.copy(), scores.copy()
            up[g, j] += np.float32(h)
            dn[g, j] -= np.float32(h)
            f = [(evaluate.pl_log_prob_host(x[g:g + 1], count[g:g + 1], picks[g:g + 1], T)[0][0] * gl[g]).sum() for x in (up, dn)]
            fd = (f[0] - f[1]) / (2 * h)
            assert abs(fd - coef[g, j]) <= 1e-3 * max(1.0, abs(coef[g, j])), (g, j, fd, coef[g, j])


@pytest.mark.parametrize("G,M,d,k,S", [(7, 9, 3, 4, 3), (3, 33, 4, 10, 2), (1, 1, 1, 1, 1), (8, 12, 2, 128, 1)])
def test_twins_and_the_cpu_path_agree_in_float64(G, M, d, k, S):
    from digat_amd import evaluate
    rng = np.random.default_rng(7 * G + M)
    users, rows, ids, count, picks, gl, _ = _exact_case(rng, G, M, d, k, S)
    P = len(rows)
    sc = _scores(users, rows, ids)
    scale, T = 0.75, 0.5
    inv_t = evaluate._pl_inv_t(scale, T)
    logp, step, coef, parts = evaluate.list_pl_host(sc, ids, count, picks, P, scale, T, grad_logp=gl, parts=True)
    live = LPL.elements(ids, count, P)
    # an independent float64 likelihood, one slate at a time
    s_logp, s_coef = LPL.stock_fp64(sc, live, picks, inv_t, gl)
    assert np.abs(logp - s_logp).max() <= 1e-10 and np.abs(coef - s_coef).max() <= 1e-10
    assert (coef[~live] == 0).all() and (parts["absolute"] >= np.abs(coef) - 1e-12).all()
    # at scale 1 the forward is pl_log_prob_host's, bit for bit
    a, b = evaluate.list_pl_host(sc, None, count, picks, 0, 1.0, T)[:2], evaluate.pl_log_prob_host(sc, count, picks, T)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the CPU-tensor path: the stock composition under autograd
    U = torch.tensor(users, dtype=torch.float64, requires_grad=True)
    R = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    t_logp, t_step, t_scores = evaluate.list_pl(U, R, torch.from_numpy(ids), torch.from_numpy(count), torch.from_numpy(picks), scale, T)
    assert t_logp.requires_grad and not t_step.requires_grad and not t_scores.requires_grad and t_logp.dtype == torch.float64
    assert np.array_equal(np.isnan(t_scores.numpy()), ~live) and np.array_equal(t_scores.numpy()[live], sc[live].astype(np.float64))
    (t_logp * torch.from_numpy(gl)).sum().backward()
    dU, dR = evaluate.list_pl_grad_host(users, rows, sc, ids, count, picks, scale, T, gl)
    for got, want, name in ((t_logp.detach().numpy(), logp, "logp"), (t_step.numpy(), parts["step"], "step"), (U.grad.numpy(), dU, "d_users"),
                            (R.grad.numpy(), dR, "d_rows")):
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), name
    # pl_scores on the same scores: the same likelihood, its gradient the coefficient
    X = torch.tensor(np.where(live, sc, np.nan).astype(np.float64), requires_grad=True)
    p_logp, p_step = evaluate.pl_scores(X, torch.from_numpy(count), torch.from_numpy(picks), 1.0 / inv_t)
    (p_logp * torch.from_numpy(gl)).sum().backward()
    w = evaluate.list_pl_host(sc, ids, count, picks, P, 1.0, 1.0 / inv_t, grad_logp=gl)
    assert np.abs(p_logp.detach().numpy() - w[0]).max() <= 1e-10 and np.abs(X.grad.numpy() - w[2]).max() <= 1e-10


def test_listmle_is_the_likelihood_of_the_ground_truth_order():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    G, M = 4, 7
    s = rng.standard_normal((G, M))
    y = rng.permutation(M)[None, :].repeat(G, 0) + rng.random((G, M))            # labels: their descending order is the slate
    order = np.argsort(-y, axis=1)
    X = torch.tensor(s, requires_grad=True)
    logp, _ = evaluate.pl_scores(X, None, torch.from_numpy(order[:, None, :].astype(np.int64)), 1.0)
    ss = torch.tensor(s).gather(1, torch.from_numpy(order))
    textbook = sum(torch.logsumexp(ss[:, t:], dim=1) - ss[:, t] for t in range(M))
    assert torch.allclose(-logp[:, 0], textbook, rtol=0, atol=1e-12)
    assert np.abs(-logp.detach().numpy()[:, 0] - -evaluate.pl_log_prob_host(s.astype(np.float32), None, order[:, None, :], 1.0)[0][:, 0]).max() < 1e-5


def test_refusals():
    from digat_amd import evaluate
    U, R = torch.zeros(3, 4), torch.zeros(5, 4)
    ids, picks = torch.zeros(3, 6, dtype=torch.int64), torch.zeros(3, 2, 3, dtype=torch.int64)
    ok = evaluate.list_pl(U, R, ids, None, picks)
    assert ok[0].shape == (3, 2) and ok[1].shape == (3, 2, 3) and ok[2].shape == (3, 6)
    bad = [lambda: evaluate.list_pl(U, R, ids, None, picks.float()), lambda: evaluate.list_pl(U, R, ids, None, picks[:2]),
           lambda: evaluate.list_pl(U, R, ids, None, picks[:, :, 0]), lambda: evaluate.list_pl(U, R, ids, None, torch.zeros(3, 1, 129, dtype=torch.int64)),
           lambda: evaluate.list_pl(U, R, torch.zeros(3, 1025, dtype=torch.int64), None, picks),
           lambda: evaluate.list_pl(torch.zeros(3, 513), torch.zeros(5, 513), ids, None, picks),
           lambda: evaluate.list_pl(U, R, ids.float(), None, picks), lambda: evaluate.list_pl(U, R[:, :3], ids, None, picks),
           lambda: evaluate.list_pl(U, R, ids, torch.zeros(2, dtype=torch.int64), picks), lambda: evaluate.list_pl(U.long(), R, ids, None, picks),
           lambda: evaluate.list_pl(U, R, ids, None, picks, temperature=0.0), lambda: evaluate.list_pl(U, R, ids, None, picks, temperature=float("nan")),
           lambda: evaluate.list_pl(U, R, ids, None, picks, temperature=float("inf")), lambda: evaluate.list_pl(U, R, ids, None, picks, scale=0.0),
           lambda: evaluate.list_pl(U, R, ids, None, picks, scale=-1.0), lambda: evaluate.list_pl(U, R, ids, None, picks, temperature=1e-320),
           lambda: evaluate.pl_scores(torch.zeros(3, 6), None, picks.float(), 1.0), lambda: evaluate.pl_scores(torch.zeros(3, 6), None, picks, 0.0),
           lambda: evaluate.pl_scores(torch.zeros(3, 1025), None, picks, 1.0), lambda: evaluate.pl_scores(torch.zeros(3, 6).long(), None, picks, 1.0),
           lambda: evaluate.pl_scores(torch.zeros(3, 6), None, torch.zeros(3, 1, 129, dtype=torch.int64), 1.0),
           lambda: evaluate.list_pl_host(np.zeros((3, 6), np.float32), None, None, picks.numpy(), 0, grad_logp=np.zeros((3, 3))),
           lambda: evaluate.list_pl_host(np.zeros((3, 6), np.float32), None, None, picks.numpy().astype(np.float32), 0)]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {n} went through")
    # no list and an empty table: defined, with a zero gradient
    Ug = U.clone().requires_grad_(True)
    logp, step, scores = evaluate.list_pl(Ug, R[:0], ids, None, picks)
    assert (logp == 0).all() and (step == 0).all() and torch.isnan(scores).all()
    logp.sum().backward()
    assert (Ug.grad == 0).all()
    assert evaluate.list_pl(U[:0], R, ids[:0], None, picks[:0])[0].shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the training surface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_policy_step_on_cpu_tensors(pre):
    from digat_amd import nrms
    users, ids, gain, count, slates, weight = LPL.policy_lists()
    dev, U = LPL.train_set()
    m = PC.double_twin(NC.model(LPL.STEP_FIXTURE, pre))
    m.train()
    loss, logp = nrms.policy_step(m, dev, users, ids, slates, weight, count, scale=2.0, temperature=0.5)
    assert loss.requires_grad and not logp.requires_grad and logp.shape == (U, 3) and np.isfinite(float(loss.detach()))
    assert (logp[:, 2] == 0).all() and (logp[:, 0] < 0).all(), "a slate that starts with -1 is empty"
    n = int((weight[:, :2] != 0).sum())                             # the first two slates of every user begin with a live news
    assert abs(float(loss.detach()) - float(-(torch.from_numpy(weight) * logp).sum() / n)) < 1e-12
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    again, _ = nrms.policy_step(m, dev, users, ids, slates, weight, count, scale=2.0, temperature=0.5)
    assert float(again.detach()) == float(loss.detach())
    with pytest.raises(ValueError):
        nrms.policy_step(m, dev, users, ids, slates, weight[:, :2], count)
    with pytest.raises(ValueError):
        nrms.policy_step(m, dev, users, ids, slates.astype(np.float32), weight, count)


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_fit_policy_and_fit_from_logs_on_cpu_tensors(pre, monkeypatch):
    from digat_amd import evaluate, nrms
    users, ids, gain, count, slates, weight = LPL.policy_lists()
    dev, U = LPL.train_set()
    seen = {"policy": [], "rank": []}
    real_policy, real_rank = nrms.policy_step, nrms.rank_step
    monkeypatch.setattr(nrms, "policy_step", lambda model, train, u, *a, **k: (seen["policy"].append(np.asarray(u).copy()), real_policy(model, train, u, *a, **k))[1])
    monkeypatch.setattr(nrms, "rank_step", lambda model, train, u, *a, **k: (seen["rank"].append(np.asarray(u).copy()), real_rank(model, train, u, *a, **k))[1])
    lists = (users, ids, gain, count)

    def run():
        torch.manual_seed(3)
        m = NC.model(LPL.STEP_FIXTURE, pre)
        return nrms.fit_policy(m, dev, lists, steps=3, k=3, samples=3, temperature=0.7, batch_users=3, lr=1e-3, seed=11, scale=1.5)
    losses, rewards = run()
    assert len(losses) == len(rewards) == 3 and np.isfinite(losses).all() and all(0.0 <= r <= 1.0 for r in rewards)
    assert run() == (losses, rewards), "seeded: the same draws, the same losses"
    torch.manual_seed(3)
    nrms.fit_ranker(NC.model(LPL.STEP_FIXTURE, pre), dev, lists, steps=3, batch_users=3, lr=1e-3, seed=11)
    assert len(seen["rank"]) == 3 and all(np.array_equal(a, b) for a, b in zip(seen["policy"][:3], seen["rank"])), "fit_ranker's draws"
    one = nrms.fit_policy(NC.model(LPL.STEP_FIXTURE, pre), dev, lists, steps=2, k=3, samples=1, batch_users=3, seed=11)
    assert np.isfinite(one[0]).all()
    # a log: slates drawn from the lists under some scores, their propensities, a reward per slate
    rng = np.random.default_rng(4)
    logged_scores = rng.standard_normal(ids.shape).astype(np.float32)
    picks, _, logged_logp, _ = evaluate.pl_sample_host(logged_scores, count, 3, 1.0, seed=2, samples=3)
    sl = np.where(picks >= 0, np.take_along_axis(ids, np.clip(picks, 0, None).reshape(U, -1), axis=1).reshape(picks.shape), -1)
    log = {"ids": torch.from_numpy(ids), "count": torch.from_numpy(count), "slates": torch.from_numpy(sl), "logp": torch.from_numpy(logged_logp),
           "temperature": 1.0}
    reward = rng.random((U, 3))

    def run_log(**kw):
        torch.manual_seed(3)
        return nrms.fit_from_logs(NC.model(LPL.STEP_FIXTURE, pre), dev, log, reward, steps=3, users=users, batch_users=3, lr=1e-3, seed=11, **kw)
    a = run_log()
    assert len(a) == 3 and np.isfinite(a).all() and run_log() == a
    assert all(x == 0.0 for x in run_log(clip=1e-30)), "every weight clipped: nothing to learn from"
    with pytest.raises(ValueError):
        nrms.fit_from_logs(NC.model(LPL.STEP_FIXTURE, pre), dev, log, reward, steps=1)


def test_slate_log_prob_differentiable_on_cpu_tensors():
    from digat_amd import evaluate, util
    rng = np.random.default_rng(8)
    G, M = 5, 9
    ids = torch.from_numpy(np.stack([rng.permutation(50)[:M] for _ in range(G)]).astype(np.int64))
    scores = torch.from_numpy(rng.standard_normal((G, M)).astype(np.float32))
    count = torch.full((G,), M, dtype=torch.int32)
    slates = ids[:, None, [3, 0, 5]].clone()
    slates[1, 0, 1] = 77                                            # absent: the slate ends there
    plain = util.slate_log_prob(ids, scores, count, slates, 0.5)
    X = scores.double().requires_grad_(True)
    logp, step, covered = util.slate_log_prob(ids, X, count, slates, 0.5, differentiable=True)
    assert logp.requires_grad and torch.equal(covered, plain[2]) and not covered[1, 0]
    assert np.abs(logp.detach().numpy() - plain[0].numpy()).max() < 1e-12
    logp.sum().backward()
    coef = evaluate.list_pl_host(scores.numpy(), None, count.numpy(), util.slate_positions(ids, count, slates).numpy(), 0, 1.0, 0.5,
                                 grad_logp=np.ones((G, 1)))[2]
    assert np.abs(X.grad.numpy() - coef).max() < 1e-12
