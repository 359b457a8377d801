"""CPU suite: the PL-Rank estimator (``evaluate.plrank_host``, ``plrank_grad_host``, ``list_plrank`` and ``plrank_scores`` on CPU
tensors, ``nrms.plrank_step`` / ``fit_policy(estimator="plrank")``).  The formula is held to an ENUMERATION of every ordered slate:
its mean under the policy is the exact gradient of the expected metric, and its exact variance lies below single-sample REINFORCE's.
If the formula and the enumeration ever disagree, the enumeration decides."""
import numpy as np
import pytest
import torch

import list_pl_common as LPL
import nrms_common as NC
import plrank_common as PR


def _terms(M, k, seed):
    """The per-slate terms of ``plrank_host`` for every ordered slate of the fixture, given as the S slates of one list."""
    from digat_amd import evaluate
    scores, rho, theta = PR.fixture(M, k, seed)
    slates, pi, R, grad, score = PR.enumeration(M, k, seed)
    value, sv, parts = evaluate.plrank_host(scores[None], None, None, slates[None], rho[None], 0, discount=theta, parts=True)
    assert np.abs(sv[0] - R).max() <= 1e-14 and abs(value[0] - R.mean()) <= 1e-14 and (parts["length"] == k).all()
    return parts["terms"][0], slates, pi, R, grad, score


@pytest.mark.parametrize("M,k,seed", PR.FIXTURES)
def test_the_mean_over_every_ordered_slate_is_the_exact_gradient(M, k, seed):
    terms, slates, pi, R, grad, _ = _terms(M, k, seed)
    mean = (pi[:, None] * terms).sum(axis=0)
    print((M, k, seed), "slates", len(slates), "worst |mean - exact gradient|", np.abs(mean - grad).max())
    assert np.abs(mean - grad).max() <= 1e-12


def test_the_fixtures_cover_the_shapes():
    assert {(5, 3), (5, 5), (6, 2)} <= {(M, k) for M, k, _ in PR.FIXTURES} and any(k == 1 for _, k, _ in PR.FIXTURES)


@pytest.mark.parametrize("M,k,seed", PR.FIXTURES)
def test_the_exact_variance_lies_below_reinforce(M, k, seed):
    """Total variance over the M coordinates of one slate's estimate, by enumeration: PL-Rank against ``R d log pi / d a`` with no
    baseline.  Both have the same mean (the test above; the score function's mean is 0)."""
    terms, slates, pi, R, grad, score = _terms(M, k, seed)
    reinforce = R[:, None] * score
    assert np.abs((pi[:, None] * reinforce).sum(axis=0) - grad).max() <= 1e-12
    var = lambda x: float((pi[:, None] * (x - grad[None, :]) ** 2).sum())
    ratio = var(terms) / var(reinforce)
    quoted = PR.QUOTED_RATIOS[PR.FIXTURES.index((M, k, seed))]
    print((M, k, seed), "variance PL-Rank", var(terms), "REINFORCE", var(reinforce), "ratio", ratio, "quoted", quoted)
    assert var(terms) < var(reinforce)
    assert abs(ratio - quoted) <= 1e-3, "the ratio measured when the estimator was chosen"


def test_k_equal_one():
    from digat_amd import evaluate
    M, k, seed = 4, 1, 4
    terms, slates, pi, R, grad, _ = _terms(M, k, seed)
    scores, rho, theta = PR.fixture(M, k, seed)
    a = scores.astype(np.float64)
    p = np.exp(a - a.max()) / np.exp(a - a.max()).sum()
    for y, t in zip(slates[:, 0], terms):
        assert abs(t[y]) <= 1e-15, "the picked slot's term"
        want = p * theta[0] * (rho.astype(np.float64) - float(rho[y]))
        others = np.arange(M) != y
        assert np.abs(t[others] - want[others]).max() <= 1e-15


def _numpy_scores(users, rows, ids):
    with np.errstate(all="ignore"):                                 # the float32 chain, channel by channel: the planted rows overflow
        prod = (users[:, None, :] * rows[np.clip(ids, 0, len(rows) - 1)]).astype(np.float32)
        chain = np.zeros(ids.shape, dtype=np.float32)
        for c in range(users.shape[1]):
            chain = chain + prod[:, :, c]
    return chain


def test_contractual_zeros():
    from digat_amd import evaluate
    rng = np.random.default_rng(5)
    G, M, d, k, S = 12, 9, 4, 4, 3
    users, rows, ids, count, picks, _, kind = LPL.case(rng, G, M, d, k, S)
    assert set(kind.reshape(-1)) == set(range(len(LPL.SLATE_KINDS))), "every kind of slate"
    P = len(rows)
    sc = _numpy_scores(users, rows, ids)
    elem = LPL.elements(ids, count, P)
    live = elem & np.isfinite(sc)
    assert (elem & ~np.isfinite(sc)).any() and (~elem).any()
    gain, clean = PR.odd_gains(rng, G, M)
    assert np.isnan(gain).any() and np.isposinf(gain).any() and np.isneginf(gain).any() and (gain < 0).any()
    gv = rng.standard_normal(G)
    gv[3] = 0.0
    lw = rng.random(G) + 0.5
    value, sv, coef, parts = evaluate.plrank_host(sc, ids, count, picks, gain, P, None, lw, 0.75, 1.5, grad_value=gv, parts=True)
    assert (parts["terms"][~np.broadcast_to(live[:, None, :], (G, S, M))] == 0).all(), "a slot that is not live"
    assert (coef[~live] == 0).all() and (parts["absolute"][~live] == 0).all() and (coef[3] == 0).all()
    empty = parts["length"] == 0
    assert empty.any() and (parts["terms"][empty] == 0).all() and (sv[empty] == 0).all(), "an empty slate adds nothing"
    assert (parts["length"][kind == LPL.SLATE_KINDS.index("empty")] == 0).all()
    assert np.isfinite(coef).all() and np.isfinite(value).all() and (np.abs(coef) <= parts["absolute"] + 1e-12).all()
    # an empty slate still counts in S: the value is the sum over S slates divided by S
    assert np.abs(value - lw * sv.sum(axis=1) / S).max() <= 1e-12
    # NaN, infinite and negative gains count as 0
    again = evaluate.plrank_host(sc, ids, count, picks, clean, P, None, lw, 0.75, 1.5, grad_value=gv)
    assert np.array_equal(again[0], value) and np.array_equal(again[1], sv) and np.array_equal(again[2], coef)
    # a slate cut short is the metric truncated at its length
    theta = evaluate.ndcg_discount(k)
    for g in range(G):
        for s in range(S):
            n = int(parts["length"][g, s])
            assert abs(sv[g, s] - float(np.dot(theta[:n], clean[g, picks[g, s, :n]]))) <= 1e-12


@pytest.mark.parametrize("G,M,d,k,S,scale,T", [(7, 9, 3, 4, 3, 1.0, 0.5), (3, 33, 4, 10, 2, 0.75, 1.5), (1, 1, 1, 1, 1, 1.0, 1.0)])
def test_list_plrank_on_cpu_tensors(G, M, d, k, S, scale, T):
    from digat_amd import evaluate
    rng = np.random.default_rng(11 * G + M)
    users, rows, ids, count, _, _, _ = LPL.case(rng, G, M, d, k, S, plant=False)
    rows = np.clip(rows, -3, 3)
    P = len(rows)
    gain, _ = PR.odd_gains(rng, G, M)
    lw = rng.random(G) + 0.5
    streams = rng.integers(0, 1 << 20, size=G)
    U = torch.tensor(users, dtype=torch.float64, requires_grad=True)
    R = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    gv = rng.standard_normal(G)
    value, sv, picks, scores = evaluate.list_plrank(U, R, torch.from_numpy(ids), torch.from_numpy(count), torch.from_numpy(gain), k, S, None, lw,
                                                    scale, T, seed=9, first_sample=5, streams=torch.from_numpy(streams))
    assert value.requires_grad and not sv.requires_grad and not picks.requires_grad and not scores.requires_grad
    assert value.dtype == sv.dtype == torch.float64 and picks.dtype == torch.int32 and picks.shape == (G, S, k) and sv.shape == (G, S)
    sc = scores.numpy()
    if scale == 1.0:
        want = evaluate.pl_sample_host(sc.astype(np.float32), count, k, T, seed=9, samples=S, first_sample=5, streams=streams)[0]
        assert np.array_equal(picks.numpy(), want), "pl_sample_host's picks"
    w_value, w_sv = evaluate.plrank_host(sc, ids, count, picks.numpy(), gain, P, None, lw, scale, T)
    assert np.array_equal(value.detach().numpy(), w_value) and np.array_equal(sv.numpy(), w_sv)
    (value * torch.from_numpy(gv)).sum().backward()
    dU, dR = evaluate.plrank_grad_host(users, rows, sc, ids, count, picks.numpy(), gain, None, lw, scale, T, gv)
    for got, want, name in ((U.grad.numpy(), dU, "d_users"), (R.grad.numpy(), dR, "d_rows")):
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), name
    # given picks: the same numbers; plrank_scores on the same scores: the same value, its gradient the coefficient
    given = evaluate.list_plrank(U, R, torch.from_numpy(ids), torch.from_numpy(count), torch.from_numpy(gain), k, 1, None, lw, scale, T, picks=picks)
    assert np.array_equal(given[0].detach().numpy(), w_value) and torch.equal(given[2], picks)
    X = torch.tensor(sc, requires_grad=True)
    inv_t = evaluate._pl_inv_t(scale, T)
    s_value, s_sv, s_picks = evaluate.plrank_scores(X, torch.from_numpy(count), torch.from_numpy(gain), k, S, None, lw, 1.0 / inv_t, picks=picks)
    (s_value * torch.from_numpy(gv)).sum().backward()
    coef = evaluate.plrank_host(sc, None, count, picks.numpy(), gain, 0, None, lw, 1.0, 1.0 / inv_t, grad_value=gv)[2]
    assert np.abs(X.grad.numpy() - coef).max() <= 1e-12 and np.array_equal(s_sv.numpy(), w_sv)


def test_refusals():
    from digat_amd import evaluate
    U, R = torch.zeros(2, 3), torch.zeros(4, 3)
    ids, gain = torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5)
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain[:, :4], 3)
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 129)
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 3, discount=np.array([1.0, -1.0, 0.5]))
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 3, discount=np.ones(2))
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 3, list_weight=np.array([1.0, np.inf]))
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 3, samples=2, first_sample=evaluate.PL_MAX_SAMPLE - 1)
    with pytest.raises(ValueError):
        evaluate.list_plrank(U, R, ids, None, gain, 3, picks=torch.zeros(2, 1, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        evaluate.plrank_scores(torch.zeros(2, 5), None, gain, 3, temperature=0.0)


def test_abi_names_are_exported():
    from digat_amd import _lib
    for name in ("digat_list_plrank_fwd", "digat_plrank_scores_fwd", "digat_plrank_scores_bwd", "digat_list_plrank_bwd",
                 "digat_list_plrank_workspace_bytes"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("pre", list(NC.MODELS))
def test_fit_policy_with_the_plrank_estimator_on_cpu_tensors(pre, monkeypatch):
    from digat_amd import nrms
    users, ids, gain, count, _, _ = LPL.policy_lists()
    dev, U = LPL.train_set()
    lists = (users, ids, gain, count)
    seen = {"plrank": [], "rank": []}
    real_plrank, real_rank = nrms.plrank_step, nrms.rank_step
    monkeypatch.setattr(nrms, "plrank_step", lambda model, train, u, *a, **k: (seen["plrank"].append((np.asarray(u).copy(), k["first_sample"])),
                                                                               real_plrank(model, train, u, *a, **k))[1])
    monkeypatch.setattr(nrms, "rank_step", lambda model, train, u, *a, **k: (seen["rank"].append(np.asarray(u).copy()), real_rank(model, train, u, *a, **k))[1])

    def run():
        torch.manual_seed(3)
        m = NC.model(LPL.STEP_FIXTURE, pre)
        return nrms.fit_policy(m, dev, lists, steps=3, k=3, samples=3, temperature=0.7, batch_users=3, lr=1e-3, seed=11, scale=1.5, estimator="plrank")
    losses, rewards = run()
    assert len(losses) == len(rewards) == 3 and np.isfinite(losses).all() and all(0.0 <= r <= 1.0 for r in rewards)
    assert run() == (losses, rewards), "seeded: the same draws, the same losses"
    assert [f for _, f in seen["plrank"][:3]] == [0, 3, 6], "first_sample = step * samples"
    torch.manual_seed(3)
    nrms.fit_ranker(NC.model(LPL.STEP_FIXTURE, pre), dev, lists, steps=3, batch_users=3, lr=1e-3, seed=11)
    assert all(np.array_equal(a[0], b) for a, b in zip(seen["plrank"][:3], seen["rank"])), "fit_ranker's draws"
    with pytest.raises(ValueError, match="estimator"):
        nrms.fit_policy(NC.model(LPL.STEP_FIXTURE, pre), dev, lists, steps=1, estimator="pl-rank")
    # one step: the loss is minus the mean value, the gradient reaches every parameter
    m = NC.model(LPL.STEP_FIXTURE, pre)
    m.train()
    torch.manual_seed(1)
    loss, reward = nrms.plrank_step(m, dev, users, ids, gain, count, k=3, samples=4, scale=1.5, temperature=0.7, seed=2, first_sample=8)
    assert loss.requires_grad and not reward.requires_grad and abs(float(loss.detach()) + float(reward)) <= 1e-12, "every list has a click"
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
