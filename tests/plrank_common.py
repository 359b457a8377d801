"""Shared by tests/test_plrank_cpu.py and tests/test_hip_plrank.py: the small fixtures on which the PL-Rank estimator is held to an
enumeration of EVERY ordered slate — the policy's probabilities, the expected metric and its exact gradient in float64 under
``torch.autograd``, written without ``evaluate``'s helpers — and gains with values that count as 0."""
import functools
import itertools

import numpy as np
import torch

# (M, k, seed): 3 of 5 twice, 2 of 6, 5 of 5, k = 1 and 4 of 6; a = 1.5 normal(M), rho = integers(0, 3, M) from the same generator
FIXTURES = ((5, 3, 0), (5, 3, 1), (6, 2, 2), (5, 5, 3), (4, 1, 4), (6, 4, 5))
# the variance of the estimator over single-sample REINFORCE's without a baseline, as measured in float64 when the estimator was chosen
QUOTED_RATIOS = (0.146, 0.295, 0.228, 0.386, 0.408, 0.504)


def fixture(M, k, seed):
    """``(scores float32 [M], rho float32 [M], theta float64 [k])``; the scores are the float32 roundings of ``a``."""
    rng = np.random.default_rng(seed)
    a = 1.5 * rng.normal(size=M)
    rho = rng.integers(0, 3, size=M)
    return a.astype(np.float32), rho.astype(np.float32), 1.0 / np.log2(np.arange(k) + 2.0)


@functools.lru_cache(maxsize=None)
def enumeration(M, k, seed):
    """Every ordered slate of k of the M items: ``(slates [Y, k] int32, pi [Y], R [Y], exact gradient of sum_y pi R [M], score
    [Y, M] = d log pi_y / d a)``, float64 numpy — the probabilities as products of softmax steps under ``torch.autograd``."""
    scores, rho, theta = fixture(M, k, seed)
    a = torch.tensor(scores.astype(np.float64), requires_grad=True)
    slates = np.array(list(itertools.permutations(range(M), k)), dtype=np.int32)
    logp = []
    for y in slates:
        left = list(range(M))
        lp = a.sum() * 0.0
        for p in y:
            lp = lp + a[int(p)] - torch.logsumexp(a[left], dim=0)
            left.remove(int(p))
        logp.append(lp)
    logp = torch.stack(logp)
    R = torch.tensor([float(np.dot(theta, rho[y].astype(np.float64))) for y in slates], dtype=torch.float64)
    J = (torch.exp(logp) * R).sum()
    grad = torch.autograd.grad(J, a, retain_graph=True)[0].numpy().copy()
    score = np.stack([torch.autograd.grad(lp, a, retain_graph=True)[0].numpy() for lp in logp])
    pi = torch.exp(logp).detach().numpy()
    assert abs(pi.sum() - 1.0) < 1e-12
    return slates, pi, R.numpy(), grad, score


def odd_gains(rng, G, M):
    """``(gain float32 [G, M] with NaN, +-inf and negative values planted, the same with those at 0)``."""
    clean = rng.integers(0, 4, size=(G, M)).astype(np.float32) * np.float32(0.5)
    gain = clean.copy()
    kind = rng.integers(0, 8, size=(G, M))
    for code, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, -1.5)):
        gain[kind == code] = bad
    clean[kind < 4] = 0
    return gain, clean
