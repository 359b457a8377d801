"""Shared by tests/test_pool_softmax_cpu.py and tests/test_hip_pool_softmax.py: the stock composition of the full-pool softmax loss in
float64 under ``torch.autograd`` (product, masked ``logsumexp``, gather), cases with the targets a tiled kernel can get wrong, and
the float64 CPU twin of an NRMS model for ``nrms.retrieval_step``."""
import copy

import numpy as np
import torch

import dot_rank_common as R

PER_USER = (0, 1, 5, 70)


def stock_fp64(users, news, pos, start, pool=None, skip=None, scale=1.0, grad_loss=None):
    """``(loss [T], lse [G], ranked [T] bool, d_users [G, d], d_rows [P, d])`` in float64: ``torch.autograd`` through the product of
    ``users`` with the row of every pool position (zeros where the id is no row of ``news``), ``logsumexp`` over the user's elements
    and the gather of the targets.  Written without ``evaluate``'s helpers: ids by a Python set per user."""
    U = torch.tensor(np.asarray(users, dtype=np.float64), requires_grad=True)
    N = len(news)
    P = N if pool is None else len(pool)
    ids = np.arange(P) if pool is None else np.asarray(pool, dtype=np.int64)
    valid = (ids >= 0) & (ids < N)
    rows = np.zeros((P, U.shape[1]))
    rows[valid] = np.asarray(news, dtype=np.float64)[ids[valid]]
    Rw = torch.tensor(rows, requires_grad=True)
    G, T = U.shape[0], len(pos)
    elem = np.zeros((G, P), dtype=bool)
    for g in range(G):
        banned = set() if skip is None else {int(v) for v in skip[g]}
        elem[g] = [bool(valid[p]) and int(ids[p]) not in banned for p in range(P)]
    x = float(scale) * (U @ Rw.t())
    lse = torch.full((G,), float("-inf"), dtype=torch.float64)
    terms = []
    ranked = np.zeros(T, dtype=bool)
    loss = [torch.zeros((), dtype=torch.float64)] * T
    gl = np.ones(T) if grad_loss is None else np.asarray(grad_loss, dtype=np.float64)
    lse_list = []
    for g in range(G):
        cols = np.flatnonzero(elem[g])
        l = torch.logsumexp(x[g, cols], dim=0) if len(cols) else torch.tensor(float("-inf"), dtype=torch.float64)
        lse_list.append(l)
        for t in range(int(start[g]), int(start[g + 1])):
            q = int(pos[t])
            if 0 <= q < P and elem[g, q]:
                ranked[t] = True
                loss[t] = l - x[g, q]
                terms.append(gl[t] * loss[t])
    if terms:
        torch.stack(terms).sum().backward()
    dU = U.grad.numpy() if U.grad is not None else np.zeros(tuple(U.shape))
    dR = Rw.grad.numpy() if Rw.grad is not None else np.zeros(tuple(Rw.shape))
    return (np.array([float(v.detach()) for v in loss]), np.array([float(v.detach()) for v in lse_list]), ranked, dU, dR)


def case(rng, G, P, d, pool, skip, skip_len=50):
    """``(users [G,d], news [N,d], pool [P] or None, skip [G, skip_len] or None)`` float32 / int64: an unsorted pool with repeats, skip
    rows drawn from the pool's ids with repeats."""
    N = P + 37 if pool else P
    users = rng.standard_normal((G, d)).astype(np.float32)
    news = rng.standard_normal((N, d)).astype(np.float32)
    pl = rng.integers(0, N, size=P).astype(np.int64) if pool else None
    sk = None
    if skip:
        src = pl if pool else np.arange(P, dtype=np.int64)
        sk = np.stack([src[rng.integers(0, P, size=skip_len)] for _ in range(G)])
    return users, news, pl, sk


def targets(rng, G, P, skip, pool, chunk, per_user=PER_USER, rot=0):
    """``dot_rank_common.make_targets`` — both sides of every chunk edge — plus, where the user has room for them: a repeated target, a
    target outside [0, P) on either side and a target inside the user's skip row."""
    per = per_user[rot % len(per_user):] + per_user[:rot % len(per_user)]
    pos, start = R.make_targets(rng, G, P, per, chunk)
    ids = np.arange(P, dtype=np.int64) if pool is None else pool
    for g in range(G):
        a, b = int(start[g]), int(start[g + 1])
        if b - a >= 5:
            pos[a + 1] = pos[a]                                    # a repeated target
            pos[a + 2], pos[a + 3] = -1 - g, P + g                 # outside the pool
            if skip is not None:
                hit = np.flatnonzero(ids == skip[g, 0])
                if len(hit):
                    pos[a + 4] = hit[0]                            # inside the skip row
    return pos, start


def rows_of(news, pool):
    """[P, d] float64: the row of every pool position."""
    news = np.asarray(news, dtype=np.float64)
    return news if pool is None else news[np.asarray(pool)]


def double_twin(model):
    """A float64 CPU copy of an NRMS model."""
    return copy.deepcopy(model).cpu().double()
