"""Shared by tests/test_list_softmax_cpu.py and tests/test_hip_list_softmax.py: the stock composition of the per-user list softmax in
float64 under ``torch.autograd`` (gather, product, ``logsumexp``, KL), and cases with the lists a kernel can get wrong — ids outside
the table, counts outside [0, M], repeated ids inside a list and across lists, teacher rows without mass."""
import numpy as np
import torch


def stock_fp64(users, rows, ids, count, teacher, scale=1.0, temperature=1.0, grad_loss=None):
    """``(loss [G], lse [G], valid [G] bool, scores [G, M] (NaN where the slot is no element), d_users [G, d], d_rows [P, d], keys)``
    in float64: ``torch.autograd`` through one list at a time.  Written without ``evaluate``'s helpers: a Python loop over the slots
    decides what is an element and what has mass; ``keys`` is ``sorted()`` over Python integers."""
    U = torch.tensor(np.asarray(users, dtype=np.float64), requires_grad=True)
    R = torch.tensor(np.asarray(rows, dtype=np.float64), requires_grad=True)
    G, M, P = len(ids), len(ids[0]), R.shape[0]
    gl = np.ones(G) if grad_loss is None else np.asarray(grad_loss, dtype=np.float64)
    loss, lse, valid = np.zeros(G), np.full(G, -np.inf), np.zeros(G, dtype=bool)
    scores = np.full((G, M), np.nan)
    terms, keys = [], []
    for g in range(G):
        n = M if count is None else min(max(int(count[g]), 0), M)
        slots = [j for j in range(n) if 0 <= int(ids[g][j]) < P]
        keys += [int(ids[g][j]) * (G * M) + g * M + j for j in slots]
        if not slots:
            continue
        x = float(scale) * (R[[int(ids[g][j]) for j in slots]] @ U[g])
        scores[g, slots] = x.detach().numpy() / float(scale)
        lse[g] = float(torch.logsumexp(x.detach(), dim=0))
        mass = [i for i, j in enumerate(slots) if np.isfinite(teacher[g][j])]
        if not mass:
            continue
        tau = torch.tensor([float(teacher[g][slots[i]]) / float(temperature) for i in mass], dtype=torch.float64)
        logq = tau - torch.logsumexp(tau, dim=0)
        logp = x[mass] - torch.logsumexp(x, dim=0)
        kl = (logq.exp() * (logq - logp)).sum()
        valid[g], loss[g] = True, float(kl.detach())
        terms.append(gl[g] * kl)
    if terms:
        torch.stack(terms).sum().backward()
    dU = U.grad.numpy() if U.grad is not None else np.zeros(tuple(U.shape))
    dR = R.grad.numpy() if R.grad is not None else np.zeros(tuple(R.shape))
    return loss, lse, valid, scores, dU, dR, np.array(sorted(keys), dtype=np.int64)


def case(rng, G, M, d, P=None, bad=0.1):
    """``(users [G,d] f32, rows [P,d] f32, ids [G,M] int64, count [G] int32, teacher [G,M] f32)``: a compact table smaller than G M, so
    that ids repeat across lists and inside them; about ``bad`` of the ids outside [0, P) on either side; counts that include 0, M,
    a negative one and one above M when G leaves room; teacher rows that are all -inf, one-hot, or hold a NaN and a +inf."""
    P = max(3, (G * M) // 3 + 1) if P is None else P
    users = (rng.standard_normal((G, d)) * 1.5 / np.sqrt(d)).astype(np.float32)
    rows = rng.standard_normal((P, d)).astype(np.float32)
    ids = rng.integers(0, P, size=(G, M)).astype(np.int64)
    out = rng.random((G, M)) < bad
    n_out = int(out.sum())
    ids[out] = np.where(np.arange(n_out) % 2 == 0, -1 - rng.integers(0, 5, size=n_out), P + rng.integers(0, 5, size=n_out))      # both sides, in turn
    if M >= 2:
        ids[:, 1] = np.where(ids[:, 1] < 0, ids[:, 1], ids[:, 0])  # a repeated id inside (nearly) every list
    count = rng.integers(0, M + 1, size=G).astype(np.int32)
    special = [M, 0, -3, M + 7, 1]
    for g, c in zip(range(G - 1, -1, -1), special):                # from the back: the first lists keep random counts
        count[g] = c
    if G == 1:
        count[0] = M
    teacher = (2.0 * rng.standard_normal((G, M))).astype(np.float32)
    if G >= 7:
        teacher[0, :] = -np.inf                                    # no mass at all
        teacher[1, :] = -np.inf
        teacher[1, min(M - 1, 2)] = 0.0                            # one-hot (possibly at a slot that is no element)
        teacher[2, 0], teacher[2, M - 1] = np.nan, np.inf
        count[:3] = M
    return users, rows, ids, count, teacher


def cancelled(grad_loss, scale, other):
    """The size of the two sums whose difference a gradient that is identically zero is: ``|grad_loss| scale max|other|``."""
    return float(np.abs(grad_loss).max() * abs(scale) * np.abs(other).max())
