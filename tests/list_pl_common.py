"""Shared by tests/test_list_pl_cpu.py and tests/test_hip_list_pl.py: cases for the differentiable Plackett-Luce slate likelihood —
``list_softmax_common.case`` (ids outside the table, counts 0 / negative / above M, a repeated id in nearly every list) with, where
asked, non-finite scores planted through FINITE rows (an overflowing product: +inf, -inf, and inf - inf = NaN), slates that end early
in every way the cut rule names, and weights of both signs and zero — and the stock likelihood of one slate at a time in float64
under ``torch.autograd``, written without ``evaluate``'s helpers."""
import functools

import numpy as np
import torch

import list_softmax_common as LC
import nrms_common as NC

SLATE_KINDS = ("full", "minus_one", "repeat", "dead", "outside", "empty")
BIG = np.float32(3.0e38)
STEP_FIXTURE = "nrms_train_tiny.npz"      # tests/test_hip_list_softmax.py's


def elements(ids, count, rows_num):
    G, M = ids.shape
    cnt = np.full(G, M) if count is None else np.clip(count, 0, M)
    return (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < rows_num)


def slates(rng, ids, count, rows_num, k, S, shift=0, dead_rows=()):
    """``(picks [G, S, k] int32, kind [G, S])``: slate (g, s) is of the kind ``SLATE_KINDS[(g + s + shift) % 6]`` — distinct element
    positions all the way (-1 once the list runs out); the same with a -1 in the middle and valid entries behind it; with a repeat of
    its first entry in the middle; with a slot that is not live (no element, or an element naming one of ``dead_rows``) in the middle;
    with a position outside [0, M) in the middle; and a slate whose FIRST entry is -1."""
    G, M = ids.shape
    elem = elements(ids, count, rows_num)
    elem = elem & ~np.isin(ids, np.asarray(dead_rows, dtype=np.int64))
    picks = np.full((G, S, k), -1, dtype=np.int32)
    kind = (np.arange(G)[:, None] + np.arange(S)[None, :] + shift) % len(SLATE_KINDS)
    for g in range(G):
        at = np.flatnonzero(elem[g])
        dead = np.flatnonzero(~elem[g])
        for s in range(S):
            order = rng.permutation(at)[:k]
            picks[g, s, :len(order)] = order
            mid = min(k - 1, max(1, len(order) // 2)) if k > 1 else 0
            what = SLATE_KINDS[kind[g, s]]
            if what == "minus_one":
                picks[g, s, mid] = -1
            elif what == "repeat" and k > 1:
                picks[g, s, mid] = picks[g, s, 0]
            elif what == "dead":
                picks[g, s, mid] = dead[int(rng.integers(len(dead)))] if len(dead) else -1
            elif what == "outside":
                picks[g, s, mid] = M + 5 if (g + s) % 2 else -7
            elif what == "empty":
                picks[g, s, 0] = -1
    return picks, kind


def weights(rng, G, S):
    """[G, S] float64: both signs, and about a sixth exactly zero."""
    w = rng.standard_normal((G, S))
    w[rng.random((G, S)) < 1.0 / 6.0] = 0.0
    return w


def case(rng, G, M, d, k, S, shift=0, plant=True, **kw):
    """``(users, rows, ids, count, picks, weight, kind)``.  With ``plant`` the first channels of every user are 2 and three rows of the
    table hold +-3e38 there, so their products overflow: row 0 scores +inf, row 1 -inf and, from d = 2 on, row 2 NaN, for every user —
    elements that are not live, through finite rows.  Slot 2 of list g names row g mod 3 where the list is long enough."""
    users, rows, ids, count, _ = LC.case(rng, G, M, d, **kw)
    P = len(rows)
    if plant:
        users[:, :min(d, 2)] = 2.0
        rows[0, 0], rows[1, 0] = BIG, -BIG
        if d >= 2:
            rows[2, 0], rows[2, 1] = BIG, -BIG
        if M >= 3:
            for g in range(G):
                ids[g, 2] = g % (3 if d >= 2 else 2)
    picks, kind = slates(rng, ids, count, P, k, S, shift, dead_rows=(0, 1, 2) if plant else ())
    return users, rows, ids, count, picks, weights(rng, G, S), kind


def stock_fp64(scores, live, picks, inv_t, grad_logp=None):
    """``(logp [G, S], d logp . grad_logp / d scores [G, M])`` in float64 by ``torch.autograd``, one slate at a time: the slate is cut by
    a Python loop, step t is ``a[pick] - logsumexp(a over what is left)``.  No clamp: for spreads far below 700."""
    G, M = scores.shape
    S = picks.shape[1]
    x = torch.tensor(np.where(live, scores, 0.0).astype(np.float64), requires_grad=True)
    gl = np.ones((G, S)) if grad_logp is None else np.asarray(grad_logp, dtype=np.float64)
    logp = np.zeros((G, S))
    total = x.sum() * 0.0
    for g in range(G):
        for s in range(S):
            left = [j for j in range(M) if live[g, j]]
            lp = x.sum() * 0.0
            for p in picks[g, s]:
                p = int(p)
                if p not in left:
                    break
                lp = lp + x[g, p] * inv_t - torch.logsumexp(x[g, left] * inv_t, dim=0)
                left.remove(p)
            logp[g, s] = float(lp.detach())
            total = total + gl[g, s] * lp
    total.backward()
    return logp, x.grad.numpy()


def train_set(device="cpu"):
    """The tiny training fixture as the corpus-like object the list steps read, the first candidate of every impression clicked."""
    dev = NC.dev_set(STEP_FIXTURE, device)
    U, K = NC.case(STEP_FIXTURE)[2]["candidate_ids"].shape
    dev.row_label = (np.arange(U * K) % K == 0).astype(np.int64)
    return dev, U


@functools.lru_cache(maxsize=None)
def policy_lists():
    """Per user a list of 6 news (the tiny corpus has 6), a count below M, ids outside the corpus, click gains; per user 3 slates of
    3 news: one of the list's own, one with a news that is not in the list in the middle, one that starts with -1; weights of both
    signs and a zero."""
    dev, U = train_set()
    N = int(dev.title_text.shape[0])
    rng = np.random.default_rng(23)
    M = N - 1
    ids = np.stack([rng.permutation(np.arange(1, N)) for _ in range(U)]).astype(np.int64)
    count = np.full(U, M, dtype=np.int32)
    count[1] = M - 1
    ids[0, 4], ids[2, 0] = N + 2, -1
    gain = np.zeros((U, M), dtype=np.float32)
    gain[np.arange(U), rng.integers(0, M - 2, size=U)] = 1.0
    slates = np.full((U, 3, 3), -1, dtype=np.int64)
    for g in range(U):
        slates[g, 0] = ids[g, [3, 1, 2]]
        slates[g, 1] = [ids[g, 2], N + 9, ids[g, 3]]
        slates[g, 2, 1:] = ids[g, [1, 2]]
    weight = rng.standard_normal((U, 3))
    weight[0, 0] = 0.0
    return np.arange(U), ids, gain, count, slates, weight
