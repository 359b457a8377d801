"""Shared by tests/test_list_pairwise_cpu.py and tests/test_hip_list_pairwise.py: the pairwise nDCG loss of one list at a time in
float64 under ``torch.autograd``, written without ``evaluate``'s helpers — ranks from a Python ``sorted`` with the tie rule, detached
weights, ``logaddexp`` for the logistic loss —, and cases built on ``list_softmax_common.case`` with the gains a kernel can get wrong."""
import math

import numpy as np
import torch

import list_softmax_common as LC

KINDS = ("clicks", "grades", "distinct", "zero", "single", "unlabelled")


def stock_fp64(scores, ids, count, gain, rows_num, scale, discount):
    """``(loss [G], ndcg [G], valid [G] bool, lambda [G, M])`` in float64 on given fp32 ``scores`` [G, M]: ``torch.autograd`` through
    one list at a time, the leaf being ``x = fl32(scale * score)``, so that ``lambda = scale * d loss / d x``.  ``ids`` None: a slot
    below ``count`` is an element when its score is no NaN."""
    G, M = len(scores), len(scores[0])
    loss, ndcg, valid, lam = np.zeros(G), np.zeros(G), np.zeros(G, dtype=bool), np.zeros((G, M))
    sc32 = np.float32(scale)
    for g in range(G):
        n_slots = M if count is None else min(max(int(count[g]), 0), M)
        slots, xs, gs = [], [], []
        for j in range(n_slots):
            if ids is None:
                if math.isnan(float(scores[g][j])):
                    continue
            elif not 0 <= int(ids[g][j]) < rows_num:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                x = float(sc32 * np.float32(scores[g][j]))
            gn = float(gain[g][j])
            if math.isnan(x) or not math.isfinite(gn) or gn < 0:
                continue
            slots.append(j)
            xs.append(x)
            gs.append(gn)
        n = len(slots)
        r, t = [0] * n, [0] * n
        for rank, a in enumerate(sorted(range(n), key=lambda a: (-xs[a], slots[a]))):
            r[a] = rank
        for rank, a in enumerate(sorted(range(n), key=lambda a: (-gs[a], slots[a]))):
            t[a] = rank
        idcg = math.fsum(gs[a] * float(discount[t[a]]) for a in range(n))
        if not idcg > 0:
            continue
        valid[g] = True
        ndcg[g] = math.fsum(gs[a] * float(discount[r[a]]) for a in range(n)) / idcg
        ia, ib, w = [], [], []
        for a in range(n):
            for b in range(n):
                if gs[a] > gs[b]:
                    ia.append(a)
                    ib.append(b)
                    w.append((gs[a] - gs[b]) * abs(float(discount[r[a]]) - float(discount[r[b]])) / idcg)
        if not ia:
            continue
        xt = torch.tensor(xs, dtype=torch.float64, requires_grad=True)
        tt = xt[ia] - xt[ib]
        total = (torch.tensor(w, dtype=torch.float64) * torch.logaddexp(torch.zeros_like(tt), -tt)).sum()
        total.backward()
        loss[g] = float(total.detach())
        lam[g, slots] = float(sc32) * xt.grad.numpy()
    return loss, ndcg, valid, lam


def elements(ids, count, rows_num):
    G, M = ids.shape
    cnt = np.full(G, M) if count is None else np.clip(count, 0, M)
    return (np.arange(M)[None, :] < cnt[:, None]) & (ids >= 0) & (ids < rows_num)


def gains(rng, ids, count, rows_num, shift=0):
    """``(gain [G, M] f32, kind [G])``: list g gets the kind ``KINDS[(g + shift) % 6]`` — clicks (one to three ones on elements, the
    rest zero), grades 0..3 with many equal values, all distinct, all zero (invalid), one labelled element with a positive gain
    (valid, no pair), grades with a NaN, a -inf, a +inf and a negative value among them."""
    G, M = ids.shape
    elem = elements(ids, count, rows_num)
    gain = np.zeros((G, M), dtype=np.float32)
    kind = (np.arange(G) + shift) % len(KINDS)
    for g in range(G):
        at = np.flatnonzero(elem[g])
        k = KINDS[kind[g]]
        if k == "clicks":
            where = at if len(at) else np.arange(M)
            gain[g, rng.choice(where, size=min(len(where), int(rng.integers(1, 4))), replace=False)] = 1.0
        elif k in ("grades", "unlabelled"):
            gain[g] = rng.integers(0, 4, size=M)
            if k == "unlabelled":
                for slot, v in zip((2, 3, 4, 5), (np.nan, -np.inf, np.inf, -1.5)):
                    gain[g, slot % M] = v
        elif k == "distinct":
            gain[g] = rng.permutation(M) * 0.25
        elif k == "single":
            gain[g] = np.nan
            gain[g, at[len(at) // 2] if len(at) else 0] = 2.0
    return gain, kind


def live(gain, ids, count, rows_num):
    """bool [G]: the list is valid and has a pair of labelled elements with different gains."""
    elem = elements(ids, count, rows_num)
    with np.errstate(invalid="ignore"):
        lab = elem & np.isfinite(gain) & (gain >= 0)
    out = np.zeros(len(gain), dtype=bool)
    for g in range(len(gain)):
        v = gain[g][lab[g]]
        out[g] = len(v) > 0 and v.max() > 0 and v.max() > v.min()
    return out


def case(rng, G, M, d, shift=0, **kw):
    """``(users, rows, ids, count, gain, kind)``: ``list_softmax_common.case`` — ids outside the table on both sides, counts 0, M,
    negative and above M, a repeated id in slots 0 / 1 of nearly every list (EQUAL score bits: the slot-order tie rule) — with
    ``gains``.  Checked here, on the inputs: with G >= 7 lists of at least 8 slots, at least half are valid with a live pair."""
    users, rows, ids, count, _ = LC.case(rng, G, M, d, **kw)
    gain, kind = gains(rng, ids, count, len(rows), shift)
    if G >= 7 and M >= 8:
        assert 2 * int(live(gain, ids, count, len(rows)).sum()) >= G, "the generator: half of the lists have a live pair"
    return users, rows, ids, count, gain, kind
