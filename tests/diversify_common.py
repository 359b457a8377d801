"""Shared by tests/test_diversify_cpu.py and tests/test_hip_diversify.py: short lists with everything a list may hold (ragged
counts, ids outside the table, repeated ids), a brute-force maximal-marginal-relevance selection in plain Python, and the
comparison of a result triple with an expected one."""
import math

import numpy as np


def make_lists(rng, G, M, N, ragged=True, invalid=True, repeats=True):
    """``(ids [G, M] int64, count [G] int32)``: ids in [0, N), some -1 / N / N + 5 inside the count, some repeated; counts ragged
    with 0 and M among them when G allows."""
    ids = rng.integers(0, max(N, 1), size=(G, M)).astype(np.int64)
    if repeats and M > 1:
        for g in range(G):
            a, b = rng.integers(0, M, size=2)
            ids[g, a] = ids[g, b]
    if invalid:
        hole = rng.random((G, M)) < 0.1
        ids[hole] = rng.choice(np.array([-1, N, N + 5, -7], dtype=np.int64), size=int(hole.sum()))
    count = np.full(G, M, dtype=np.int32)
    if ragged:
        count = rng.integers(0, M + 1, size=G).astype(np.int32)
        count[0] = M
        if G > 1:
            count[1] = 0
        if G > 2:
            count[2] = max(M - 1, 0)
    return ids, count


def brute_force(ids, scores, count, sim, k, lam, N, category=None, q=0):
    """One user, plain Python: greedy picks over tuples ``(NaN last, value descending, position ascending)``.  ``sim[i][j]`` is
    read as given.  Returns ``[(position, id)]``."""
    M = len(ids)
    c = M if count is None else max(0, min(M, int(count)))
    elems = [p for p in range(c) if 0 <= int(ids[p]) < N]
    pen = {p: 0.0 for p in elems}
    picked = []
    mu = 1.0 - lam
    for _ in range(k):
        cand = []
        for p in elems:
            if p in picked:
                continue
            if q > 0 and sum(1 for e in picked if category[int(ids[e])] == category[int(ids[p])]) >= q:
                continue
            value = lam * float(scores[p]) - mu * pen[p]
            cand.append((1, 0.0, p) if math.isnan(value) else (0, -value, p))
        if not cand:
            break
        j = sorted(cand)[0][2]
        picked.append(j)
        for p in elems:
            x = float(sim[p][j])
            if not math.isnan(x):
                pen[p] = max(pen[p], x)
    return [(p, int(ids[p])) for p in picked]


def bits(x):
    return np.ascontiguousarray(np.asarray(x), dtype=np.float32).view(np.uint32)


def same(got, want, what=""):
    """Two ``(scores [G,k], ids [G,k], count [G])`` triples: counts, ids and score bits, fills included."""
    gs, gi, gc = (np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in got)
    ws, wi, wc = (np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in want)
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gc.dtype == np.int32, what
    assert gs.shape == ws.shape and gi.shape == wi.shape and gc.shape == wc.shape, what
    assert np.array_equal(gc, wc), (what, "count", np.flatnonzero(gc != wc)[:8].tolist())
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ for users", bad[:8].tolist(), gi[bad[0]].tolist(), wi[bad[0]].tolist())
    assert np.array_equal(bits(gs), bits(ws)), (what, "score bits")
