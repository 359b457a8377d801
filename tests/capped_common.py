"""What the two suites of exposure-capped top-k share (tests/test_capped_cpu.py, tests/test_hip_capped.py): one generator of
batches of lists, one table of cases, the reference of every case — the host contract ``evaluate.capped_select_host``, computed
once per case and cap and handed out read-only — and the exact comparison.

The lists: per list min(M, P) distinct news drawn with a strong popularity head (so many lists contend for few news), padded with
id -1 where the pool is smaller than the list; scores with a popularity bias, rounded to quarters, so exact ties abound; a ragged
``count`` with an empty list; news 1 in slot 0 of every list and twice in list 0 (a repeated id: with list 1 empty its segment has
G pairs), news 2 in slot 1 (G - 1 pairs at most); some ``-inf``, ``+inf`` and NaN scores and some ids outside [0, P)."""
import functools

import numpy as np

# (G, M, k, P): segments of 65 / 299 / 300 pairs across the wave and workgroup boundaries, lists on both kernel shapes and on
# M = 64 / 65 / 129, starved calls (supply below demand) and nearly unconstrained ones
CASES = [(1, 1, 1, 3), (3, 63, 10, 40), (65, 64, 10, 50), (65, 65, 1, 30), (300, 64, 10, 200), (300, 129, 128, 400), (33, 257, 10, 300),
         (300, 1024, 10, 1100), (65, 1024, 128, 1500)]
CAPS = (1, 2, 7, "array")          # "array": a per-news capacity of 0 / 1 / 2
ROUND_LIMIT = 64                   # every case reaches its fixed point within this many rounds (asserted below)


def seed_of(G, M, k, P):
    return G * 1000003 + M * 1009 + k * 31 + P


def make_lists(seed, G, M, P, priority=False):
    """``(ids [G,M] int64, scores [G,M] float32, count [G] int32, priority [G,M] float32 or None)``."""
    rng = np.random.default_rng(seed)
    n = min(M, P)
    weight = -1.5 * np.log(np.arange(P) + 1.0)                                   # the popularity head: news 0 first
    draw = np.argsort(-(weight[None, :] + rng.gumbel(size=(G, P))), axis=1)[:, :n]          # n distinct news per list
    ids = np.full((G, M), -1, dtype=np.int64)
    ids[:, :n] = np.take_along_axis(draw, np.argsort(rng.random((G, n)), axis=1), axis=1)   # in no particular slot order
    bias = np.where(ids >= 0, weight[np.clip(ids, 0, P - 1)], 0.0)
    scores = (np.round((0.7 * bias + rng.standard_normal((G, M))) * 4) / 4).astype(np.float32)
    count = rng.integers(max(1, n // 2), M + 1, size=G).astype(np.int32)
    count[rng.random(G) < 0.3] = M
    if P > 2 and M >= 2:
        for slot, news in ((0, 1), (1, 2)):                                      # two news that (nearly) every list names
            there = ids == news
            ids[there] = ids[:, slot:slot + 1].repeat(M, axis=1)[there]
            ids[:, slot] = news
        ids[0, 1] = 1                                                            # list 0 names news 1 twice: two pairs
        count[0] = max(int(count[0]), 2)
    if G > 1:
        count[1] = 0                                                             # an empty list
    if G > 2:
        count[2] = M + 3                                                         # clipped to M
    odd = rng.random((G, M))
    scores[odd < 0.02] = -np.inf
    scores[(odd >= 0.02) & (odd < 0.03)] = np.nan
    ids[(odd >= 0.03) & (odd < 0.04)] = P + 5
    ids[(odd >= 0.04) & (odd < 0.05)] = P
    ids[(odd >= 0.05) & (odd < 0.055)] = -7
    scores[(odd >= 0.055) & (odd < 0.06)] = np.inf                               # an element, the best of its list
    pr = None
    if priority:
        pr = (np.round(rng.standard_normal((G, M)) * 2) / 2).astype(np.float32)
        pr[rng.random((G, M)) < 0.01] = np.nan                                   # no element
        pr[rng.random((G, M)) < 0.01] = -np.inf                                  # an element, the last its item takes
    return ids, scores, count, pr


def make_cap(seed, cap, P):
    if cap == "array":
        return np.random.default_rng(seed + 17).integers(0, 3, size=P).astype(np.int32)
    return int(cap)


@functools.lru_cache(maxsize=None)
def case(G, M, k, P, cap, priority=False):
    """``(inputs, cap, reference)`` of a case, built once: ``inputs = (ids, scores, count, priority)``, ``reference`` the host
    contract's ``(ids, scores, count, slots, rounds)``.  All arrays are read-only."""
    from digat_amd import evaluate
    seed = seed_of(G, M, k, P)
    inputs = make_lists(seed, G, M, P, priority)
    capv = make_cap(seed, cap, P)
    want = evaluate.capped_select_host(inputs[0], inputs[1], inputs[2], k, capv, P, priority=inputs[3], max_rounds=ROUND_LIMIT)
    assert want[4] <= ROUND_LIMIT
    for a in inputs + want[:4] + (capv,):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inputs, capv, want


def bits(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def same(got, want, what=""):
    """ids, score BITS, count, slots and rounds of ``got`` (tensors or arrays) are ``want``'s."""
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    for name, g, w in zip(("ids", "scores", "count", "slots"), got[:4], want[:4]):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8].tolist())
    assert int(got[4]) == int(want[4]), (what, "rounds", got[4], want[4])
