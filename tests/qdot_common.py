"""Shared by tests/test_qdot_cpu.py and tests/test_hip_qdot.py: the inputs of the quantised first stage — random vectors, the special
rows of the quantiser, integer data whose codes are known in advance — and the containment test of the two-stage contract."""
import functools

import numpy as np

NEW = ("digat_quantize_rows_i8", "digat_qdot_scores", "digat_qdot_topk_workspace_bytes", "digat_qdot_topk",
       "digat_qdot_shortlist_workspace_bytes", "digat_qdot_shortlist")
OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3


def width(d):
    return (d + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def normal(G, N, d, seed=0):
    """``default_rng(seed).standard_normal`` users [G, d] and news [N, d], float32 (read-only: shared between tests)."""
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal((G, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def coded(G, N, d, seed=0):
    """``normal`` with its host codes: ``(users, news, qu, su, qn, sn)``."""
    from digat_amd import evaluate
    u, v = normal(G, N, d, seed)
    return (u, v) + evaluate.quantize_rows_host(u) + evaluate.quantize_rows_host(v)


def special_rows(d, seed=5):
    """Rows the quantiser treats one by one: random, zero, a NaN, +inf, -inf, a single non-zero entry, a subnormal row (amax / 127
    underflows to a subnormal or to zero), huge magnitudes, and a row of halves of the step (ties of rint)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((10, d)).astype(np.float32)
    x[1] = 0
    x[2, d // 2] = np.nan
    x[3, 0] = np.inf
    x[4, d - 1] = -np.inf
    x[5] = 0
    x[5, d // 3] = -2.5
    x[6] = np.float32(1e-44) * rng.integers(-3, 4, size=d)
    x[7] *= np.float32(1e37)
    x[8] = (rng.integers(-254, 255, size=d) * 0.5).astype(np.float32)        # with amax 127: every odd entry is a tie
    x[8, 0] = 127.0
    return x


def oriented(G, P, d):
    """Integer data whose codes and scores are known without a quantiser: news[p][c] = (p + 3 c) mod 7 - 3 with +-127 in the last
    channel (amax 127: scale exactly 1, codes = values), users one-hot with magnitude g + 1 in channel (5 g + 1) mod (d - 1) (code
    127, scale (g + 1) / 127).  Returns ``(users, news, acc int64 [G, P])`` with ``acc`` the integer product of the codes; nothing in
    it is symmetric in (g, p) or in c."""
    assert d >= 3
    p, c = np.arange(P)[:, None], np.arange(d)[None, :]
    news = ((p + 3 * c) % 7 - 3).astype(np.float32)
    news[:, d - 1] = np.where(np.arange(P) % 2 == 0, 127.0, -127.0)
    users = np.zeros((G, d), dtype=np.float32)
    chan = (5 * np.arange(G) + 1) % (d - 1)
    users[np.arange(G), chan] = np.arange(G) + 1.0
    acc = 127 * news[:, chan].T.astype(np.int64)
    return users, news, acc


def tied(G, N, d, seed=7):
    """Low-magnitude integer vectors, entries -1, 0, 1 with a 1 in front: codes -127, 0, 127 and one scale for all rows, so a user
    has at most 2 d + 1 different quantised scores: long runs of equal ones."""
    rng = np.random.default_rng(seed)
    u = rng.integers(-1, 2, size=(G, d)).astype(np.float32)
    v = rng.integers(-1, 2, size=(N, d)).astype(np.float32)
    u[:, 0], v[:, 0] = 1.0, 1.0
    return u, v


def contained(exact_ids, exact_count, short_ids, short_count):
    """bool [G]: every one of the user's first ``exact_count`` exact ids stands among its first ``short_count`` shortlist ids."""
    out = np.zeros(len(exact_ids), dtype=bool)
    for g in range(len(exact_ids)):
        out[g] = set(exact_ids[g, :exact_count[g]].tolist()) <= set(short_ids[g, :short_count[g]].tolist())
    return out
