"""Shared by tests/test_pl_expect_cpu.py and tests/test_hip_pl_expect.py: the lists, values and slates of every case from one
generator, seeded like tests/pl_sample_common.py, the host twin's answer computed once per case, and the comparison of a device
result with it: ``length``, ``step_value`` and the contractual zeros exactly, ``step_mean`` inside ``evaluate.pl_expect_bound``."""
import functools

import numpy as np

import pl_sample_common as P

G = 5
MS, KS, SS, TS = P.MS, P.KS, P.SS, P.TS
VALUE_FLOOR = 2.0 ** -10        # pl_expect_bound's domain: |v| >= 2^-12 or 0 keeps every product w |v| a normal float64


def make_values(rng, groups, M):
    """``values`` [groups, M] float32: signed N(0, 1) — the weighted mean cancels, ``|mean| << A_t`` — with everything below
    ``VALUE_FLOOR`` set to 0 and a NaN, a +inf and a -inf among them (they count as 0)."""
    v = rng.standard_normal((groups, M)).astype(np.float32)
    v[np.abs(v) < VALUE_FLOOR] = 0.0
    v[0, 0] = np.nan
    v[groups - 1, M // 2] = np.inf
    v[min(2, groups - 1), M - 1] = -np.inf
    return v


def make_picks(rng, live, k, S):
    """``picks`` [G, S, k] int32: a random order of all positions (-1 behind it where M < k), so a list with dead positions is cut
    where the order first meets one; on top of that list 2 (three live entries), slate 0, repeats its first pick at slot 2, list 3
    meets a score that is not finite at slot 1 and list 4, slate 0, holds a -1 at slot k // 2."""
    groups, M = live.shape
    picks = np.full((groups, S, k), -1, dtype=np.int32)
    for g in range(groups):
        for s in range(S):
            order = rng.permutation(M)[:k]
            if g == 0:                                                    # list 0 is full: a slate that is never cut (beyond M)
                pos = np.flatnonzero(live[0])
                order = pos[rng.permutation(len(pos))][:k]
            picks[g, s, :len(order)] = order
    if groups > 2 and k >= 3 and M >= 2:
        picks[2, 0, :3] = (0, 1, 0)
    if groups > 3 and k >= 2:
        dead = np.flatnonzero(~live[3])
        if len(dead):
            picks[3, :, 1] = dead[0]
    if groups > 4:
        picks[4, 0, k // 2] = -1
    return picks


def make_case(M, k, S, groups=G, seed=0):
    """``(scores [G, M] float32, count [G] int32, values [G, M] float32, picks [G, S, k] int32)``.  Scores N(0, scale^2) with the
    scale of list g cycling through 1, 3, 30 (list 0 in pairs that cancel); counts: M (list 0), 0 (list 1), min(M, 3) (list 2), M (list 3, which holds a NaN, a
    +inf and a -inf where M >= 8), ragged beyond."""
    rng = np.random.default_rng([seed, M, k, S, groups])
    scale = np.array([1.0, 3.0, 30.0])[np.arange(groups) % 3]
    scores = (rng.standard_normal((groups, M)) * scale[:, None]).astype(np.float32)
    count = rng.integers(1, M + 1, size=groups).astype(np.int32)
    for g, c in {0: M, 1: 0, 2: min(M, 3), 3: M}.items():
        if g < groups:
            count[g] = c
    if groups > 3 and M >= 8:
        scores[3, [1, M // 2, M - 1]] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    live = (np.arange(M)[None, :] < np.clip(count, 0, M)[:, None]) & np.isfinite(scores)
    values = make_values(rng, groups, M)
    even = M // 2 * 2                       # list 0 in pairs of equal scores and nearly opposite values: at step 0 |mean| is ~2^-11 A_t
    scores[0, 1:even:2] = scores[0, 0:even:2]
    values[0, 1:even:2] = -values[0, 0:even:2] * np.float32(1 + 2.0 ** -10)
    return scores, count, values, make_picks(rng, live, k, S)


@functools.lru_cache(maxsize=None)
def case_and_twin(M, k, S, T, groups=G):
    """The case of (M, k, S) and ``evaluate.pl_expect_host(..., parts=True)`` on it at temperature T: computed once, never changed."""
    from digat_amd import evaluate
    case = make_case(M, k, S, groups)
    want = evaluate.pl_expect_host(case[0], case[1], case[3], case[2], T, parts=True)
    for x in case + want[:5] + tuple(want[5].values()):
        x.setflags(write=False)
    return case, want


def clamp_case(S=3):
    """``pl_sample_common``'s clamp lists (a spread far above 700 T at T = 1) with values and random slates of all 70 positions."""
    scores, count, _, k, T, _ = P.extra_cases()["clamp"]
    rng = np.random.default_rng(78)
    live = (np.arange(scores.shape[1])[None, :] < count[:, None]) & np.isfinite(scores)
    return scores, count, make_values(rng, scores.shape[0], scores.shape[1]), make_picks(rng, live, k, S), T


def host(t):
    return np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t)


def bits(x):
    return np.ascontiguousarray(host(x)).reshape(-1).view(np.uint8)


def same(got, want, what=""):
    """``(logp, step_logp, step_mean, step_value, length)`` of the device against the twin's ``want`` (with its parts): ``length``,
    ``step_value``'s bits and the zeros at and beyond ``length`` exactly, ``step_mean`` inside ``pl_expect_bound``.  Returns the
    worst error-to-bound ratio of ``step_mean``."""
    from digat_amd import evaluate
    mean, used, length = host(got[2]), host(got[3]), host(got[4])
    parts = want[5]
    assert mean.dtype == np.float64 and used.dtype == np.float32 and length.dtype == np.int32, what
    assert mean.shape == want[2].shape and used.shape == want[3].shape and length.shape == want[4].shape, what
    assert np.array_equal(length, want[4]), (what, "length", length.tolist(), want[4].tolist())
    assert np.array_equal(used.view(np.uint32), want[3].view(np.uint32)), (what, "step_value")
    beyond = np.arange(mean.shape[2])[None, None, :] >= length[:, :, None]
    assert not mean[beyond].any() and not used[beyond].any() and not host(got[1])[beyond].any(), (what, "zeros beyond length")
    assert np.isfinite(mean).all(), what
    bound = evaluate.pl_expect_bound(parts["live"][:, None, None], parts["absolute"], want[2])
    err = np.abs(mean - want[2])
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (what, "step_mean", bad[:4].tolist(), err[tuple(bad[0])], bound[tuple(bad[0])])
    inside = ~beyond & (bound > 0)
    return float(np.max(err[inside] / bound[inside])) if inside.any() else 0.0
