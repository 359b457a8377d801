"""Shared by tests/test_pl_sample_cpu.py and tests/test_hip_pl_sample.py: the lists of every GPU case from one generator and one table
of seeds (the CPU suite holds every one of them to be robust — ``pl_sample_host(return_robust=True)`` — so that the GPU suite may
compare picks exactly) and the comparison of a device result with the twin's: picks and lengths exactly, ``logp`` and ``step_logp``
inside ``evaluate.pl_bound``."""
import numpy as np

G = 16
MS = (1, 63, 64, 65, 129, 257, 1024)       # wave and workgroup edges, a sort that is no power of two, the full list
KS = (1, 10, 128)
SS = (1, 3)
TS = (0.05, 1.0, 8.0)
# the seed of every (M, T): the first one from 0 on whose 16 lists are robust at k = 128 and 3 samples — which covers every smaller k
# (a prefix of the same keys) and S = 1 (sample 0 of the same call) — 0 unless named here (first_robust_seed)
SEEDS = {}


def seed_of(M, T):
    return SEEDS.get((M, T), 0)


def make_case(seed, M, groups=G):
    """``(scores [G, M] float32, count [G] int32, streams [G] int64)``.  Scores N(0, scale^2) with the scale of list g cycling through
    1, 3, 30 (at T = 0.05 a spread far above 700 T: the clamp) and list 5 all equal (scale 0); counts ragged, with M (list 0), 0
    (list 1), M + 5 (list 2), 3 at most (list 4: fewer live entries than k) and a negative one (list 7) among them; list 3 holds a
    NaN, a +inf and a -inf and list 8 nothing but -inf; the streams are scattered 32-bit ids, 2^32 - 1 among them."""
    rng = np.random.default_rng([seed, M])
    scale = np.array([1.0, 3.0, 30.0])[np.arange(groups) % 3]
    scores = (rng.standard_normal((groups, M)) * scale[:, None]).astype(np.float32)
    count = rng.integers(1, M + 1, size=groups).astype(np.int32)
    streams = rng.integers(0, 1 << 32, size=groups, dtype=np.int64)
    streams[0] = (1 << 32) - 1
    fixed = {0: M, 1: 0, 2: M + 5, 3: M, 4: min(M, 3), 7: -2}
    for g, c in fixed.items():
        if g < groups:
            count[g] = c
    if groups > 3 and M >= 8:
        scores[3, [1, M // 2, M - 1]] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    if groups > 5:
        scores[5] = np.float32(0.25)
    if groups > 8:
        scores[8] = -np.inf
    return scores, count, streams


def extra_cases():
    """The GPU cases beyond the (M, k, S, T) grid, by name: ``(scores, count, streams, k, T, seed)``.  ``clamp``: scores N(0, 400^2)
    at T = 1, a spread far above 700 T, so most weights sit on the clamp; ``many``: 1100 short lists, more workgroups than compute
    units."""
    rng = np.random.default_rng(77)
    clamp = (rng.standard_normal((4, 70)) * 400.0).astype(np.float32)
    many, many_count, many_streams = make_case(3, 16, groups=1100)
    return {"clamp": (clamp, np.array([70, 70, 33, 70], dtype=np.int32), np.arange(4, dtype=np.int64) + 1000, 70, 1.0, 5),
            "many": (many, many_count, many_streams, 10, 1.0, 3)}


def first_robust_seed(M, T, limit=40):
    """How SEEDS was chosen: the first seed whose lists are all robust."""
    from digat_amd import evaluate
    for seed in range(limit):
        scores, count, streams = make_case(seed, M)
        if evaluate.pl_sample_host(scores, count, 128, T, seed=seed, samples=3, streams=streams, return_robust=True)[4].all():
            return seed
    raise AssertionError(f"no robust seed below {limit} for {(M, T)}")


def host(t):
    return np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t)


def within_bound(got_logp, got_step, want_logp, want_step, parts, what=""):
    """``logp`` [G, S] float64 and ``step_logp`` [G, S, k] float32 against the twin's inside ``evaluate.pl_bound`` (``parts``: the
    twin's dict).  Returns the worst error-to-bound ratio."""
    from digat_amd import evaluate
    gl, gs = host(got_logp), host(got_step)
    assert gl.dtype == np.float64 and gs.dtype == np.float32 and gl.shape == want_logp.shape and gs.shape == want_step.shape, what
    n = parts["live"][:, None, None]
    b_step = evaluate.pl_bound(n, parts["logZ"], parts["step"], float32=True)
    b_logp = evaluate.pl_bound(n, parts["logZ"], parts["step"], total=True)
    e_step = np.abs(gs.astype(np.float64) - want_step.astype(np.float64))
    e_logp = np.abs(gl - want_logp)
    assert np.isfinite(gl).all() and np.isfinite(gs).all(), what
    bad = np.argwhere(~(e_step <= b_step))
    assert bad.size == 0, (what, "step_logp", bad[:4].tolist(), e_step[tuple(bad[0])], b_step[tuple(bad[0])])
    bad = np.argwhere(~(e_logp <= b_logp))
    assert bad.size == 0, (what, "logp", bad[:4].tolist(), e_logp[tuple(bad[0])], b_logp[tuple(bad[0])])
    # the ratio that is recorded is the float64 one: logp against its bound (step_logp's is dominated by its float32 rounding)
    return float(np.max(e_logp / b_logp)) if e_logp.size else 0.0


def same(got, want, parts, what=""):
    """``(picks, n_out, logp, step_logp)`` of the device against the twin's: picks and lengths exactly, the probabilities inside
    the bound.  Returns the worst ratio."""
    gp, gn = host(got[0]), host(got[1])
    assert gp.dtype == np.int32 and gn.dtype == np.int32, what
    assert np.array_equal(gn, want[1]), (what, "n_out", gn.tolist(), want[1].tolist())
    bad = np.argwhere(gp != want[0])
    assert gp.shape == want[0].shape and bad.size == 0, (what, "picks", bad[:4].tolist())
    return within_bound(got[2], got[3], want[2], want[3], parts, what)
