"""Shared by tests/test_calibrate_cpu.py and tests/test_hip_calibrate.py: the lists, categories and targets of every GPU case from one
generator and one table of seeds (the CPU suite holds every one of them to be robust — ``calibrated_select_host(return_robust=True)``
— so that the GPU suite may compare picks exactly), a plain-Python float64 brute force of the literal objective, the bound of the
``kl`` output and the comparison of a result with an expected one."""
import math

import numpy as np

import diversify_common as V

G = 37
NEWS = 3000
LAMS = (0.3, 0.5, 0.7)
SHAPES = ((1, 1, 1), (64, 17, 10), (65, 17, 10), (128, 64, 128), (129, 17, 16), (1000, 17, 100), (1024, 17, 128), (1024, 64, 128))      # (M, C, k)
# the seed of every (M, C, k, lam): the first one from 0 on whose 37 lists are all robust (first_robust_seed) — 0 unless named here.
# Short lists and small k are robust by hundreds of ulps whatever the seed; a long list with k >= 100 meets a near-tie now and then
SEEDS = {(1000, 17, 100, 0.7): 1, (1024, 17, 128, 0.7): 4}
GRID_CASES = ((100, 32, 0), (1000, 64, 0))        # (M, k, seed) of the uniform-target cases: C = 16, target 1/16, scores on a 1/16 grid, lam 0.5


def seed_of(M, C, k, lam):
    return SEEDS.get((M, C, k, lam), 0)


def make_case(seed, M, C, groups=G, N=NEWS, grid=False, uniform=False):
    """``(ids [G,M], scores [G,M], count [G], category [N], target [G,C])``.  Lists: ragged counts with 0 and M among them, ids
    outside [0, N) and repeated ids (``diversify_common.make_lists``); categories -1 .. C + 1, so some lie outside [0, C); scores
    standard normal with a NaN, a +inf and a -inf in list 3 (``grid``: rounded to multiples of 1/16, no negative zero); targets
    Dirichlet rows with a fifth of their entries zeroed, row 4 all zero, row 5 with a NaN, a negative and an infinite entry — all
    three count as 0 (``uniform``: 1 / C everywhere)."""
    rng = np.random.default_rng(seed)
    ids, count = V.make_lists(rng, groups, M, N)
    scores = rng.standard_normal((groups, M)).astype(np.float32)
    if grid:
        scores = (np.round(scores * 16) / 16 + 0.0).astype(np.float32)
    if groups > 3 and M >= 8:
        scores[3, [1, M // 2, M - 1]] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        count[3] = M
    category = rng.integers(-1, C + 2, size=N).astype(np.int32)
    if uniform:
        target = np.full((groups, C), 1.0 / C, dtype=np.float32)
    else:
        target = rng.dirichlet(np.full(C, 0.7), size=groups).astype(np.float32)
        target[rng.random((groups, C)) < 0.2] = 0.0
        if groups > 4:
            target[4] = 0.0
        if groups > 5 and C >= 3:
            target[5, :3] = np.array([np.nan, -0.25, np.inf], dtype=np.float32)
    return ids, scores, count, category, target


def first_robust_seed(M, C, k, lam, alpha=0.01, limit=40, **kw):
    """How SEEDS and GRID_CASES were chosen: the first seed whose lists are all robust."""
    from digat_amd import evaluate
    for seed in range(limit):
        ids, scores, count, category, target = make_case(seed, M, C, **kw)
        if evaluate.calibrated_select_host(ids, scores, count, category, target, k, lam, alpha, return_robust=True)[4].all():
            return seed
    raise AssertionError(f"no robust seed below {limit} for {(M, C, k, lam)}")


def brute_force(ids, scores, count, category, target, k, lam, alpha=0.01):
    """One list, plain Python floats: at every step the unpicked element that maximises the LITERAL objective ``lam sum(s) - mu
    KL(p || q)`` of the list it would make (``q_c = (1 - alpha) n_c / T + alpha p_c``, the sum over ``p_c > 0`` by ``math.fsum``),
    ties to the lowest position, NaNs last.  ``lam`` / ``mu`` are the float32 weights of ``mmr_weights``.  Returns the positions."""
    lam = float(np.float32(lam))
    mu = float(np.float32(1) - np.float32(lam))
    M, N, C = len(ids), len(category), len(target)
    c = M if count is None else max(0, min(M, int(count)))
    elems = [p for p in range(c) if 0 <= int(ids[p]) < N]
    p_c = [float(x) if math.isfinite(float(x)) and float(x) > 0 else 0.0 for x in target]
    cat = {p: int(category[int(ids[p])]) for p in elems}

    def kl(n, T):
        return math.fsum(p_c[j] * (math.log(p_c[j]) - math.log((1.0 - alpha) * n[j] / T + alpha * p_c[j])) for j in range(C) if p_c[j] > 0)
    picked, n, total = [], [0] * C, 0.0
    for t in range(k):
        cand = []
        for p in elems:
            if p in picked:
                continue
            m = list(n)
            if 0 <= cat[p] < C:
                m[cat[p]] += 1
            value = lam * (total + float(scores[p])) - mu * kl(m, t + 1.0)
            cand.append((1, 0.0, p) if math.isnan(value) else (0, -value, p))
        if not cand:
            break
        j = sorted(cand)[0][2]
        picked.append(j)
        total += float(scores[j])
        if 0 <= cat[j] < C:
            n[cat[j]] += 1
    return picked


def kl_bound(out_ids, out_count, category, target, alpha, want_kl):
    """The bound of ``|kl - twin|`` per list: ``2 ulp32(twin) + 64 * 2^-52 * sum_c p_c (|log p_c| + |log q_c|)`` — the rounding of
    one float32 conversion plus a float64 sum in any order — from the finished lists themselves."""
    out_ids, out_count, tgt = np.asarray(out_ids), np.asarray(out_count), np.asarray(target, dtype=np.float32)
    Gn, C = tgt.shape
    bound = np.zeros(Gn, dtype=np.float64)
    for g in range(Gn):
        p = np.where(np.isfinite(tgt[g]) & (tgt[g] > 0), tgt[g], np.float32(0)).astype(np.float64)
        cg = np.asarray(category)[out_ids[g, :int(out_count[g])]]
        n = np.bincount(cg[(cg >= 0) & (cg < C)], minlength=C).astype(np.float64)
        live = p > 0
        q = ((1.0 - alpha) * n[live]) / max(int(out_count[g]), 1) + alpha * p[live]
        bound[g] = 64 * 2.0 ** -52 * float(np.sum(p[live] * (np.abs(np.log(p[live])) + np.abs(np.log(q)))))
    return 2 * np.spacing(np.abs(np.asarray(want_kl, dtype=np.float32))).astype(np.float64) + bound


def same(got, want, category, target, alpha, what=""):
    """``(scores, ids, count, kl)`` against the twin's: counts, ids and score bits exactly (``diversify_common.same``), ``kl``
    inside ``kl_bound``."""
    V.same(got[:3], want[:3], what)
    gk = np.asarray(got[3].cpu()) if hasattr(got[3], "cpu") else np.asarray(got[3])
    wk = np.asarray(want[3])
    assert gk.dtype == np.float32 and gk.shape == wk.shape, what
    err = np.abs(gk.astype(np.float64) - wk.astype(np.float64))
    bound = kl_bound(want[1], want[2], category, target, alpha, wk)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (what, "kl", bad[:8].tolist(), gk[bad[:4]].tolist(), wk[bad[:4]].tolist(), bound[bad[:4]].tolist())
