"""Shared by tests/test_rerank_cpu.py and tests/test_hip_rerank.py: the lists, categories, targets and vectors of every case of the
joint re-rank from one generator (``calibrate_common.make_case`` plus vectors of two kinds), the weight triples, a plain-Python
float64 brute force of the literal objective and the comparison of a result with an expected one.  The CPU suite holds every case to
be robust at its seed (``rerank_select_host(return_robust=True)``), so that the GPU suite may compare picks exactly."""
import math

import numpy as np

import calibrate_common as K

NEWS = K.NEWS
ALPHA = 0.01
SEED = 0
WEIGHTS = ((0.5, 0.3, 0.2), (0.4, 0.2, 0.4))                          # (w_rel, w_div, w_cal)
# (kind, M, C, k, d).  grid: entries multiples of 1/8 in [-1, 1] — every product sum is exact in fp32 for d <= 512, so sim is the same
# in any order; unit: standard normal rows, normalised
CASES = (("grid", 1, 1, 1, 1), ("grid", 64, 17, 10, 3), ("grid", 65, 17, 10, 33), ("grid", 128, 64, 128, 32), ("grid", 129, 17, 16, 64),
         ("grid", 257, 17, 32, 64), ("grid", 1024, 17, 128, 64),
         ("unit", 128, 17, 10, 512), ("unit", 129, 17, 10, 400), ("unit", 1024, 64, 100, 400))


def groups_of(M):
    return 37 if M <= 257 else 8                                      # the twin takes about 0.2 s per list of 1024


def make_vectors(kind, seed, d, N=NEWS):
    rng = np.random.default_rng(1000 + seed)
    if kind == "grid":
        return (rng.integers(-8, 9, size=(N, d)) / 8.0).astype(np.float32)
    v = rng.standard_normal((N, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_case(kind, M, C, d, seed=SEED, groups=None):
    """``(ids [G,M], scores [G,M], count [G], category [N], target [G,C], vectors [N,d])``."""
    return K.make_case(seed, M, C, groups=groups or groups_of(M)) + (make_vectors(kind, seed, d),)


def host_gram(ids, vectors):
    """sim [G, M, M] float32 from the float64 product of the gathered rows (an id outside [0, N) gathers row 0: no element).  Exact
    for grid vectors; for unit vectors within an ulp or two of any fp32 chain."""
    N = len(vectors)
    safe = np.where((ids >= 0) & (ids < N), ids, 0)
    rows = vectors.astype(np.float64)[safe]
    return np.matmul(rows, rows.transpose(0, 2, 1)).astype(np.float32)


def brute_force(ids, scores, count, sim, category, target, k, w, alpha=ALPHA, max_per_category=0):
    """One list, plain Python floats: at every step the eligible element that maximises the LITERAL objective ``w_rel s - w_div max(0,
    max over the picked of sim) - w_cal KL(p || q of the list it would make)``, ties to the lowest position, NaNs last.  Returns the
    positions."""
    wr, wd, wc = (float(np.float32(x)) for x in w)
    M, N, C = len(ids), len(category), len(target)
    c = M if count is None else max(0, min(M, int(count)))
    elems = [p for p in range(c) if 0 <= int(ids[p]) < N]
    p_c = [float(x) if math.isfinite(float(x)) and float(x) > 0 else 0.0 for x in target]
    cat = {p: int(category[int(ids[p])]) for p in elems}

    def kl(n, T):
        return math.fsum(p_c[j] * (math.log(p_c[j]) - math.log((1.0 - alpha) * n[j] / T + alpha * p_c[j])) for j in range(C) if p_c[j] > 0)
    picked, n = [], [0] * C
    for t in range(k):
        cand = []
        for p in elems:
            if p in picked:
                continue
            if max_per_category and sum(1 for j in picked if cat[j] == cat[p]) >= max_per_category:
                continue
            m = list(n)
            if 0 <= cat[p] < C:
                m[cat[p]] += 1
            pen = max([0.0] + [float(sim[j][p]) for j in picked])
            value = wr * float(scores[p]) - wd * pen - wc * kl(m, t + 1.0)
            cand.append((1, 0.0, p) if math.isnan(value) else (0, -value, p))
        if not cand:
            break
        j = sorted(cand)[0][2]
        picked.append(j)
        if 0 <= cat[j] < C:
            n[cat[j]] += 1
    return picked


def same(got, want, category, target, alpha=ALPHA, what="", lists=None):
    """``(scores, ids, count, kl)`` against the twin's: counts, ids and score bits exactly, ``kl`` inside ``calibrate_common.kl_bound``
    (exactly 0 without a target).  ``lists``: the rows compared (None: all)."""
    host = [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in got]
    want = [np.asarray(x) for x in want[:4]]
    if lists is not None:
        host, want = [x[lists] for x in host], [x[lists] for x in want]
        target = None if target is None else np.asarray(target)[lists]
    if target is None:
        K.V.same(host[:3], want[:3], what)
        assert host[3].dtype == np.float32 and not host[3].any() and not want[3].any(), (what, "kl without a target")
    else:
        K.same(host, want, category, target, alpha, what)
