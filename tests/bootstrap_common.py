"""Shared by tests/test_bootstrap_cpu.py and tests/test_hip_bootstrap.py: an independent scalar restatement of the bootstrap draws
(plain Python integers, no numpy), value tables, the bound of a double sum against the correctly rounded one, and a direct numpy
computation of what ``metric_intervals`` / ``compare_metrics`` return from the draws."""
import numpy as np

SLICE = 8192                     # include/digat_hip.h: DIGAT_BOOTSTRAP_SLICE
MAX_COLUMNS = 16                 # ... DIGAT_BOOTSTRAP_MAX_COLUMNS
M32 = 0xFFFFFFFF


def hash32(x):
    x &= M32
    x ^= x >> 16
    x = x * 0x7feb352d & M32
    x ^= x >> 15
    x = x * 0x846ca68b & M32
    return x ^ (x >> 16)


def draw(n, replicate, j, seed):
    """The unit of draw j of a replicate, in Python integers."""
    e = replicate * n + j
    w = hash32(((e & M32) * 0x9E3779B9 & M32) + hash32((seed & M32) + (e >> 32)))
    return (w * n) >> 32


def real_values(seed, n, c):
    """Reals of mixed sign and widely different magnitudes: a sum whose rounding depends on its order."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, c)) * 10.0 ** rng.integers(-3, 4, size=(n, c))


def integer_values(seed, n, c):
    """Integers in [-2^20, 2^20]: every partial sum of up to 2^31 of them is an integer below 2^53 — exact in any order."""
    return np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, size=(n, c)).astype(np.float64)


def sum_bound(values, idx):
    """[B, c]: ``n 2^-53 sum_j |values[idx_j]|`` — a double sum of n terms in ANY order against their correctly rounded sum (each
    of the n - 1 additions rounds a partial sum that is at most sum |terms| by half an ulp, and the yardstick's own rounding is one
    more half ulp: n half ulps in all)."""
    v = np.abs(np.asarray(values, dtype=np.float64))
    n = v.shape[0]
    return n * 2.0 ** -53 * np.stack([v[idx[b]].sum(axis=0) for b in range(idx.shape[0])])


def quantile_linear(x, q):
    """The ``method="linear"`` rule by hand: position q (B - 1) in the sorted replicates, interpolated."""
    s = sorted(float(v) for v in x)
    pos = q * (len(s) - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(s) - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


def direct_interval(stats, value, level):
    stats = np.asarray(stats, dtype=np.float64)
    a = (1.0 - level) / 2.0
    return {"value": float(value), "lo": quantile_linear(stats, a), "hi": quantile_linear(stats, 1.0 - a),
            "se": float(np.sqrt(((stats - stats.mean()) ** 2).sum() / (len(stats) - 1))), "replicates": len(stats), "level": level}


def direct_paired(a, b, diffs, level):
    diffs = np.asarray(diffs, dtype=np.float64)
    f = direct_interval(diffs, a - b, level)
    B = len(diffs)
    le, ge = sum(1 for d in diffs if d <= 0), sum(1 for d in diffs if d >= 0)
    return {"a": float(a), "b": float(b), "diff": float(a - b), "lo": f["lo"], "hi": f["hi"], "se": f["se"],
            "p": min(1.0, 2.0 * min((le + 1) / (B + 1), (ge + 1) / (B + 1))), "wins": sum(1 for d in diffs if d > 0) / B}


def same_fields(got, want, rel, what=""):
    """Two result dicts (name -> fields) agree: integers and the level exactly, floats within ``rel`` (0: exactly), NaN with NaN."""
    assert list(got) == list(want), (what, list(got), list(want))
    for name in want:
        assert list(got[name]) == list(want[name]), (what, name)
        for f, w in want[name].items():
            g = got[name][f]
            if isinstance(w, float) and np.isnan(w):
                assert np.isnan(g), (what, name, f, g)
            elif rel == 0 or f in ("replicates", "level"):
                assert g == w, (what, name, f, g, w)
            else:
                assert abs(g - w) <= rel * max(abs(w), abs(g)) + 1e-300, (what, name, f, g, w)
