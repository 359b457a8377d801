"""Shared by tests/test_list_quality_cpu.py and tests/test_hip_list_quality.py: a brute force of the list-quality contract for one
list in plain Python, the bound on ``sim_sum``, and the comparison of a result dict with an expected one.  The awkward lists
(ragged counts, ids outside the table, repeated ids) are ``diversify_common.make_lists``."""
import math

import numpy as np

INT_KEYS = ("elements", "categories", "category_max", "overlap", "exposure")


def elements_of(ids, count, N):
    k = len(ids)
    c = k if count is None else max(0, min(k, int(count)))
    return [p for p in range(c) if 0 <= int(ids[p]) < N]


def brute_force(ids, count, N, sim=None, category=None, base_ids=None, base_count=None):
    """One list, plain Python: the dict of ``list_quality_host`` with scalars.  ``sim[p][q]`` is read as given, p < q."""
    elems = elements_of(ids, count, N)
    out = {"elements": len(elems)}
    if sim is not None:
        vals = [float(sim[p][q]) for i, p in enumerate(elems) for q in elems[i + 1:]]
        out["sim_sum"] = math.fsum(vals)
        best = -math.inf
        for x in vals:
            if not math.isnan(x) and x > best:
                best = x
        out["sim_max"] = 0.0 if best == 0 else best                  # a maximum of zero is +0.0
    if category is not None:
        seen = {}
        for p in elems:
            c = int(category[int(ids[p])])
            seen[c] = seen.get(c, 0) + 1
        out["categories"], out["category_max"] = len(seen), max(seen.values(), default=0)
    if base_ids is not None:
        base = {int(base_ids[p]) for p in elements_of(base_ids, base_count, N)}
        out["overlap"] = sum(1 for p in elems if int(ids[p]) in base)
    return out


def sum_bound(ids, count, sim, N):
    """[G] float64: ``pairs * 2^-52 * sum |sim(p, q)|`` over a list's element pairs — what a double sum of ``pairs`` float32 terms
    in ANY order can differ by from the exactly rounded sum (each of the pairs - 1 additions errs by at most 2^-53 of a partial
    sum that never exceeds the sum of the magnitudes, and the exact sum's own rounding is another 2^-53 of it)."""
    ids = np.asarray(ids)
    out = np.zeros(len(ids), dtype=np.float64)
    for g in range(len(ids)):
        el = elements_of(ids[g], None if count is None else count[g], N)
        vals = [abs(float(sim[g][p][q])) for i, p in enumerate(el) for q in el[i + 1:]]
        out[g] = len(vals) * 2.0 ** -52 * math.fsum(vals)
    return out


def host(x):
    return np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x)


def bits(x):
    return np.ascontiguousarray(host(x), dtype=np.float32).view(np.uint32)


def same(got, want, bound=None, what=""):
    """Two result dicts: the same keys; every integer output exactly; ``sim_max`` by bits; ``sim_sum`` within ``bound`` [G]
    (``sum_bound``) of the expected — exactly rounded — value, or by bits when ``bound`` is None."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in got:
        g, w = host(got[key]), host(want[key])
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        if key in INT_KEYS:
            assert g.dtype.kind == "i" and (key == "exposure" or g.dtype == np.int32), (what, key, g.dtype)
            bad = np.flatnonzero(g.astype(np.int64) != w.astype(np.int64))
            assert bad.size == 0, (what, key, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
        elif key == "sim_max":
            assert g.dtype == np.float32, (what, g.dtype)
            bad = np.flatnonzero(bits(g) != bits(w))
            assert bad.size == 0, (what, key, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
        else:
            assert key == "sim_sum" and g.dtype == np.float64, (what, key, g.dtype)
            if bound is None:
                bad = np.flatnonzero(g.view(np.uint64) != w.astype(np.float64).view(np.uint64))
            else:
                bad = np.flatnonzero(~(np.abs(g - w) <= bound))
            assert bad.size == 0, (what, key, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
