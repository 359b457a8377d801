"""Shared by tests/test_shortlist_cpu.py and tests/test_hip_shortlist.py: ragged segment cases for the long selection (lengths around
the list length, the direct-sort limit and the chunk; random, heavily tied, all-equal and special values), and an NRMS model over a
``devset_tiny``-sized news table (``dot_topk_common``'s model and brute force on 512 news)."""
import functools
import types

import numpy as np
import torch

import dot_topk_common as D

CHUNK = 16384            # evaluate.TOPK_CHUNK
SMALL = 1024             # the longest segment level 2 sorts directly
MS = (1, 128, 129, 255, 256, 257, 1000, 1024)
KINDS = ("random", "seven", "equal", "special")
NEWS, USERS = 512, 6     # devset_tiny's news_num


def lengths(m):
    """Every length at which the selection takes another path, for list length m."""
    return sorted({0, 1, m - 1, m, m + 1, SMALL, SMALL + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5})


def values(rng, kind, n):
    if kind == "random":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "seven":                               # seven values: ties straddle every chunk edge and fill the threshold bin
        return rng.integers(-3, 4, size=n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0], dtype=np.float32)
    hit = rng.random(n) < 0.3
    x[hit] = special[rng.integers(0, len(special), size=int(hit.sum()))]
    return x


def plant_edges(x, start):
    """NaN, +-inf and the two zeros at the first and last element of every segment and on both sides of its chunk edges."""
    plant = np.array([np.nan, np.inf, -0.0, 0.0, -np.inf], dtype=np.float32)
    n = 0
    for a, b in zip(start[:-1], start[1:]):
        for p in (0, 255, 256, SMALL - 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, b - a - 1):
            if 0 <= p < b - a:
                x[a + p] = plant[n % len(plant)]
                n += 1
    return x


def segment_case(rng, m, kind, with_ids, skip_len):
    """``(scores [R], seg_start [S+1], ids [R] or None, skip [S, skip_len] or None)``: ``lengths(m)`` in a shuffled order.  Ids repeat
    (2000 values), and a skip row names ids of its own segment, so that it removes elements — from a short segment most of them."""
    lens = np.array(lengths(m), dtype=np.int64)[rng.permutation(len(lengths(m)))]
    start = np.r_[0, np.cumsum(lens)].astype(np.int64)
    x = values(rng, kind, int(start[-1]))
    if kind == "special":
        x = plant_edges(x, start)
    ids = rng.integers(0, 2000, size=len(x)).astype(np.int64) if with_ids else None
    skip = None
    if with_ids and skip_len:
        skip = np.full((len(lens), skip_len), 2001, dtype=np.int64)
        for s, (a, b) in enumerate(zip(start[:-1], start[1:])):
            if b > a:
                skip[s] = ids[a + rng.integers(0, b - a, size=skip_len)]
    return x, start, ids, skip


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    """Score bits, ids and counts of two ``(scores, ids, count)`` triples (tensors or arrays)."""
    s, i, c = (np.asarray(t.cpu()) if torch.is_tensor(t) else np.asarray(t) for t in got)
    ws, wi, wc = (np.asarray(t.cpu()) if torch.is_tensor(t) else np.asarray(t) for t in want)
    assert s.shape == ws.shape and i.shape == wi.shape and c.shape == wc.shape, (what, s.shape, ws.shape)
    assert s.dtype == np.float32 and i.dtype == np.int64 and c.dtype == np.int32, what
    assert np.array_equal(c, wc), (what, "count", c.tolist(), wc.tolist())
    assert np.array_equal(i, wi), (what, "ids", np.argwhere(i != wi)[:5].tolist())
    assert np.array_equal(bits(s), bits(ws)), (what, "score bits", np.argwhere(bits(s) != bits(ws))[:5].tolist())


@functools.lru_cache(maxsize=None)
def inputs(seed=5):
    from digat_amd import synthetic
    return synthetic.make_nrms_inputs(NEWS, D.AUG, D.LW, D.VOCAB, USERS, D.HIST, 5, seed=seed)


def dev_set(device="cpu"):
    """``dot_topk_common.dev_set`` over 512 news."""
    t = {k: torch.from_numpy(v.astype(np.int64)).to(device) for k, v in inputs().items()}
    return types.SimpleNamespace(title_text=t["title_text"], title_mask=t["title_mask"], augmented_title_text=t["augmented_title_text"],
                                 augmented_title_mask=t["augmented_title_mask"], history_ids=t["history_ids"], history_mask=t["history_mask"])
