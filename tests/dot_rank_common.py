"""Shared by tests/test_dot_rank_cpu.py and tests/test_hip_dot_rank.py: a brute-force ``sorted()`` rank over a score matrix, target
lists with the positions a chunked kernel can get wrong, and ``dot_topk_common``'s dev object with impression rows."""
import math
import types

import numpy as np

import dot_topk_common as D

CANDS = 5                                # candidates per impression in D.inputs()


def brute_ranks(scores, target_pos, target_start, pool=None, skip=None, news_num=None):
    """rank [T] int32 by sorting every user's elements as Python tuples (NaN last, score descending, position ascending): the place
    of the target's own tuple, -1 where the target is no element (position outside the pool, id outside [0, news_num), id in the
    user's skip row)."""
    S = np.asarray(scores, dtype=np.float32)
    G, P = S.shape
    ids = list(range(P)) if pool is None else [int(v) for v in pool]
    out = np.full(len(target_pos), -1, dtype=np.int32)
    for g in range(G):
        banned = set() if skip is None else {int(v) for v in skip[g]}
        elems = []
        for p in range(P):
            if ids[p] in banned or ids[p] < 0 or (news_num is not None and ids[p] >= news_num):
                continue
            x = float(S[g, p])
            elems.append((1, 0.0, p) if math.isnan(x) else (0, -x, p))
        elems.sort()                     # -0.0 == 0.0 for Python too: signed zeros tie and fall back to the position
        place = {e[2]: r for r, e in enumerate(elems)}
        for t in range(int(target_start[g]), int(target_start[g + 1])):
            out[t] = place.get(int(target_pos[t]), -1)
    return out


def edge_positions(P, chunk):
    """Positions 0, P - 1 and both sides of every chunk edge inside the pool."""
    edges = {0, P - 1}
    for c in range(chunk, P, chunk):
        edges |= {c - 1, c}
    return sorted(e for e in edges if 0 <= e < P)


def make_targets(rng, G, P, per_user, chunk):
    """``(target_pos [T] int64, target_start [G+1] int64)``: user g gets ``per_user[g % len]`` random positions (repeats happen);
    the last user gets ``edge_positions`` on top, so every call ranks both sides of every chunk edge."""
    pos, start = [], [0]
    for g in range(G):
        mine = rng.integers(0, P, size=per_user[g % len(per_user)]).astype(np.int64)
        if g == G - 1:
            mine = np.r_[mine, np.asarray(edge_positions(P, chunk), dtype=np.int64)]
        pos.append(mine)
        start.append(start[-1] + len(mine))
    return np.concatenate(pos), np.asarray(start, dtype=np.int64)


def dev_with_rows(device="cpu", labels=None, seed=3):
    """``D.dev_set`` with the impression rows ``nrms.compute_scores`` reads: every user's ``candidate_ids`` in order, and ``labels``
    [USERS, CANDS] (None: every candidate clicked)."""
    dev = D.dev_set(device, seed)
    cand = D.inputs(seed)["candidate_ids"]
    lab = np.ones_like(cand) if labels is None else np.asarray(labels)
    assert cand.shape == lab.shape == (D.USERS, CANDS)
    return types.SimpleNamespace(**vars(dev), row_candidate=cand.reshape(-1).astype(np.int64),
                                 row_impression=np.repeat(np.arange(D.USERS, dtype=np.int64), CANDS), row_label=lab.reshape(-1).astype(np.int64))
