"""Ranking + metrics of the dev/test driver (the reference's util.py:70-80 and evaluate.py:7-89).

``impression_ranks``: per impression, stable descending sort of the scores -> 1-based rank of every
candidate (ties keep candidate order, as Python's stable ``list.sort(reverse=True)`` does).
``scoring``: AUC / MRR / nDCG@5 / nDCG@10 averaged over impressions on ``1/rank`` scores.
Vectorised numpy; AUC by the rank-sum identity (ranks are distinct, so no tie handling is needed —
identical to ``sklearn.metrics.roc_auc_score`` on these inputs).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np


def impression_ranks(scores: np.ndarray, row_impression: np.ndarray) -> np.ndarray:
    """ranks[r] = 1-based rank of row r inside its impression (rows are impression-major)."""
    scores = np.asarray(scores, dtype=np.float64)
    imp = np.asarray(row_impression, dtype=np.int64)
    n = len(scores)
    # stable sort by (impression ascending, score descending): lexsort is stable, last key is primary
    order = np.lexsort((-scores, imp))
    starts = np.r_[0, np.flatnonzero(np.diff(imp[order])) + 1]
    first_of_group = np.repeat(starts, np.diff(np.r_[starts, n]))
    ranks = np.empty(n, dtype=np.int64)
    ranks[order] = np.arange(n) - first_of_group + 1
    return ranks


def rank_lines(ranks: np.ndarray, row_impression: np.ndarray) -> List[str]:
    """``"<impression id> [r1,r2,...]"`` per impression (util.py:74-80), ids are 1-based."""
    imp = np.asarray(row_impression, dtype=np.int64)
    lines = []
    bounds = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, len(imp)]
    count = int(imp[-1]) + 1 if len(imp) else 0
    per_imp = {int(imp[s]): ranks[s:e] for s, e in zip(bounds[:-1], bounds[1:])}
    for i in range(count):
        r = per_imp.get(i, np.zeros(0, dtype=np.int64))
        lines.append(f"{i + 1} " + str(r.tolist()).replace(" ", ""))      # the reference's own formatting (util.py:80), at C speed
    return lines


def _dcg(labels_sorted: np.ndarray, k: int) -> float:
    g = labels_sorted[:k]
    return float(np.sum((2.0 ** g - 1.0) / np.log2(np.arange(len(g)) + 2.0)))


def impression_metric_rows(labels: np.ndarray, ranks: np.ndarray, row_impression: np.ndarray) -> np.ndarray:
    """[I, 4] float64: (AUC, MRR, nDCG@5, nDCG@10) of every impression that has at least one row — the values ``scoring`` averages.
    An impression without a positive or without a negative divides by zero: its row is not finite."""
    labels = np.asarray(labels, dtype=np.float64)
    imp = np.asarray(row_impression, dtype=np.int64)
    bounds = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, len(imp)] if len(imp) else np.zeros(1, dtype=np.int64)
    out = np.empty((len(bounds) - 1, 4), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
            y, r = labels[s:e], ranks[s:e].astype(np.float64)
            n_pos = float(y.sum())
            n_neg = float(len(y) - n_pos)
            # score = 1/rank is strictly decreasing in rank, so ascending-score rank = len - rank + 1
            asc = len(y) - r + 1.0
            out[i, 0] = (asc[y > 0].sum() - n_pos * (n_pos + 1) / 2.0) / np.float64(n_pos * n_neg)
            by_rank = y[np.argsort(r, kind="stable")]
            out[i, 1] = np.sum(by_rank / (np.arange(len(y)) + 1.0)) / np.float64(n_pos)
            ideal = np.sort(y)[::-1]
            out[i, 2] = np.float64(_dcg(by_rank, 5)) / np.float64(_dcg(ideal, 5))
            out[i, 3] = np.float64(_dcg(by_rank, 10)) / np.float64(_dcg(ideal, 10))
    return out


def scoring(labels: np.ndarray, ranks: np.ndarray, row_impression: np.ndarray) -> Tuple[float, float, float, float]:
    """(AUC, MRR, nDCG@5, nDCG@10), mean over impressions that have at least one row."""
    per = impression_metric_rows(labels, ranks, row_impression)
    return tuple(float(np.mean(np.ascontiguousarray(per[:, k]))) for k in range(4))


def rank_file_bytes(ranks: np.ndarray, row_impression: np.ndarray) -> bytes:
    """``"\\n".join(rank_lines(ranks, row_impression))`` as bytes, formatted by the library's host-side C routine
    (``digat_format_rank_file``): the Python loop spends 0.3 s of a 3 s MIND-small dev run on 2.7 M integers."""
    import ctypes
    from . import _lib
    imp = np.asarray(row_impression, dtype=np.int64)
    r = np.ascontiguousarray(ranks, dtype=np.int64)
    if imp.size == 0:
        return b""
    count = int(imp[-1]) + 1
    starts = np.ascontiguousarray(np.r_[0, np.cumsum(np.bincount(imp, minlength=count))], dtype=np.int64)
    L = _lib.lib()
    need = L.digat_format_rank_file(r.ctypes.data, starts.ctypes.data, count, None, 0)
    buf = ctypes.create_string_buffer(int(need))
    got = L.digat_format_rank_file(r.ctypes.data, starts.ctypes.data, count, ctypes.addressof(buf), need)
    assert got == need
    return buf.raw[:got]


def device_ranks_and_metrics(scores, row_impression: np.ndarray, labels: np.ndarray = None):
    """Ranks (and, with labels, the four metrics) computed on the GPU by ``digat_rank_metrics``.

    ``scores``: a CUDA float32 tensor [R] in impression-major row order; ``row_impression`` / ``labels``: host
    arrays.  Returns ``(ranks int64 numpy [R], (auc, mrr, ndcg5, ndcg10) or None)`` — the same values as
    ``impression_ranks`` + ``scoring`` (ranks identical; metrics equal to float64 rounding)."""
    import torch
    from . import _lib
    imp = np.asarray(row_impression, dtype=np.int64)
    R = len(imp)
    dev = _lib.require_device(scores)
    if R == 0:
        return np.zeros(0, dtype=np.int64), None
    if np.any(np.diff(imp) < 0):
        raise ValueError("rows must be impression-major")
    starts = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, R].astype(np.int64)
    I = len(starts) - 1
    sc = scores.detach().to(torch.float32).contiguous()
    st = torch.from_numpy(starts).to(dev)
    ranks = torch.empty(R, dtype=torch.int32, device=dev)
    lab = per = mean = None
    if labels is not None:
        lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels) > 0).view(np.uint8)).to(dev)
        per = torch.empty((I, 4), dtype=torch.float64, device=dev)
        mean = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().digat_rank_metrics(sc.data_ptr(), lab.data_ptr() if lab is not None else None, st.data_ptr(), I,
                                             ranks.data_ptr(), per.data_ptr() if per is not None else None,
                                             mean.data_ptr() if mean is not None else None, _lib.stream_ptr()),
               "digat_rank_metrics")
    metrics = tuple(float(v) for v in mean.cpu().numpy()) if mean is not None else None
    return ranks.cpu().numpy().astype(np.int64), metrics


def ranks_metrics_file(scores, row_impression: np.ndarray, labels=None, result_file=None):
    """The end of a dev run: ``(ranks int64 numpy [R], (auc, mrr, ndcg5, ndcg10) or None)`` of a score tensor [R] — on the device
    for CUDA scores (``device_ranks_and_metrics``), ``impression_ranks`` + ``scoring`` for host ones — and the rank file written
    to ``result_file`` when one is named."""
    if scores.is_cuda:
        ranks, metrics = device_ranks_and_metrics(scores, row_impression, labels)
    else:
        ranks = impression_ranks(scores.detach().numpy(), row_impression)
        metrics = scoring(np.asarray(labels), ranks, row_impression) if labels is not None else None
    if result_file is not None:
        with open(result_file, "wb") as f:
            f.write(rank_file_bytes(ranks, row_impression))
    return ranks, metrics


TOPK_CHUNK = 16384       # include/digat_hip.h: DIGAT_TOPK_CHUNK, the elements one level-1 workgroup of digat_topk_segments selects from
TOPK_MAX_K = 128
TOPK_MAX_SKIP = 256
SHORTLIST_MAX_K = 1024   # include/digat_hip.h: DIGAT_SHORTLIST_MAX_K, the longest list of digat_shortlist_segments / digat_dot_shortlist
SHORTLIST_SLAB_USERS = 256      # the users digat_dot_shortlist scores at a time when the caller names no slab
_TOPK_LIMIT = ("k", "%d" % TOPK_MAX_K, TOPK_MAX_K)      # what a selection calls its list length, how it words the bound, the bound
_SHORTLIST_LIMIT = ("m", "SHORTLIST_MAX_K = %d" % SHORTLIST_MAX_K, SHORTLIST_MAX_K)


def topk_keys(scores: np.ndarray) -> np.ndarray:
    """The kernel's monotone 32-bit key of every score (csrc/digat_topk.inc): a larger key orders first.  ``-0.0`` and ``+0.0``
    share a key, every NaN has key 1 — below ``-inf``'s 0x007fffff."""
    b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 1
    return key


def topk_segments_host(scores, seg_start, k: int, ids=None, skip=None):
    """The contract of ``digat_topk_segments`` in numpy — the yardstick of the kernel.  Per segment: the elements whose id is not
    in the segment's ``skip`` row, in a stable descending sort of their keys (``topk_keys``: ties keep position order, NaNs last),
    the first k of them.  Returns ``(scores [S,k] float32, ids [S,k] int64, count [S] int32)``; slots at or beyond ``count`` hold
    ``-inf`` / ``-1``; without ``ids`` the position inside the segment is returned."""
    return _select_segments_host(scores, seg_start, k, ids, skip, _TOPK_LIMIT)


def _select_segments_host(scores, seg_start, k, ids, skip, limit):
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    st = np.asarray(seg_start, dtype=np.int64)
    _check_topk_args(len(sc), st.shape, k, None if ids is None else np.shape(ids), None if skip is None else np.shape(skip), limit)
    S = len(st) - 1
    out_s = np.full((S, k), -np.inf, dtype=np.float32)
    out_i = np.full((S, k), -1, dtype=np.int64)
    count = np.zeros(S, dtype=np.int32)
    keys = topk_keys(sc).astype(np.int64)
    idv = None if ids is None else np.asarray(ids, dtype=np.int64)
    skv = None if skip is None else np.asarray(skip, dtype=np.int64).reshape(S, -1)
    for s in range(S):
        a, b = int(st[s]), int(st[s + 1])
        pos = np.arange(b - a, dtype=np.int64)
        if skv is not None and skv.shape[1]:
            pos = pos[~np.isin(idv[a:b], skv[s])]
        order = pos[np.argsort(-keys[a:b][pos], kind="stable")][:k]
        m = len(order)
        count[s] = m
        out_s[s, :m] = sc[a:b][order]
        out_i[s, :m] = order if idv is None else idv[a:b][order]
    return out_s, out_i, count


def _check_limit(k, limit=_TOPK_LIMIT) -> int:
    name, words, bound = limit
    if not 1 <= int(k) <= bound:
        raise ValueError(f"{name} must be in [1, {words}], got {k}")
    return int(k)


def _check_topk_args(rows, start_shape, k, ids_shape, skip_shape, limit=_TOPK_LIMIT):
    _check_limit(k, limit)
    if len(start_shape) != 1 or start_shape[0] < 1:
        raise ValueError("seg_start must be a 1-D array of segments + 1 row offsets")
    if ids_shape is not None and tuple(ids_shape) != (rows,):
        raise ValueError(f"ids must have one entry per score ({rows}), got shape {tuple(ids_shape)}")
    if skip_shape is not None:
        if ids_shape is None:
            raise ValueError("skip needs ids")
        if len(skip_shape) != 2 or skip_shape[0] != start_shape[0] - 1 or skip_shape[1] > TOPK_MAX_SKIP:
            raise ValueError(f"skip must be [segments, at most {TOPK_MAX_SKIP}], got shape {tuple(skip_shape)}")


def topk_segments(scores, seg_start, k: int, ids=None, skip=None):
    """Per segment of a ragged score array, the k best elements in order, on the GPU (``digat_topk_segments``).

    ``scores`` [R] float32 and ``seg_start`` [S+1] int64 (non-decreasing row offsets) are device tensors; ``ids`` [R] int64
    (returned in place of positions) and ``skip`` [S, L <= 256] int64 (ids a segment must not return) are optional.  Order: score
    descending, ties by position — the rank file's; NaNs last.  Returns ``(scores [S,k] float32, ids [S,k] int64, count [S] int32)``
    on the device; slots at or beyond ``count`` hold ``-inf`` / ``-1``.  Stream-ordered: nothing is read back."""
    return _select_segments(scores, seg_start, k, ids, skip, _TOPK_LIMIT, "digat_topk_segments", "topk")


def _select_segments(scores, seg_start, k, ids, skip, limit, entry, tag):
    import torch
    from . import _lib
    given = [t for t in (scores, seg_start, ids, skip) if t is not None]
    dev = _lib.require_device(*given)
    _check_topk_args(int(scores.shape[0]) if scores.dim() == 1 else -1, tuple(seg_start.shape), k,
                     None if ids is None else tuple(ids.shape), None if skip is None else tuple(skip.shape), limit)
    if scores.dim() != 1:
        raise ValueError("scores must be 1-D")
    sc = _lib.f32(scores.detach())
    st = seg_start.to(torch.int64).contiguous()
    idt = None if ids is None else ids.to(torch.int64).contiguous()
    sk = None if skip is None or skip.shape[1] == 0 else skip.to(torch.int64).contiguous()
    R, S, k = int(sc.shape[0]), int(st.shape[0]) - 1, int(k)
    out_s = torch.empty((S, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((S, k), dtype=torch.int64, device=dev)
    count = torch.empty((S,), dtype=torch.int32, device=dev)
    if S == 0:
        return out_s, out_i, count
    L = _lib.lib()
    need = int(getattr(L, entry + "_workspace_bytes")(R, S, k))
    ws = _lib.workspace(need, dev, tag)
    dummy = ws if R == 0 else sc                        # an empty tensor has no storage to point at
    _lib.check(getattr(L, entry)(dummy.data_ptr(), st.data_ptr(), R, S, _lib.ptr(idt) if R else None,
                                 _lib.ptr(sk) if R else None, 0 if sk is None or not R else int(sk.shape[1]), k,
                                 out_s.data_ptr(), out_i.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()),
               entry)
    return out_s, out_i, count


def shortlist_segments_host(scores, seg_start, m: int, ids=None, skip=None):
    """The contract of ``digat_shortlist_segments`` in numpy: ``topk_segments_host`` with lists of up to ``SHORTLIST_MAX_K``."""
    return _select_segments_host(scores, seg_start, m, ids, skip, _SHORTLIST_LIMIT)


def shortlist_segments(scores, seg_start, m: int, ids=None, skip=None):
    """``topk_segments`` for lists of up to ``SHORTLIST_MAX_K`` = 1024 entries, on the GPU (``digat_shortlist_segments``): the same
    arguments, order and returns — ``(scores [S,m] float32, ids [S,m] int64, count [S] int32)`` — and for ``m <= 128`` the same bits.
    The winners of a long list are ordered by a sort in LDS where ``topk_segments`` counts ranks."""
    return _select_segments(scores, seg_start, m, ids, skip, _SHORTLIST_LIMIT, "digat_shortlist_segments", "shortlist")


DOT_TOPK_CHUNK = 2048    # include/digat_hip.h: DIGAT_DOT_TOPK_CHUNK, the pool positions one level-1 workgroup of digat_dot_topk walks
DOT_TOPK_USERS = 64      # ... DIGAT_DOT_TOPK_USERS, the users of that workgroup's tile
DOT_TOPK_SUB = 64        # ... DIGAT_DOT_TOPK_SUB, the pool positions of one product sub-tile


def dot_topk_host(scores, k: int, pool=None, skip=None, limit=_TOPK_LIMIT):
    """The contract of ``digat_dot_topk`` on a given score matrix ``scores`` [G, P], in numpy: ``topk_segments_host`` over G
    segments of length P whose ids are ``pool`` (the positions when None).  Returns ``(scores [G,k], ids [G,k], count [G])``."""
    S = np.ascontiguousarray(scores, dtype=np.float32)
    if S.ndim != 2:
        raise ValueError("scores must be [G, P]")
    G, P = S.shape
    ids = np.arange(P, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64)
    if ids.shape != (P,):
        raise ValueError(f"pool must have one id per column ({P}), got shape {ids.shape}")
    return _select_segments_host(S.ravel(), np.arange(G + 1, dtype=np.int64) * P, k, np.tile(ids, G), skip, limit)


def dot_shortlist_host(scores, m: int, pool=None, skip=None):
    """The contract of ``digat_dot_shortlist`` on a given score matrix: ``dot_topk_host`` with lists of up to ``SHORTLIST_MAX_K``."""
    return dot_topk_host(scores, m, pool=pool, skip=skip, limit=_SHORTLIST_LIMIT)


def _check_dot_args(users, news, pool, skip=None, k=None, limit=_TOPK_LIMIT):
    import torch
    if users.dim() != 2 or news.dim() != 2 or users.shape[1] != news.shape[1] or users.shape[1] < 1:
        raise ValueError(f"users [G, d] and news [N, d] must share d >= 1, got {tuple(users.shape)} and {tuple(news.shape)}")
    G, N = int(users.shape[0]), int(news.shape[0])
    if k is not None:
        _check_limit(k, limit)
    if pool is not None:
        if pool.dim() != 1 or pool.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
            raise ValueError("pool must be a 1-D integer tensor of news rows")
        if pool.numel() and (int(pool.min()) < 0 or int(pool.max()) >= N):
            raise ValueError(f"pool ids must lie in [0, {N})")
    if skip is not None and (skip.dim() != 2 or skip.shape[0] != G or skip.shape[1] > TOPK_MAX_SKIP):
        raise ValueError(f"skip must be [users, at most {TOPK_MAX_SKIP}], got shape {tuple(skip.shape)}")
    return G, N, N if pool is None else int(pool.shape[0]), int(users.shape[1])


def dot_topk(users, news, k: int, pool=None, skip=None):
    """For every row of ``users`` [G, d] the k best rows of ``news`` [N, d] by inner product, on the GPU without the [G, P] score
    matrix (``digat_dot_topk``).  ``pool`` [P] int64: the news rows to choose from, in this order (None: all N); ``skip``
    [G, L <= 256] int64: ids a user must not get.  Order: score descending, ties by pool position, NaNs last.  Returns
    ``(scores [G,k] float32, ids [G,k] int64, count [G] int32)`` on the device; slots at or beyond ``count`` hold ``-inf`` / ``-1``.
    A score is the fp32 fmaf chain over the d channels: the bits ``dot_scores`` gives.  Stream-ordered; only the pool's id range is
    read back, for the check."""
    return _dot_select(users, news, k, pool, skip, _TOPK_LIMIT, None)


def _dot_select(users, news, k, pool, skip, limit, slab_users):
    """``dot_topk`` (``slab_users`` None) or ``dot_shortlist``: the checks, the outputs, the workspace and the call."""
    import torch
    from . import _lib
    given = [t for t in (users, news, pool, skip) if t is not None]
    dev = _lib.require_device(*given)
    G, N, P, d = _check_dot_args(users, news, pool, skip, k, limit)
    u, v = _lib.f32(users.detach()), _lib.f32(news.detach())
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    sk = None if skip is None or skip.shape[1] == 0 else skip.to(torch.int64).contiguous()
    k = int(k)
    out_s = torch.full((G, k), float("-inf"), dtype=torch.float32, device=dev)
    out_i = torch.full((G, k), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((G,), dtype=torch.int32, device=dev)
    if G == 0 or P == 0:
        return out_s, out_i, count
    L = _lib.lib()
    head = (u.data_ptr(), v.data_ptr(), _lib.ptr(pl), G, N, P, d, _lib.ptr(sk), 0 if sk is None else int(sk.shape[1]), k)
    outs = (out_s.data_ptr(), out_i.data_ptr(), count.data_ptr())
    if slab_users is None:
        need = int(L.digat_dot_topk_workspace_bytes(G, P, k))
        ws = _lib.workspace(need, dev, "dot_topk")
        _lib.check(L.digat_dot_topk(*head, *outs, ws.data_ptr(), need, _lib.stream_ptr()), "digat_dot_topk")
    else:
        need = int(L.digat_dot_shortlist_workspace_bytes(G, P, k, slab_users))
        ws = _lib.workspace(need, dev, "dot_shortlist")
        _lib.check(L.digat_dot_shortlist(*head, slab_users, *outs, ws.data_ptr(), need, _lib.stream_ptr()), "digat_dot_shortlist")
    return out_s, out_i, count


def dot_shortlist(users, news, m: int, pool=None, skip=None, slab_users=None):
    """``dot_topk`` for lists of up to ``SHORTLIST_MAX_K`` = 1024 entries (``digat_dot_shortlist``): the same arguments, elements,
    score bits, order and returns — ``(scores [G,m] float32, ids [G,m] int64, count [G] int32)``.  Lists this long do not fit the
    fused kernel's LDS, so the users are walked in slabs of ``slab_users`` (None: ``SHORTLIST_SLAB_USERS`` = 256; never more than
    G): per slab the [slab, P] scores are stored — ``dot_scores``' kernel — and selected from.  The workspace, slab x P x 4 bytes
    plus the selection's, does not grow with G; the results do not depend on the slab."""
    slab = SHORTLIST_SLAB_USERS if slab_users is None else int(slab_users)
    if slab < 1:
        raise ValueError(f"slab_users must be positive, got {slab_users}")
    return _dot_select(users, news, m, pool, skip, _SHORTLIST_LIMIT, max(1, min(slab, int(users.shape[0]))))


def dot_scores(users, news, pool=None):
    """``users`` [G, d] x ``news[pool]`` [P, d] -> [G, P] float32 on the GPU (``digat_dot_scores``): the product ``dot_topk`` selects
    from, bit for bit — its yardstick, and the way to the matrix for a caller who wants it."""
    import torch
    from . import _lib
    given = [t for t in (users, news, pool) if t is not None]
    dev = _lib.require_device(*given)
    G, N, P, d = _check_dot_args(users, news, pool)
    u, v = _lib.f32(users.detach()), _lib.f32(news.detach())
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    out = torch.empty((G, P), dtype=torch.float32, device=dev)
    if G and P:
        _lib.check(_lib.lib().digat_dot_scores(u.data_ptr(), v.data_ptr(), _lib.ptr(pl), G, N, P, d, out.data_ptr(), _lib.stream_ptr()),
                   "digat_dot_scores")
    return out


QDOT_MAX_D = 1024        # include/digat_hip.h: DIGAT_QDOT_MAX_D, the widest vectors the quantised entries take


def _qdot_width(d: int) -> int:
    if not 1 <= int(d) <= QDOT_MAX_D:
        raise ValueError(f"the quantised entries take vectors of 1 to QDOT_MAX_D = {QDOT_MAX_D} channels, got {d}")
    return (int(d) + 15) // 16 * 16


def quantize_rows_host(x):
    """The contract of ``digat_quantize_rows_i8`` in numpy float32 — the yardstick of the kernel, byte for byte.  ``x`` [R, d] ->
    ``(q int8 [R, dq], scale float32 [R])`` with dq = d rounded up to 16 and zeros from d on: per row ``amax = max |x|``,
    ``scale = amax / 127`` and ``q = clip(rint(x / scale), -127, 127)`` — float32 divisions, rint to nearest even.  ``scale == 0``
    (a zero row, an amax that underflows): codes 0.  A row with a NaN or an infinity: codes 0 and scale NaN."""
    X = np.ascontiguousarray(x, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("x must be [R, d]")
    R, d = X.shape
    dq = _qdot_width(d)
    q = np.zeros((R, dq), dtype=np.int8)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bad = ~np.isfinite(X).all(axis=1)
        amax = np.abs(np.where(bad[:, None], np.float32(0), X)).max(axis=1).astype(np.float32)
        scale = (amax / np.float32(127.0)).astype(np.float32)
        live = ~bad & (scale > 0)
        codes = np.clip(np.rint((X[live] / scale[live, None]).astype(np.float32)), -127, 127)
    q[live, :d] = codes.astype(np.int8)
    scale[bad] = np.float32("nan")
    return q, scale


def _check_qdot_host(qu, su, qn, sn):
    QU, QN = np.asarray(qu), np.asarray(qn)
    if QU.ndim != 2 or QN.ndim != 2 or QU.shape[1] != QN.shape[1] or QU.dtype != np.int8 or QN.dtype != np.int8:
        raise ValueError(f"qu [G, dq] and qn [N, dq] must be int8 codes of one width, got {QU.shape} {QU.dtype} and {QN.shape} {QN.dtype}")
    if QU.shape[1] != _qdot_width(QU.shape[1]):
        raise ValueError(f"rows of codes are padded to a multiple of 16, got dq = {QU.shape[1]}")
    SU, SN = np.ascontiguousarray(su, dtype=np.float32), np.ascontiguousarray(sn, dtype=np.float32)
    if SU.shape != (QU.shape[0],) or SN.shape != (QN.shape[0],):
        raise ValueError(f"one scale per row: su {SU.shape} for {QU.shape[0]} users, sn {SN.shape} for {QN.shape[0]} news")
    return QU, SU, QN, SN


def qdot_scores_host(qu, su, qn, sn, pool=None):
    """The contract of ``digat_qdot_scores`` in numpy — its bits: ``score(g, p) = (float32(acc) * su[g]) * sn[id]`` with ``acc`` the
    exact integer product of the code rows, ``id = pool[p]`` (None: p); a position whose id lies outside [0, N) holds +0.0."""
    QU, SU, QN, SN = _check_qdot_host(qu, su, qn, sn)
    N = QN.shape[0]
    ids = np.arange(N, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64)
    if ids.ndim != 1:
        raise ValueError("pool must be 1-D")
    ok = (ids >= 0) & (ids < N)
    safe = np.where(ok, ids, 0)
    acc = QU.astype(np.float64) @ QN[safe].astype(np.float64).T if N else np.zeros((QU.shape[0], len(ids)))     # exact: |acc| < 2^24
    with np.errstate(invalid="ignore", over="ignore"):
        S = ((acc.astype(np.float32) * SU[:, None]).astype(np.float32) * (SN[safe][None, :] if N else np.float32(0))).astype(np.float32)
    S[:, ~ok] = np.float32(0)
    return S


def qdot_bound(users, news, su, sn):
    """The derived error of a quantised score against the real product (csrc/digat_qdot.inc), float64 [G, N]:
    ``(sn/2 |u|_1 + su/2 |v|_1 + d su sn / 4) (1 + 2^-15)`` for the codes, plus ``2^-23 (|u|_2 |v|_2 + that)`` for the two fp32
    multiplications.  Rows with a NaN scale have no bound (NaN)."""
    U, V = np.asarray(users, dtype=np.float64), np.asarray(news, dtype=np.float64)
    SU, SN = np.asarray(su, dtype=np.float64), np.asarray(sn, dtype=np.float64)
    d = U.shape[1]
    u1, v1 = np.abs(U).sum(axis=1), np.abs(V).sum(axis=1)
    u2, v2 = np.sqrt((U * U).sum(axis=1)), np.sqrt((V * V).sum(axis=1))
    code = (0.5 * SN[None, :] * u1[:, None] + 0.5 * SU[:, None] * v1[None, :] + 0.25 * d * SU[:, None] * SN[None, :]) * (1.0 + 2.0 ** -15)
    return code + 2.0 ** -23 * (u2[:, None] * v2[None, :] + code)


def quantize_rows(x):
    """``x`` [R, d] float32 -> ``(q int8 [R, dq], scale float32 [R])``: per-row symmetric int8 codes, dq = d rounded up to 16 with a
    zero tail (``digat_quantize_rows_i8``; on CPU tensors ``quantize_rows_host``, the same bytes).  d <= ``QDOT_MAX_D`` = 1024."""
    import torch
    from . import _lib
    if x.dim() != 2:
        raise ValueError("x must be [R, d]")
    R, d = int(x.shape[0]), int(x.shape[1])
    dq = _qdot_width(d)
    if x.device.type != "cuda":
        return tuple(map(torch.from_numpy, quantize_rows_host(x.detach().float().numpy())))
    xs = _lib.f32(x.detach())
    q = torch.empty((R, dq), dtype=torch.int8, device=x.device)
    scale = torch.empty((R,), dtype=torch.float32, device=x.device)
    if R:
        _lib.check(_lib.lib().digat_quantize_rows_i8(xs.data_ptr(), R, d, dq, q.data_ptr(), scale.data_ptr(), _lib.stream_ptr()),
                   "digat_quantize_rows_i8")
    return q, scale


def _check_qdot_args(qu, su, qn, sn, pool, skip=None, k=None, limit=_TOPK_LIMIT):
    import torch
    if qu.dim() != 2 or qn.dim() != 2 or qu.shape[1] != qn.shape[1] or qu.dtype != torch.int8 or qn.dtype != torch.int8:
        raise ValueError(f"qu [G, dq] and qn [N, dq] must be int8 codes of one width, got {tuple(qu.shape)} {qu.dtype} and "
                         f"{tuple(qn.shape)} {qn.dtype}")
    dq = int(qu.shape[1])
    if dq != _qdot_width(dq):
        raise ValueError(f"rows of codes are padded to a multiple of 16, got dq = {dq}")
    if tuple(su.shape) != (qu.shape[0],) or tuple(sn.shape) != (qn.shape[0],) or su.dtype != torch.float32 or sn.dtype != torch.float32:
        raise ValueError("su [G] and sn [N] must hold one float32 scale per row of codes")
    G, N = int(qu.shape[0]), int(qn.shape[0])
    if k is not None:
        _check_limit(k, limit)
    if pool is not None:
        if pool.dim() != 1 or pool.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
            raise ValueError("pool must be a 1-D integer tensor of news rows")
        if pool.numel() and (int(pool.min()) < 0 or int(pool.max()) >= N):
            raise ValueError(f"pool ids must lie in [0, {N})")
    if skip is not None and (skip.dim() != 2 or skip.shape[0] != G or skip.shape[1] > TOPK_MAX_SKIP):
        raise ValueError(f"skip must be [users, at most {TOPK_MAX_SKIP}], got shape {tuple(skip.shape)}")
    return G, N, N if pool is None else int(pool.shape[0]), dq


def _qdot_head(qu, su, qn, sn, pl, G, N, P, dq):
    # the codes' tail is zero, so the padded width is the d the entry is told
    return (qu.data_ptr(), su.data_ptr(), qn.data_ptr(), sn.data_ptr(), None if pl is None else pl.data_ptr(), G, N, P, dq, dq)


def qdot_scores(qu, su, qn, sn, pool=None):
    """Quantised scores [G, P] float32 of code rows ``qu`` [G, dq] / ``qn`` [N, dq] (int8, ``quantize_rows``) with scales ``su`` [G] /
    ``sn`` [N]: ``(float32(acc) * su[g]) * sn[pool[p]]`` with ``acc`` the int32 product on the int8 matrix cores
    (``digat_qdot_scores``) — the bits ``qdot_topk`` and ``qdot_shortlist`` select from, and ``qdot_scores_host``'s, which CPU tensors
    go through.  ``qdot_bound`` holds them to the real product."""
    import torch
    from . import _lib
    G, N, P, dq = _check_qdot_args(qu, su, qn, sn, pool)
    if qu.device.type != "cuda":
        return torch.from_numpy(qdot_scores_host(qu.numpy(), su.numpy(), qn.numpy(), sn.numpy(), None if pool is None else pool.numpy()))
    dev = _lib.require_device(*[t for t in (qu, su, qn, sn, pool) if t is not None])
    qu, su, qn, sn = qu.contiguous(), su.contiguous(), qn.contiguous(), sn.contiguous()
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    out = torch.empty((G, P), dtype=torch.float32, device=dev)
    if G and P:
        _lib.check(_lib.lib().digat_qdot_scores(*_qdot_head(qu, su, qn, sn, pl, G, N, P, dq), out.data_ptr(), _lib.stream_ptr()),
                   "digat_qdot_scores")
    return out


def _qdot_select(qu, su, qn, sn, k, pool, skip, limit, slab_users):
    """``qdot_topk`` (``slab_users`` None) or ``qdot_shortlist``: ``_dot_select`` on codes."""
    import torch
    from . import _lib
    G, N, P, dq = _check_qdot_args(qu, su, qn, sn, pool, skip, k, limit)
    k = int(k)
    if qu.device.type != "cuda":
        host = lambda t: None if t is None else t.numpy()
        S = qdot_scores_host(qu.numpy(), su.numpy(), qn.numpy(), sn.numpy(), host(pool))
        sk = None if skip is None or skip.shape[1] == 0 else host(skip)
        return tuple(map(torch.from_numpy, dot_topk_host(S, k, pool=host(pool), skip=sk, limit=limit)))
    dev = _lib.require_device(*[t for t in (qu, su, qn, sn, pool, skip) if t is not None])
    qu, su, qn, sn = qu.contiguous(), su.contiguous(), qn.contiguous(), sn.contiguous()
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    sk = None if skip is None or skip.shape[1] == 0 else skip.to(torch.int64).contiguous()
    out_s = torch.full((G, k), float("-inf"), dtype=torch.float32, device=dev)
    out_i = torch.full((G, k), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((G,), dtype=torch.int32, device=dev)
    if G == 0 or P == 0:
        return out_s, out_i, count
    L = _lib.lib()
    head = _qdot_head(qu, su, qn, sn, pl, G, N, P, dq) + (_lib.ptr(sk), 0 if sk is None else int(sk.shape[1]), k)
    outs = (out_s.data_ptr(), out_i.data_ptr(), count.data_ptr())
    if slab_users is None:
        need = int(L.digat_qdot_topk_workspace_bytes(G, P, k))
        ws = _lib.workspace(need, dev, "dot_topk")
        _lib.check(L.digat_qdot_topk(*head, *outs, ws.data_ptr(), need, _lib.stream_ptr()), "digat_qdot_topk")
    else:
        need = int(L.digat_qdot_shortlist_workspace_bytes(G, P, k, slab_users))
        ws = _lib.workspace(need, dev, "dot_shortlist")
        _lib.check(L.digat_qdot_shortlist(*head, slab_users, *outs, ws.data_ptr(), need, _lib.stream_ptr()), "digat_qdot_shortlist")
    return out_s, out_i, count


def qdot_topk(qu, su, qn, sn, k: int, pool=None, skip=None):
    """``dot_topk`` on quantised scores (``digat_qdot_topk``): for every row of codes ``qu`` the k <= 128 best rows of ``qn`` by
    ``qdot_scores``' bits, in ``dot_topk``'s order, with its ``pool``, ``skip``, fill and returns ``(scores [G,k], ids [G,k],
    count [G])``; the [G, P] scores never reach memory.  On CPU tensors: ``dot_topk_host`` over ``qdot_scores_host``."""
    return _qdot_select(qu, su, qn, sn, k, pool, skip, _TOPK_LIMIT, None)


def qdot_shortlist(qu, su, qn, sn, m: int, pool=None, skip=None, slab_users=None):
    """``dot_shortlist`` on quantised scores (``digat_qdot_shortlist``): lists of up to ``SHORTLIST_MAX_K`` = 1024, the users walked
    in slabs of ``slab_users`` (None: 256) whose scores ``qdot_scores``' kernel stores; the results do not depend on the slab.  On
    CPU tensors: ``dot_shortlist_host`` over ``qdot_scores_host``."""
    slab = SHORTLIST_SLAB_USERS if slab_users is None else int(slab_users)
    if slab < 1:
        raise ValueError(f"slab_users must be positive, got {slab_users}")
    return _qdot_select(qu, su, qn, sn, m, pool, skip, _SHORTLIST_LIMIT, max(1, min(slab, int(qu.shape[0]))))


def refine_lists(users, rows, ids, count, k: int):
    """The second stage behind a quantised shortlist: the exact fp32 scores of given lists and their k <= 128 best —
    ``(scores [G,k] float32, ids [G,k] int64, count [G] int32)`` in selection order (score descending, ties by position IN THE LIST,
    NaNs last; ``-inf`` / ``-1`` at and beyond ``count``).  ``users`` [G, d], ``rows`` [N, d], ``ids`` [G, M] rows of ``rows`` and
    ``count`` [G] (None: M) — what ``qdot_shortlist`` returns; slot (g, j) is an element when ``j < count[g]`` and
    ``0 <= ids[g, j] < N``.  A caller who wants ties in pool order hands the lists over in pool order (``nrms.recommend`` does).

    On the device no new kernel: ``list_softmax``'s forward stores the lists' scores — ``dot_scores``' bits, M <= 1024 and d <= 512 —
    and ``topk_segments`` selects from them, the non-elements skipped as id -1.  On CPU tensors: a gather, ``(c * u).sum(1)`` as
    ``recommend``'s brute force scores its pairs, and ``topk_segments_host``."""
    import torch
    if ids.dim() != 2 or ids.shape[0] != users.shape[0]:
        raise ValueError(f"ids must be [G = {int(users.shape[0])}, M], got {tuple(ids.shape)}")
    k = _check_limit(k)
    G, M, N = int(ids.shape[0]), int(ids.shape[1]), int(rows.shape[0])
    dev = users.device
    ids = ids.to(torch.int64)
    cnt = None if count is None else torch.as_tensor(count).to(dev)
    elem = list_elements(ids, cnt, N)
    flat_ids = torch.where(elem, ids, torch.full_like(ids, -1)).reshape(-1).contiguous()
    seg = torch.arange(G + 1, dtype=torch.int64, device=dev) * M
    skip = torch.full((G, 1), -1, dtype=torch.int64, device=dev)
    if G == 0 or M == 0:
        return (torch.full((G, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((G, k), -1, dtype=torch.int64, device=dev),
                torch.zeros((G,), dtype=torch.int32, device=dev))
    if dev.type == "cuda":
        with torch.no_grad():
            S = list_softmax(users.detach(), rows.detach(), ids, cnt, torch.zeros((G, M), dtype=torch.float32, device=dev))[2]
        return topk_segments(S.reshape(-1), seg, k, ids=flat_ids, skip=skip)
    safe = torch.where(elem, ids, torch.zeros_like(ids)).reshape(-1)
    owner = torch.arange(G, dtype=torch.int64).repeat_interleave(M)
    with torch.no_grad():
        S = (rows.index_select(0, safe) * users.index_select(0, owner)).sum(dim=1).float()
    return tuple(map(torch.from_numpy, topk_segments_host(S.numpy(), seg.numpy(), k, ids=flat_ids.numpy(), skip=skip.numpy())))


def _check_target_start(target_start, users: int, targets: int) -> np.ndarray:
    """``target_start`` of the rank entries as a host int64 array: [users + 1] row offsets from 0 to ``targets`` that never decrease."""
    import torch
    st = np.asarray(target_start.cpu() if torch.is_tensor(target_start) else target_start)
    if st.ndim != 1 or st.shape[0] != users + 1 or st.dtype.kind not in "iu":
        raise ValueError(f"target_start must be a 1-D integer array of users + 1 = {users + 1} offsets, got shape {st.shape} {st.dtype}")
    st = st.astype(np.int64)
    if st[0] != 0 or np.any(np.diff(st) < 0) or int(st[-1]) != targets:
        raise ValueError(f"target_start must begin at 0, never decrease and end at the number of targets ({targets})")
    return st


def dot_rank_host(scores, target_pos, target_start, pool=None, skip=None, news_num=None):
    """The contract of ``digat_dot_rank`` on a given score matrix ``scores`` [G, P], in numpy — the yardstick of the kernel.  The
    elements of user g are ``dot_topk_host``'s: the pool positions whose id (``pool``; the position when None) is not in ``skip[g]``
    and lies in [0, ``news_num``) (None: no upper bound).  ``target_pos`` [T] holds pool positions, ``target_start`` [G + 1] gives
    every user its slice.  Returns ``rank`` [T] int32: the elements of the target's user that order before it — a larger key
    (``topk_keys``: NaNs last, ``-0.0 == +0.0``), or the same key at a smaller position — or -1 where the target is no element of
    its user."""
    S = np.ascontiguousarray(scores, dtype=np.float32)
    if S.ndim != 2:
        raise ValueError("scores must be [G, P]")
    G, P = S.shape
    pos = np.asarray(target_pos, dtype=np.int64)
    if pos.ndim != 1:
        raise ValueError("target_pos must be 1-D")
    st = _check_target_start(target_start, G, len(pos))
    ids = np.arange(P, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64)
    if ids.shape != (P,):
        raise ValueError(f"pool must have one id per column ({P}), got shape {ids.shape}")
    skv = None if skip is None else np.asarray(skip, dtype=np.int64).reshape(G, -1)
    if skv is not None and skv.shape[1] > TOPK_MAX_SKIP:
        raise ValueError(f"skip must be [users, at most {TOPK_MAX_SKIP}], got shape {skv.shape}")
    base = ids >= 0
    if news_num is not None:
        base &= ids < int(news_num)
    where = np.arange(P, dtype=np.int64)
    rank = np.full(len(pos), -1, dtype=np.int32)
    for g in range(G):
        a, b = int(st[g]), int(st[g + 1])
        if a == b:
            continue
        elem = base if skv is None or not skv.shape[1] else base & ~np.isin(ids, skv[g])
        keys = topk_keys(S[g]).astype(np.int64)
        q = pos[a:b]
        ok = (q >= 0) & (q < P)
        ok[ok] = elem[q[ok]]
        qs = q[ok]
        before = (keys[None, :] > keys[qs][:, None]) | ((keys[None, :] == keys[qs][:, None]) & (where[None, :] < qs[:, None]))
        out = rank[a:b]
        out[ok] = (before & elem[None, :]).sum(axis=1)
    return rank


def dot_rank(users, news, target_pos, target_start, pool=None, skip=None):
    """For every target — a pool position of one user — its rank in that user's whole ordered pool, on the GPU without the [G, P]
    score matrix (``digat_dot_rank``).  ``users`` [G, d], ``news`` [N, d], ``pool`` [P] and ``skip`` [G, L <= 256] are ``dot_topk``'s,
    and so are a user's elements and their order; ``target_pos`` [T] int64 (a device tensor or a host array) holds pool positions,
    ``target_start`` [G + 1] is a HOST array — checked here, then uploaded — that gives user g the targets
    ``[start[g], start[g+1])``: none, one or many, repeats allowed.  Returns ``(rank [T] int32, scores [T] float32)`` on the device:
    the number of the user's elements that order before the target, and the target's score with the bits ``dot_scores`` gives; -1
    and NaN where the target is no element of its user (a position outside [0, P), a skipped id).  The contract is
    ``dot_rank_host``'s on ``dot_scores``, exactly; ``rank < k`` holds exactly when ``dot_topk``'s list carries the element at slot
    ``rank``.  Stream-ordered; only the pool's id range is read back, for the check."""
    import torch
    from . import _lib
    given = [t for t in (users, news, pool, skip) if t is not None]
    dev = _lib.require_device(*given)
    G, N, P, d = _check_dot_args(users, news, pool, skip)
    tp = torch.as_tensor(np.asarray(target_pos) if not torch.is_tensor(target_pos) else target_pos)
    if tp.dim() != 1 or tp.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise ValueError("target_pos must be a 1-D integer array of pool positions")
    T = int(tp.shape[0])
    st = _check_target_start(target_start, G, T)
    u, v = _lib.f32(users.detach()), _lib.f32(news.detach())
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    sk = None if skip is None or skip.shape[1] == 0 else skip.to(torch.int64).contiguous()
    rank = torch.full((T,), -1, dtype=torch.int32, device=dev)
    scores = torch.full((T,), float("nan"), dtype=torch.float32, device=dev)
    if G == 0 or T == 0 or P == 0:                                  # an empty pool: nothing is an element
        return rank, scores
    tp = tp.to(dev, torch.int64).contiguous()
    std = torch.from_numpy(st).to(dev)
    L = _lib.lib()
    need = int(L.digat_dot_rank_workspace_bytes(G, P, T))
    ws = _lib.workspace(need, dev, "dot_rank")
    _lib.check(L.digat_dot_rank(u.data_ptr(), v.data_ptr(), _lib.ptr(pl), G, N, P, d, _lib.ptr(sk), 0 if sk is None else int(sk.shape[1]),
                                tp.data_ptr(), std.data_ptr(), T, rank.data_ptr(), scores.data_ptr(), ws.data_ptr(), need,
                                _lib.stream_ptr()),
               "digat_dot_rank")
    return rank, scores


def list_ranks(ids, count, target_ids, target_start):
    """The slot of every target id in its user's list: ``rank`` [T] int32, -1 where the list does not hold it (its first occurrence
    where it holds it twice).  ``ids`` [G, k] and ``count`` [G] (None: k) are what ``util.recommend`` / ``nrms.recommend`` return —
    slots at or beyond ``count`` are fill —, ``target_ids`` [T] news ids, ``target_start`` [G + 1] the users' slices.  Torch
    operations only, on the device of ``ids``: the way to hold a second stage (a re-rank, a diversified list) to ``rank_metrics``."""
    import torch
    ids = torch.as_tensor(ids)
    if ids.dim() != 2:
        raise ValueError(f"ids must be [G, k], got {tuple(ids.shape)}")
    G, k = int(ids.shape[0]), int(ids.shape[1])
    dev = ids.device
    tg = torch.as_tensor(np.asarray(target_ids) if not torch.is_tensor(target_ids) else target_ids).to(dev, torch.int64)
    if tg.dim() != 1:
        raise ValueError("target_ids must be 1-D")
    T = int(tg.shape[0])
    st = torch.from_numpy(_check_target_start(target_start, G, T)).to(dev)
    cnt = torch.full((G,), k, dtype=torch.int64, device=dev) if count is None else torch.as_tensor(count).to(dev, torch.int64)
    if tuple(cnt.shape) != (G,):
        raise ValueError(f"count must have one entry per list ({G}), got shape {tuple(cnt.shape)}")
    owner = torch.repeat_interleave(torch.arange(G, device=dev), st[1:] - st[:-1], output_size=T)
    slot = torch.arange(k, device=dev)
    hit = (ids.to(torch.int64).index_select(0, owner) == tg[:, None]) & (slot[None, :] < cnt.index_select(0, owner)[:, None])
    first = torch.where(hit, slot[None, :], torch.full_like(slot, k)[None, :]).amin(dim=1) if k else tg.new_zeros(T)
    return torch.where(first < k, first, torch.full_like(first, -1)).to(torch.int32)


def rank_metrics(rank, target_start, ks=(10, 50, 100, 128)):
    """Full-catalogue retrieval metrics of a rank array (``dot_rank``, ``dot_rank_host``, ``list_ranks``: 0-based, -1 = not ranked),
    in float64 on the host.  A dict with, for every k of ``ks`` (any positive k): ``recall@k`` — the targets with
    ``0 <= rank < k`` over ALL targets, an unranked one is a miss — and ``user_recall@k`` — the mean over the users with at least
    one target of their share of targets inside k —; ``mrr`` — the mean over those users of ``1 / (1 + their best rank)``, 0 for a
    user none of whose targets is ranked —; ``median_rank`` over the ranked targets; the counts ``not_ranked``, ``targets`` and
    ``users`` (those with a target).  What has nothing to average over is NaN."""
    import torch
    r = np.asarray(rank.cpu() if torch.is_tensor(rank) else rank).astype(np.int64)
    if r.ndim != 1:
        raise ValueError("rank must be 1-D")
    T = len(r)
    st = np.asarray(target_start.cpu() if torch.is_tensor(target_start) else target_start)
    if st.size == 0:
        st = np.zeros(1, dtype=np.int64)                            # nobody
    st = _check_target_start(st, len(st) - 1 if st.ndim == 1 else 0, T)
    per_user = np.diff(st)
    have = per_user > 0
    users = int(have.sum())
    ranked = r >= 0
    owner = np.repeat(np.arange(len(per_user)), per_user)
    nan = float("nan")
    out = {}
    for k in ks:
        if int(k) != k or k < 1:
            raise ValueError(f"every k must be a positive integer, got {k}")
        inside = ranked & (r < int(k))
        out[f"recall@{int(k)}"] = float(inside.sum()) / T if T else nan
        share = np.bincount(owner, weights=inside.astype(np.float64), minlength=len(per_user))[have] / per_user[have]
        out[f"user_recall@{int(k)}"] = float(share.mean()) if users else nan
    best = np.full(len(per_user), np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(best, owner[ranked], r[ranked])
    best = best[have]
    found = best != np.iinfo(np.int64).max
    out["mrr"] = float(np.where(found, 1.0 / (1.0 + np.where(found, best, 0).astype(np.float64)), 0.0).mean()) if users else nan
    out["median_rank"] = float(np.median(r[ranked])) if ranked.any() else nan
    out["not_ranked"], out["targets"], out["users"] = int(T - ranked.sum()), T, users
    return out


def shortlist_for(rank, share: float):
    """The smallest shortlist length k with ``recall@k >= share`` for a rank array (``rank_metrics``' recall: over all targets, an
    unranked one is a miss), or None when no k reaches it — too many targets are unranked, or there is no target."""
    import torch
    r = np.asarray(rank.cpu() if torch.is_tensor(rank) else rank).astype(np.int64)
    T = len(r)
    if not 0.0 <= float(share) <= 1.0:
        raise ValueError(f"share must lie in [0, 1], got {share}")
    if T == 0:
        return None
    m = int(np.ceil(float(share) * T))                              # the targets that must be inside: the smallest m with m / T >= share
    while m > 0 and (m - 1) / T >= share:
        m -= 1
    while m / T < share:
        m += 1
    got = np.sort(r[r >= 0])
    if m > len(got):
        return None
    return 1 if m == 0 else int(got[m - 1]) + 1


POOL_SOFTMAX_MAX_D = 512      # csrc/digat_pool_softmax.inc: PSM_MAX_D, the widest vectors digat_pool_softmax_bwd takes


def _pool_softmax_host_args(scores, target_pos, target_start, pool, skip, news_num):
    """The checks of ``dot_rank_host`` and its element rule: ``(S float64 [G,P], pos, start, elements bool [G,P], ranked bool [T],
    owner [T])``."""
    S = np.ascontiguousarray(scores, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("scores must be [G, P]")
    G, P = S.shape
    pos = np.asarray(target_pos, dtype=np.int64)
    if pos.ndim != 1:
        raise ValueError("target_pos must be 1-D")
    st = _check_target_start(target_start, G, len(pos))
    ids = np.arange(P, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64)
    if ids.shape != (P,):
        raise ValueError(f"pool must have one id per column ({P}), got shape {ids.shape}")
    skv = None if skip is None else np.asarray(skip, dtype=np.int64).reshape(G, -1)
    if skv is not None and skv.shape[1] > TOPK_MAX_SKIP:
        raise ValueError(f"skip must be [users, at most {TOPK_MAX_SKIP}], got shape {skv.shape}")
    base = ids >= 0
    if news_num is not None:
        base &= ids < int(news_num)
    elem = np.repeat(base[None, :], G, axis=0)
    if skv is not None and skv.shape[1]:
        for g in range(G):
            elem[g] &= ~np.isin(ids, skv[g])
    owner = np.repeat(np.arange(G), np.diff(st))
    ranked = (pos >= 0) & (pos < P)
    ranked[ranked] = elem[owner[ranked], pos[ranked]]
    return S, pos, st, elem, ranked, owner


def pool_softmax_host(scores, target_pos, target_start, pool=None, skip=None, news_num=None, scale=1.0):
    """The contract of ``digat_pool_softmax_fwd`` on a given score matrix ``scores`` [G, P], in numpy float64 — the yardstick of the
    kernel.  The elements of user g are ``dot_rank_host``'s.  With ``x = scale * scores``: ``lse`` [G] = log of the sum of ``exp(x)``
    over the user's elements (-inf without one); ``loss`` [T] = ``lse[user] - x[user, target]`` where the target is an element of its
    user, 0 elsewhere; ``ranked`` [T] bool says where.  Returns ``(loss, lse, ranked)``."""
    S, pos, st, elem, ranked, owner = _pool_softmax_host_args(scores, target_pos, target_start, pool, skip, news_num)
    G = S.shape[0]
    x = np.where(elem, float(scale) * S, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=1) if x.shape[1] else np.full(G, -np.inf)
        safe = np.where(np.isfinite(m), m, 0.0)
        lse = safe + np.log(np.exp(x - safe[:, None]).sum(axis=1))
    loss = np.zeros(len(pos), dtype=np.float64)
    loss[ranked] = lse[owner[ranked]] - x[owner[ranked], pos[ranked]]
    return loss, lse, ranked


def pool_softmax_grad_host(users, rows, scores, target_pos, target_start, pool=None, skip=None, news_num=None, scale=1.0, grad_loss=None):
    """The contract of ``digat_pool_softmax_bwd`` in numpy float64: ``users`` [G, d], ``rows`` [P, d] — the news row of every pool
    POSITION (zeros where the id is no row) —, ``scores`` [G, P] the matrix the loss was taken on, ``grad_loss`` [T] (None: ones;
    ignored where the target is not ranked).  Returns ``(d_users [G, d], d_rows [P, d])``, the gradients of ``sum(grad_loss * loss)``
    with the scores' dependence on ``users`` and ``rows`` being the inner product."""
    S, pos, st, elem, ranked, owner = _pool_softmax_host_args(scores, target_pos, target_start, pool, skip, news_num)
    _, lse, _ = pool_softmax_host(scores, target_pos, target_start, pool, skip, news_num, scale)
    U, R = np.asarray(users, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    G, P = S.shape
    if U.ndim != 2 or R.ndim != 2 or U.shape[0] != G or R.shape[0] != P or U.shape[1] != R.shape[1]:
        raise ValueError(f"users must be [{G}, d] and rows [{P}, d], got {U.shape} and {R.shape}")
    gl = np.ones(len(pos)) if grad_loss is None else np.asarray(grad_loss, dtype=np.float64)
    if gl.shape != pos.shape:
        raise ValueError("grad_loss must have one entry per target")
    gl = np.where(ranked, gl, 0.0)
    c = np.bincount(owner, weights=gl, minlength=G) if len(pos) else np.zeros(G)
    C = np.zeros((G, P), dtype=np.float64)
    live = c != 0
    with np.errstate(invalid="ignore", over="ignore"):
        C[live] = np.where(elem[live], c[live, None] * np.exp(float(scale) * S[live] - lse[live, None]), 0.0)
    np.subtract.at(C, (owner[ranked], pos[ranked]), gl[ranked])
    return float(scale) * (C @ R), float(scale) * (C.T @ U)


def pool_softmax_bound(P, lse, x_max, x_target=None, loss=None):
    """The error bound csrc/digat_pool_softmax.inc derives for ``lse`` (and, with ``x_target`` and ``loss``, for ``loss``) against an
    exact evaluation on the same fp32 scores: ``u (15 + ceil(C / 64) + log n + 4 |lse| + 2 max|x|)`` with u = 2^-24, n <= P elements
    and C chunks, plus ``u (|x_target| + |loss|)`` for a loss."""
    u = 2.0 ** -24
    chunks = -(-int(P) // DOT_TOPK_CHUNK)
    b = u * (15.0 + -(-chunks // 64) + np.log(max(int(P), 1)) + 4.0 * np.abs(lse) + 2.0 * np.abs(x_max))
    if x_target is not None:
        b = b + u * (np.abs(x_target) + np.abs(loss))
    return b


def _pool_softmax_args(users, news, target_pos, target_start, pool, skip):
    """``dot_rank``'s checks: ``(G, N, P, d, target_pos as a tensor, target_start as a host array)``."""
    import torch
    G, N, P, d = _check_dot_args(users, news, pool, skip)
    tp = torch.as_tensor(np.asarray(target_pos) if not torch.is_tensor(target_pos) else target_pos)
    if tp.dim() != 1 or tp.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise ValueError("target_pos must be a 1-D integer array of pool positions")
    st = _check_target_start(target_start, G, int(tp.shape[0]))
    return G, N, P, d, tp, st


def _pool_softmax_call(entry, u, v, pl, sk, tp, std, scale, tail):
    """One of the two entries: the shared head of the argument list, the workspace and the call."""
    from . import _lib
    L = _lib.lib()
    G, d = int(u.shape[0]), int(u.shape[1])
    N, P, T = int(v.shape[0]), int(v.shape[0] if pl is None else pl.shape[0]), int(tp.shape[0])
    need = int(L.digat_pool_softmax_workspace_bytes(G, P, T, d))
    ws = _lib.workspace(need, u.device, "pool_softmax")
    _lib.check(getattr(L, entry)(u.data_ptr(), v.data_ptr(), _lib.ptr(pl), G, N, P, d, _lib.ptr(sk), 0 if sk is None else int(sk.shape[1]),
                                 tp.data_ptr() if T else ws.data_ptr(), std.data_ptr(), T, float(scale), *tail, ws.data_ptr(), need,
                                 _lib.stream_ptr()), entry)


def _pool_softmax_function():
    import torch

    class PoolSoftmax(torch.autograd.Function):
        """``digat_pool_softmax_fwd`` / ``digat_pool_softmax_bwd``: the gradient of ``news`` [N, d] is the ``index_add_`` of the
        per-position rows the library writes."""

        @staticmethod
        def forward(ctx, users, news, pl, sk, tp, std, scale):
            u, v = users.detach().float().contiguous(), news.detach().float().contiguous()
            G, T = int(u.shape[0]), int(tp.shape[0])
            f = dict(dtype=torch.float32, device=u.device)
            per_target, lse = torch.empty((2, max(T, 1)), **f), torch.empty(G, **f)          # no target: still two pointers to hand over
            loss, score = per_target[0, :T], per_target[1, :T]
            _pool_softmax_call("digat_pool_softmax_fwd", u, v, pl, sk, tp, std, scale,
                               (per_target[0].data_ptr(), lse.data_ptr(), per_target[1].data_ptr()))
            ctx.save_for_backward(u, v, lse, tp, std)
            ctx.pl, ctx.sk, ctx.scale, ctx.dtypes = pl, sk, scale, (users.dtype, news.dtype)
            ctx.mark_non_differentiable(lse, score)
            return loss, lse, score

        @staticmethod
        def backward(ctx, grad_loss, _lse, _score):
            u, v, lse, tp, std = ctx.saved_tensors
            pl, sk = ctx.pl, ctx.sk
            G, d, N = int(u.shape[0]), int(u.shape[1]), int(v.shape[0])
            P = N if pl is None else int(pl.shape[0])
            if d > POOL_SOFTMAX_MAX_D:
                raise ValueError(f"the backward of pool_softmax takes vectors of at most {POOL_SOFTMAX_MAX_D} channels, got {d}")
            f = dict(dtype=torch.float32, device=u.device)
            d_users, d_rows = torch.empty((G, d), **f), torch.empty((P, d), **f)
            gl = grad_loss.float().contiguous()
            _pool_softmax_call("digat_pool_softmax_bwd", u, v, pl, sk, tp, std, ctx.scale,
                               (lse.data_ptr(), gl.data_ptr() if gl.numel() else lse.data_ptr(), d_users.data_ptr(), d_rows.data_ptr()))
            d_news = None
            if ctx.needs_input_grad[1]:
                d_news = d_rows if pl is None else torch.zeros((N, d), **f).index_add_(0, pl, d_rows)
            return (d_users.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None), (None if d_news is None else d_news.to(ctx.dtypes[1])), \
                None, None, None, None, None

    return PoolSoftmax


_PoolSoftmax = None


def pool_softmax(users, news, target_pos, target_start, pool=None, skip=None, scale=1.0):
    """The softmax loss of every target — a pool position of one user — over that user's WHOLE pool: ``(loss [T], lse [G],
    target_score [T])`` float32.  ``users`` [G, d], ``news`` [N, d], ``pool`` [P], ``skip`` [G, L <= 256], ``target_pos`` [T] and the
    HOST array ``target_start`` [G + 1] are ``dot_rank``'s, and so are a user's elements.  With ``x = scale * <user, news>``:
    ``lse`` = log-sum-exp of x over the user's elements (-inf without one), ``loss = lse - x[target]``; a target that is no element of
    its user (``dot_rank``'s -1) has loss 0 and a NaN ``target_score``.  ``loss`` is differentiable in ``users`` and ``news``; ``lse``
    and ``target_score`` are not.

    On CUDA tensors: ``digat_pool_softmax_fwd`` / ``_bwd`` under autograd — no [G, P] scores, softmax or score gradient in memory;
    the backward takes ``d <= POOL_SOFTMAX_MAX_D`` = 512 and raises ``ValueError`` beyond.  Two calls give the same bits, the gradient of
    ``news`` included as long as ``pool`` repeats no id (repeated ids are summed by ``index_add_``, whose order torch does not fix).
    On CPU tensors: the stock composition —
    product, masked ``logsumexp``, gather — differentiable by autograd."""
    import torch
    global _PoolSoftmax
    G, N, P, d, tp, st = _pool_softmax_args(users, news, target_pos, target_start, pool, skip)
    dev = users.device
    given = [t for t in (news, pool, skip) if t is not None]
    if any(t.device != dev for t in given):
        raise ValueError("users, news, pool and skip must live on one device")
    pl = None if pool is None else pool.to(torch.int64).contiguous()
    sk = None if skip is None or skip.shape[1] == 0 else skip.to(torch.int64).contiguous()
    tp = tp.to(dev, torch.int64).contiguous()
    T = int(tp.shape[0])
    if dev.type == "cuda":
        if _PoolSoftmax is None:
            _PoolSoftmax = _pool_softmax_function()
        if G == 0 or P == 0:                                          # nothing is an element: no launch, a zero gradient
            z = users.new_zeros(T, dtype=torch.float32) + 0.0 * (users.float().sum() + news.float().sum())
            return z, users.new_full((G,), float("-inf"), dtype=torch.float32), users.new_full((T,), float("nan"), dtype=torch.float32)
        return _PoolSoftmax.apply(users, news, pl, sk, tp, torch.from_numpy(st).to(dev), float(scale))
    ids = torch.arange(P) if pl is None else pl
    S = users @ news.index_select(0, ids).t()                                        # [G, P]
    x = float(scale) * S
    elem = torch.ones((G, P), dtype=torch.bool)
    if sk is not None:
        elem &= ~(ids[None, :, None] == sk[:, None, :]).any(dim=2)
    has = elem.any(dim=1)                                                            # a row without an element never meets logsumexp
    masked = torch.where(has[:, None], x.masked_fill(~elem, float("-inf")), torch.zeros_like(x))
    lse = torch.where(has, torch.logsumexp(masked, dim=1), x.new_full((G,), float("-inf"))) if P else x.new_full((G,), float("-inf"))
    owner = torch.from_numpy(np.repeat(np.arange(G), np.diff(st)))
    inside = (tp >= 0) & (tp < P)
    at = torch.where(inside, tp, torch.zeros_like(tp))
    if P and T:
        ranked = inside & elem[owner, at]
        loss = torch.where(ranked, torch.where(ranked, lse[owner], torch.zeros_like(lse[owner])) - x[owner, at], x.new_zeros(T))
        score = torch.where(ranked, S.detach()[owner, at], S.new_full((T,), float("nan")))
    else:
        loss = x.new_zeros(T) + 0.0 * x.sum()
        score = S.new_full((T,), float("nan"))
    return loss, lse.detach(), score


LIST_SOFTMAX_MAX_D = 512      # include/digat_hip.h: DIGAT_LIST_SOFTMAX_MAX_D, the widest vectors digat_list_softmax_fwd / _bwd take


def _list_softmax_host_args(scores, ids, count, teacher, rows_num):
    """The element rule of ``digat_list_softmax_fwd`` in numpy: ``(S float64 [G,M], ids int64 [G,M], teacher float64 [G,M], elements
    bool [G,M], mass bool [G,M])``."""
    S = np.ascontiguousarray(scores, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("scores must be [G, M]")
    G, M = S.shape
    I = np.asarray(ids)
    if I.shape != (G, M) or I.dtype.kind not in "iu":
        raise ValueError(f"ids must be an integer array of shape {(G, M)}, got {I.shape} {I.dtype}")
    I = I.astype(np.int64)
    Tt = np.asarray(teacher, dtype=np.float64)
    if Tt.shape != (G, M):
        raise ValueError(f"teacher must have one value per slot {(G, M)}, got shape {Tt.shape}")
    cnt = np.full(G, M, dtype=np.int64) if count is None else np.asarray(count).astype(np.int64)
    if cnt.shape != (G,):
        raise ValueError(f"count must have one entry per list ({G}), got shape {cnt.shape}")
    elem = (np.arange(M)[None, :] < np.clip(cnt, 0, M)[:, None]) & (I >= 0) & (I < int(rows_num))
    return S, I, Tt, elem, elem & np.isfinite(Tt)


def _masked_lse_host(v, mask):
    """log of the sum of exp(v) over ``mask`` per row, the maximum subtracted; -inf for a row without a True."""
    w = np.where(mask, v, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = w.max(axis=1) if w.shape[1] else np.full(w.shape[0], -np.inf)
        safe = np.where(np.isfinite(m), m, 0.0)
        return safe + np.log(np.exp(w - safe[:, None]).sum(axis=1))


def _list_softmax_host_parts(scores, ids, count, teacher, rows_num, scale, temperature):
    if not float(temperature) > 0.0:
        raise ValueError(f"temperature must be positive, got {temperature}")
    S, I, Tt, elem, mass = _list_softmax_host_args(scores, ids, count, teacher, rows_num)
    x = float(scale) * S
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tau = np.where(mass, Tt, 0.0) / float(temperature)
    lse_x, lse_t = _masked_lse_host(x, elem), _masked_lse_host(tau, mass)
    valid = elem.any(axis=1) & mass.any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where(mass & valid[:, None], np.exp(np.where(mass, tau, 0.0) - np.where(valid, lse_t, 0.0)[:, None]), 0.0)
        p = np.where(elem & valid[:, None], np.exp(np.where(elem, x, 0.0) - np.where(valid, lse_x, 0.0)[:, None]), 0.0)
    return S, I, elem, mass, x, tau, lse_x, lse_t, valid, p, q


def list_softmax_host(scores, ids, count, teacher, rows_num, scale=1.0, temperature=1.0):
    """The contract of ``digat_list_softmax_fwd`` on given scores ``scores`` [G, M] (slot (g, j) holds the inner product of user g
    with row ``ids[g, j]``), in numpy float64 — the yardstick of the kernel.  Slot (g, j) is an element when
    ``j < clip(count[g], 0, M)`` (``count`` None: M) and ``0 <= ids[g, j] < rows_num``; a repeated id is two elements.  With
    ``x = scale * scores`` and ``tau = teacher / temperature`` where the element's teacher value is finite (any other element has no
    target mass): ``lse`` [G] = log-sum-exp of x over the elements (-inf without one), ``loss`` [G] = KL(softmax(tau) over the elements
    with mass || softmax(x) over the elements) = ``lse_x - lse_tau + sum_j q_j (tau_j - x_j)``; ``valid`` [G] bool says where the list
    has an element and an element with mass — loss is 0 elsewhere.  Returns ``(loss, lse, valid)``."""
    S, I, elem, mass, x, tau, lse_x, lse_t, valid, p, q = _list_softmax_host_parts(scores, ids, count, teacher, rows_num, scale, temperature)
    with np.errstate(invalid="ignore"):
        cross = np.where(q > 0, q * (np.where(mass, tau, 0.0) - np.where(mass, x, 0.0)), 0.0).sum(axis=1)
        loss = np.where(valid, np.where(valid, lse_x, 0.0) - np.where(valid, lse_t, 0.0) + cross, 0.0)
    return loss, lse_x, valid


def list_softmax_grad_host(users, rows, scores, ids, count, teacher, scale=1.0, temperature=1.0, grad_loss=None):
    """The contract of ``digat_list_softmax_bwd`` in numpy float64: ``users`` [G, d], ``rows`` [P, d], ``scores`` [G, M] the scores the
    loss was taken on, ``grad_loss`` [G] (None: ones).  With ``coef = grad_loss scale (p - q)`` on the elements of valid lists and 0
    elsewhere: ``d_users[g] = sum_j coef[g, j] rows[ids[g, j]]`` and ``d_rows[p]`` = the sum of ``coef[g, j] users[g]`` over the
    elements with ``ids[g, j] == p``.  Returns ``(d_users [G, d], d_rows [P, d])``."""
    U, R = np.asarray(users, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    if U.ndim != 2 or R.ndim != 2 or U.shape[1] != R.shape[1]:
        raise ValueError(f"users [G, d] and rows [P, d] must share d, got {U.shape} and {R.shape}")
    S, I, elem, mass, x, tau, lse_x, lse_t, valid, p, q = _list_softmax_host_parts(scores, ids, count, teacher, R.shape[0], scale,
                                                                                    temperature)
    G = S.shape[0]
    if U.shape[0] != G:
        raise ValueError(f"users must have one row per list ({G}), got {U.shape}")
    gl = np.ones(G) if grad_loss is None else np.asarray(grad_loss, dtype=np.float64)
    if gl.shape != (G,):
        raise ValueError("grad_loss must have one entry per list")
    coef = np.where(elem & valid[:, None], gl[:, None] * float(scale) * (p - q), 0.0)
    g_of, j_of = np.nonzero(elem)
    d_users, d_rows = np.zeros_like(U), np.zeros_like(R)
    np.add.at(d_users, g_of, coef[g_of, j_of][:, None] * R[I[g_of, j_of]])
    np.add.at(d_rows, I[g_of, j_of], coef[g_of, j_of][:, None] * U[g_of])
    return d_users, d_rows


def list_softmax_keys_host(ids, count, rows_num):
    """``entry_keys`` of ``digat_list_softmax_bwd`` in numpy: the sorted int64 values ``ids[g, j] * (G M) + (g M + j)`` of all elements."""
    I = np.asarray(ids)
    if I.ndim != 2:
        raise ValueError("ids must be [G, M]")
    G, M = I.shape
    _, I, _, elem, _ = _list_softmax_host_args(np.zeros((G, M)), I, count, np.zeros((G, M)), rows_num)
    flat = np.arange(G * M, dtype=np.int64).reshape(G, M)
    return np.sort(I[elem] * np.int64(G * M) + flat[elem])


def list_softmax_bound(lse, x_max, tau_max=0.0, loss=None):
    """The error bound csrc/digat_list_softmax.inc derives against an exact evaluation on the same fp32 scores, with ``scale`` and
    ``temperature`` the float32 numbers the entry receives: for ``lse`` (``loss`` None) ``u (max|x| + |lse|) + e64``, for ``loss``
    ``u (max|x| min(2, sqrt(2 loss)) + |loss|) + 2 e64``, with u = 2^-24 and ``e64 = 2^-40 (1 + max|x| + max|tau|)``."""
    u = 2.0 ** -24
    e64 = 2.0 ** -40 * (1.0 + np.abs(x_max) + np.abs(tau_max))
    if loss is None:
        return u * (np.abs(x_max) + np.abs(lse)) + e64
    return u * (np.abs(x_max) * np.minimum(2.0, np.sqrt(2.0 * np.abs(loss))) + np.abs(loss)) + 2.0 * e64


def _check_list_args(users, rows, ids, count, name="list_softmax"):
    """The list checks every per-list entry shares (``list_softmax``, ``list_pl``): ``(G, P, M, d)``."""
    import torch
    if users.dim() != 2 or rows.dim() != 2 or users.shape[1] != rows.shape[1] or users.shape[1] < 1:
        raise ValueError(f"users [G, d] and rows [P, d] must share d >= 1, got {tuple(users.shape)} and {tuple(rows.shape)}")
    G, d, P = int(users.shape[0]), int(users.shape[1]), int(rows.shape[0])
    if d > LIST_SOFTMAX_MAX_D:
        raise ValueError(f"{name} takes vectors of at most LIST_SOFTMAX_MAX_D = {LIST_SOFTMAX_MAX_D} channels, got {d}")
    if ids.dim() != 2 or ids.shape[0] != G or ids.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise ValueError(f"ids must be an integer tensor [G = {G}, M], got {tuple(ids.shape)} {ids.dtype}")
    M = int(ids.shape[1])
    if not 1 <= M <= SHORTLIST_MAX_K:
        raise ValueError(f"a list holds between 1 and SHORTLIST_MAX_K = {SHORTLIST_MAX_K} slots, got M = {M}")
    if G * M >= 1 << 31:
        raise ValueError(f"G x M must stay below 2^31, got {G} x {M}")
    if count is not None and (tuple(count.shape) != (G,) or count.dtype in (torch.float16, torch.float32, torch.float64, torch.bool)):
        raise ValueError(f"count must be an integer tensor with one entry per list ({G}), got {tuple(count.shape)} {count.dtype}")
    return G, P, M, d


def _check_list_softmax_args(users, rows, ids, count, teacher, temperature):
    G, P, M, d = _check_list_args(users, rows, ids, count)
    if tuple(teacher.shape) != (G, M) or not teacher.is_floating_point():
        raise ValueError(f"teacher must be a floating-point tensor with one value per slot {(G, M)}, got {tuple(teacher.shape)} {teacher.dtype}")
    if not float(temperature) > 0.0 or float(temperature) == float("inf"):
        raise ValueError(f"temperature must be a positive finite number, got {temperature}")
    return G, P, M, d


def list_elements(ids, count, rows_num: int):
    """bool [G, M]: the slots of ``ids`` that are elements — ``j < clip(count[g], 0, M)`` and ``0 <= ids[g, j] < rows_num``."""
    import torch
    G, M = int(ids.shape[0]), int(ids.shape[1])
    slot = torch.arange(M, device=ids.device)
    inside = (ids >= 0) & (ids < int(rows_num))
    if count is None:
        return inside
    return inside & (slot[None, :] < count.to(ids.device, torch.int64).clamp(0, M)[:, None])


def _list_softmax_function():
    import torch
    from . import _lib

    def head(u, v, ids, cnt, teacher, scale, temperature):
        G, d = int(u.shape[0]), int(u.shape[1])
        return (u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(cnt), teacher.data_ptr(), G, int(v.shape[0]), int(ids.shape[1]), d,
                float(scale), float(temperature))

    class ListSoftmax(torch.autograd.Function):
        """``digat_list_softmax_fwd`` / ``digat_list_softmax_bwd``; the sorted entry keys of the rows kernel are built here, in the
        forward: the ids carry no gradient."""

        @staticmethod
        def forward(ctx, users, rows, ids, cnt, teacher, scale, temperature):
            u, v = users.detach().float().contiguous(), rows.detach().float().contiguous()
            G, M, P = int(u.shape[0]), int(ids.shape[1]), int(v.shape[0])
            f = dict(dtype=torch.float32, device=u.device)
            per_list, scores = torch.empty((2, G), **f), torch.empty((G, M), **f)
            valid = torch.empty(G, dtype=torch.int32, device=u.device)
            _lib.check(_lib.lib().digat_list_softmax_fwd(*head(u, v, ids, cnt, teacher, scale, temperature), per_list[0].data_ptr(),
                                                         per_list[1].data_ptr(), valid.data_ptr(), scores.data_ptr(), _lib.stream_ptr()),
                       "digat_list_softmax_fwd")
            keys = None
            if ctx.needs_input_grad[1]:
                elem = list_elements(ids, cnt, P).view(-1)
                flat = torch.arange(G * M, device=u.device)
                keys = torch.sort(ids.view(-1)[elem] * (G * M) + flat[elem]).values.contiguous()
            loss, lse = per_list[0], per_list[1]
            ctx.save_for_backward(u, v, ids, teacher, lse, scores)
            ctx.cnt, ctx.keys, ctx.scale, ctx.temperature, ctx.dtypes = cnt, keys, scale, temperature, (users.dtype, rows.dtype)
            ctx.mark_non_differentiable(lse, scores)
            return loss, lse, scores

        @staticmethod
        def backward(ctx, grad_loss, _lse, _scores):
            u, v, ids, teacher, lse, scores = ctx.saved_tensors
            G, d, P, M = int(u.shape[0]), int(u.shape[1]), int(v.shape[0]), int(ids.shape[1])
            f = dict(dtype=torch.float32, device=u.device)
            want_rows = ctx.needs_input_grad[1] and ctx.keys is not None
            d_users = torch.empty((G, d), **f)
            d_rows = torch.empty((P, d), **f) if want_rows else None
            gl = grad_loss.float().contiguous()
            L = _lib.lib()
            need = int(L.digat_list_softmax_workspace_bytes(G, M))
            ws = _lib.workspace(need, u.device, "list_softmax")
            keys = ctx.keys if want_rows else None
            _lib.check(L.digat_list_softmax_bwd(*head(u, v, ids, ctx.cnt, teacher, ctx.scale, ctx.temperature), lse.data_ptr(),
                                                scores.data_ptr(), gl.data_ptr(), _lib.ptr(keys) if keys is not None and keys.numel() else None,
                                                0 if keys is None else int(keys.numel()), d_users.data_ptr(), _lib.ptr(d_rows), ws.data_ptr(),
                                                need, _lib.stream_ptr()), "digat_list_softmax_bwd")
            return (d_users.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None), (None if d_rows is None else d_rows.to(ctx.dtypes[1])), \
                None, None, None, None, None

    return ListSoftmax


_ListSoftmax = None


def list_softmax(users, rows, ids, count, teacher, scale=1.0, temperature=1.0):
    """The softmax of every user's OWN list held against a target distribution given as scores: ``(loss [G], lse [G], scores [G, M])``.
    ``users`` [G, d], ``rows`` [P, d], ``ids`` [G, M] integer rows of ``rows`` and ``count`` [G] (None: M) — what ``util.recommend`` /
    ``nrms.shortlist`` return —, ``teacher`` [G, M].  Slot (g, j) is an element when ``j < clip(count[g], 0, M)`` and
    ``0 <= ids[g, j] < P``; a repeated id is two elements.  With ``x = scale * <users[g], rows[ids[g, j]]>`` and
    ``tau = teacher / temperature`` where the element's teacher value is finite (``-inf``, ``+inf`` and NaN mean "no target mass": the
    ``-inf`` fill of ``recommend`` and a one-hot click target go through unchanged): ``lse`` = log-sum-exp of x over the elements (-inf
    without one), ``loss`` = KL(softmax(tau) over the elements with mass || softmax(x) over the elements) — 0 for a list without an
    element or without mass —, ``scores`` = the inner products at elements, NaN elsewhere.  ``loss`` is differentiable in ``users`` and
    ``rows``; ``lse`` and ``scores`` are not, and ``teacher`` gets no gradient.  M <= ``SHORTLIST_MAX_K`` = 1024,
    d <= ``LIST_SOFTMAX_MAX_D`` = 512, G M < 2^31.

    On CUDA tensors: ``digat_list_softmax_fwd`` / ``_bwd`` under autograd — no [G, M, d] gather in memory, no float atomics: two calls
    give the same bits in every output and gradient; float32 outputs, the score bits are ``dot_scores``'.  On CPU tensors: the stock
    composition — ``index_select``, ``bmm``, ``log_softmax``, KL — in the dtype of ``users``, differentiable by autograd."""
    import torch
    global _ListSoftmax
    cnt = None if count is None else torch.as_tensor(count)
    G, P, M, d = _check_list_softmax_args(users, rows, ids, cnt, teacher, temperature)
    dev = users.device
    if any(t.device != dev for t in (rows, ids, teacher) + (() if cnt is None else (cnt,))):
        raise ValueError("users, rows, ids, count and teacher must live on one device")
    ids = ids.to(torch.int64).contiguous()
    teacher = teacher.detach()
    if dev.type == "cuda":
        if _ListSoftmax is None:
            _ListSoftmax = _list_softmax_function()
        if G == 0 or P == 0:                                          # nothing is an element: no launch, a zero gradient
            z = users.new_zeros(G, dtype=torch.float32) + 0.0 * (users.float().sum() + rows.float().sum())
            return z, users.new_full((G,), float("-inf"), dtype=torch.float32), users.new_full((G, M), float("nan"), dtype=torch.float32)
        return _ListSoftmax.apply(users, rows, ids, None if cnt is None else cnt.to(torch.int32).contiguous(),
                                  teacher.float().contiguous(), float(scale), float(temperature))
    elem = list_elements(ids, cnt, P)
    mass = elem & torch.isfinite(teacher)
    gathered = rows.index_select(0, torch.where(elem, ids, torch.zeros_like(ids)).view(-1)).view(G, M, d)        # [G, M, d]
    S = torch.bmm(gathered, users.unsqueeze(2)).squeeze(2)
    x = float(scale) * S
    neg = float("-inf")
    has, hm = elem.any(dim=1), mass.any(dim=1)
    xm = torch.where(has[:, None], x.masked_fill(~elem, neg), torch.zeros_like(x))          # a row without an element never meets the softmax
    tau = (torch.where(mass, teacher, torch.zeros_like(teacher)).to(x.dtype) / float(temperature)).masked_fill(~mass, neg)
    tm = torch.where(hm[:, None], tau, torch.zeros_like(tau))
    logp, logq = torch.log_softmax(xm, dim=1), torch.log_softmax(tm, dim=1)
    keep = mass & (has & hm)[:, None]
    zero = torch.zeros_like(x)
    loss = (torch.where(keep, logq.exp(), zero) * (torch.where(keep, logq, zero) - torch.where(keep, logp, zero))).sum(dim=1)
    lse = torch.where(has, torch.logsumexp(xm, dim=1), x.new_full((G,), neg)).detach()
    return loss, lse, torch.where(elem, S.detach(), S.new_full((G, M), float("nan")))


# ---- pairwise nDCG loss (LambdaRank) over a user's own list: csrc/digat_list_pairwise.inc ---------------------------------------
def ndcg_discount(M: int, k: int = 0) -> np.ndarray:
    """The nDCG discount table ``D(r) = 1 / log2(2 + r)`` for the 0-based ranks ``r < M``, float64 numpy [M] — zero from rank ``k`` on
    when ``k > 0`` (nDCG@k).  Built on the host, once: the kernels and the numpy twin read the same bits."""
    M, k = int(M), int(k)
    if M < 0 or k < 0:
        raise ValueError(f"M and k must not be negative, got {M} and {k}")
    D = 1.0 / np.log2(2.0 + np.arange(M, dtype=np.float64))
    if k > 0:
        D[k:] = 0.0
    return D


def _check_discount(discount, M: int) -> np.ndarray:
    """``discount`` (None: ``ndcg_discount(M)``) as a contiguous float64 numpy [M] table: finite, non-negative, non-increasing."""
    if discount is None:
        return ndcg_discount(M)
    D = discount.cpu().numpy() if _is_tensor(discount) else np.asarray(discount)
    if D.dtype != np.float64:
        raise ValueError(f"discount must be a float64 table (ndcg_discount builds one), got {D.dtype}")
    if D.shape != (M,):
        raise ValueError(f"discount must hold one value per rank ({M}), got shape {D.shape}")
    if not np.isfinite(D).all() or (D < 0).any() or (np.diff(D) > 0).any():
        raise ValueError("discount must be finite, non-negative and non-increasing")
    return np.ascontiguousarray(D)


def _list_pairwise_host_parts(scores, ids, count, gain, rows_num, scale, discount):
    import math
    S = np.asarray(scores)
    if S.ndim != 2:
        raise ValueError("scores must be [G, M]")
    G, M = S.shape
    S32 = np.ascontiguousarray(S, dtype=np.float32)
    gn = np.asarray(gain)
    if gn.shape != (G, M) or gn.dtype.kind != "f":
        raise ValueError(f"gain must be a floating-point array with one value per slot {(G, M)}, got {gn.shape} {gn.dtype}")
    gn = gn.astype(np.float32)
    D = _check_discount(discount, M)
    cnt = np.full(G, M, dtype=np.int64) if count is None else np.asarray(count).astype(np.int64)
    if cnt.shape != (G,):
        raise ValueError(f"count must have one entry per list ({G}), got shape {cnt.shape}")
    elem = np.arange(M)[None, :] < np.clip(cnt, 0, M)[:, None]
    if ids is None:
        elem = elem & ~np.isnan(S32)
    else:
        I = np.asarray(ids)
        if I.shape != (G, M) or I.dtype.kind not in "iu":
            raise ValueError(f"ids must be an integer array of shape {(G, M)}, got {I.shape} {I.dtype}")
        elem = elem & (I >= 0) & (I < int(rows_num))
    with np.errstate(invalid="ignore", over="ignore"):
        X = (np.float32(scale) * S32).astype(np.float64)              # fl32(scale * score), widened
    lab = elem & np.isfinite(gn) & (gn >= 0) & ~np.isnan(X)
    sc = float(np.float32(scale))
    loss, ndcg, valid = np.zeros(G), np.zeros(G), np.zeros(G, dtype=bool)
    lam, absum, num = np.zeros((G, M)), np.zeros((G, M)), lab.sum(axis=1)
    for g in range(G):
        at = np.flatnonzero(lab[g])
        n = len(at)
        if n == 0:
            continue
        x, gv = X[g, at], gn[g, at].astype(np.float64)
        r, t = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        r[np.lexsort((at, -x))] = np.arange(n)                        # x descending, then slot ascending
        t[np.lexsort((at, -gv))] = np.arange(n)
        Dr = D[r]
        idcg = math.fsum(gv * D[t])
        if not idcg > 0.0:
            continue
        valid[g] = True
        ndcg[g] = math.fsum(gv * Dr) / idcg
        dG = gv[:, None] - gv[None, :]
        up = dG > 0
        W = np.where(up, (dG * np.abs(Dr[:, None] - Dr[None, :])) / idcg, 0.0)
        live = W != 0
        with np.errstate(invalid="ignore", over="ignore"):
            T = np.where(live, x[:, None] - x[None, :], 0.0)
            sp = np.maximum(-T, 0.0) + np.log1p(np.exp(-np.abs(T)))
            sg = 1.0 / (1.0 + np.exp(T))
        loss[g] = math.fsum((W * sp)[live])
        L = np.where(live, W * sg, 0.0)
        for a in range(n):
            lam[g, at[a]] = sc * math.fsum(np.concatenate((-L[a, :], L[:, a])))
            absum[g, at[a]] = abs(sc) * math.fsum(np.concatenate((L[a, :], L[:, a])))
    return loss, ndcg, valid, lam, num, absum


def list_pairwise_host(scores, ids, count, gain, rows_num, scale=1.0, discount=None, parts: bool = False):
    """The contract of ``digat_list_pairwise_fwd`` on given scores ``scores`` [G, M] (slot (g, j) holds the inner product of user g
    with row ``ids[g, j]``), in numpy float64 with ``math.fsum`` sums — the yardstick of the kernels.  Slot (g, j) is an element when
    ``j < clip(count[g], 0, M)`` (``count`` None: M) and ``0 <= ids[g, j] < rows_num`` — or, with ``ids`` None (the contract of
    ``digat_list_pairwise_scores_fwd``), when its score is no NaN.  ``x = fl32(scale * scores)``.  An element is labelled when its
    ``gain`` is finite and >= 0 and x is no NaN.  Among a list's labelled elements ``r`` ranks by (x descending, slot ascending), ``t``
    by (gain descending, slot ascending), both 0-based; ``idcg = sum gain discount[t]``, ``dcg = sum gain discount[r]``, the list is
    valid when ``idcg > 0``, ``ndcg = dcg / idcg``.  Over the ordered pairs with ``gain_i > gain_j``:
    ``w = ((gain_i - gain_j) |discount[r_i] - discount[r_j]|) / idcg``, ``loss = sum w sp(x_i - x_j)`` with
    ``sp(t) = max(-t, 0) + log1p(exp(-|t|))``, and ``lambda_i = scale (-sum_{gain_i > gain_j} w_ij sg(x_i - x_j) +
    sum_{gain_j > gain_i} w_ji sg(x_j - x_i))`` with ``sg(t) = 1 / (1 + exp(t))``; all three are 0 for an invalid list, ``lambda`` is 0
    at every slot that is no labelled element.  Returns ``(loss [G], ndcg [G], valid [G] bool, lambda [G, M])``; with ``parts`` also
    ``n [G]``, the labelled elements of each list, and ``A [G, M]``, lambda's ABSOLUTE sum ``|scale| sum w sg`` —
    ``list_pairwise_bound``'s arguments."""
    out = _list_pairwise_host_parts(scores, ids, count, gain, rows_num, scale, discount)
    return out if parts else out[:4]


def list_pairwise_grad_host(users, rows, scores, ids, count, gain, scale=1.0, discount=None, grad_loss=None):
    """The contract of ``digat_list_pairwise_bwd`` in numpy float64: with ``coef = grad_loss[:, None] * lambda`` (``lambda`` of
    ``list_pairwise_host`` on ``scores``; ``grad_loss`` None: ones), ``d_users[g] = sum_j coef[g, j] rows[ids[g, j]]`` and ``d_rows[p]``
    = the sum of ``coef[g, j] users[g]`` over the elements with ``ids[g, j] == p``.  Returns ``(d_users [G, d], d_rows [P, d])``."""
    U, R = np.asarray(users, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    if U.ndim != 2 or R.ndim != 2 or U.shape[1] != R.shape[1]:
        raise ValueError(f"users [G, d] and rows [P, d] must share d, got {U.shape} and {R.shape}")
    lam = _list_pairwise_host_parts(scores, ids, count, gain, R.shape[0], scale, discount)[3]
    G = lam.shape[0]
    if U.shape[0] != G:
        raise ValueError(f"users must have one row per list ({G}), got {U.shape}")
    gl = np.ones(G) if grad_loss is None else np.asarray(grad_loss, dtype=np.float64)
    if gl.shape != (G,):
        raise ValueError("grad_loss must have one entry per list")
    coef = gl[:, None] * lam
    I = np.asarray(ids).astype(np.int64)
    g_of, j_of = np.nonzero(lam != 0)
    d_users, d_rows = np.zeros_like(U), np.zeros_like(R)
    np.add.at(d_users, g_of, coef[g_of, j_of][:, None] * R[I[g_of, j_of]])
    np.add.at(d_rows, I[g_of, j_of], coef[g_of, j_of][:, None] * U[g_of])
    return d_users, d_rows


def list_pairwise_bound(n, value, absolute=None):
    """The error bound csrc/digat_list_pairwise.inc derives for ``loss``, ``ndcg`` and ``lambda`` against ``list_pairwise_host`` on the
    same scores: ``u |value| + c(n) 2^-53 A (1 + u) + 2^-149`` with u = 2^-24, ``c(n) = 2 n + 32`` for a list of ``n`` labelled
    elements, and ``A = |value|`` for ``loss`` and ``ndcg`` (sums of positive terms) or lambda's absolute sum ``absolute``."""
    u = 2.0 ** -24
    v = np.abs(np.asarray(value, dtype=np.float64))
    A = v if absolute is None else np.abs(np.asarray(absolute, dtype=np.float64))
    return u * v + (2.0 * np.asarray(n, dtype=np.float64) + 32.0) * 2.0 ** -53 * A * (1.0 + u) + 2.0 ** -149


def _check_list_pairwise_args(scores_or_users, rows, ids, count, gain):
    """Shapes of ``list_pairwise`` (``rows`` and ``ids`` given) and of ``pairwise_scores`` (both None): ``(G, P, M, d)``."""
    import torch
    no_index = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool)
    if rows is None:
        S = scores_or_users
        if S.dim() != 2 or not S.is_floating_point():
            raise ValueError(f"scores must be a floating-point tensor [G, M], got {tuple(S.shape)} {S.dtype}")
        G, M, P, d = int(S.shape[0]), int(S.shape[1]), 0, 0
    else:
        users = scores_or_users
        if users.dim() != 2 or rows.dim() != 2 or users.shape[1] != rows.shape[1] or users.shape[1] < 1:
            raise ValueError(f"users [G, d] and rows [P, d] must share d >= 1, got {tuple(users.shape)} and {tuple(rows.shape)}")
        G, d, P = int(users.shape[0]), int(users.shape[1]), int(rows.shape[0])
        if d > LIST_SOFTMAX_MAX_D:
            raise ValueError(f"list_pairwise takes vectors of at most LIST_SOFTMAX_MAX_D = {LIST_SOFTMAX_MAX_D} channels, got {d}")
        if ids.dim() != 2 or ids.shape[0] != G or ids.dtype in no_index:
            raise ValueError(f"ids must be an integer tensor [G = {G}, M], got {tuple(ids.shape)} {ids.dtype}")
        M = int(ids.shape[1])
    if not 1 <= M <= SHORTLIST_MAX_K:
        raise ValueError(f"a list holds between 1 and SHORTLIST_MAX_K = {SHORTLIST_MAX_K} slots, got M = {M}")
    if G * M >= 1 << 31:
        raise ValueError(f"G x M must stay below 2^31, got {G} x {M}")
    if tuple(gain.shape) != (G, M) or not gain.is_floating_point():
        raise ValueError(f"gain must be a floating-point tensor with one value per slot {(G, M)}, got {tuple(gain.shape)} {gain.dtype}")
    if count is not None and (tuple(count.shape) != (G,) or count.dtype in no_index):
        raise ValueError(f"count must be an integer tensor with one entry per list ({G}), got {tuple(count.shape)} {count.dtype}")
    return G, P, M, d


_DISCOUNT_TABLES = {}         # (device, the table's bytes) -> the uploaded float64 table


def _device_discount(D: np.ndarray, device):
    import torch
    key = (str(device), D.tobytes())
    t = _DISCOUNT_TABLES.get(key)
    if t is None:
        if len(_DISCOUNT_TABLES) >= 32:
            _DISCOUNT_TABLES.clear()
        t = _DISCOUNT_TABLES[key] = torch.from_numpy(D.copy()).to(device)
    return t


def _pairwise_stock(S, elem, gain, scale, disc):
    """The stock [G, M, M] composition on scores ``S`` [G, M] (differentiable), in their dtype: ``(loss [G], ndcg [G])``."""
    import torch
    G, M = int(S.shape[0]), int(S.shape[1])
    x = float(scale) * S
    xd = x.detach()
    gain = gain.detach()
    lab = elem & torch.isfinite(gain) & (gain >= 0) & ~torch.isnan(xd)
    gv = torch.where(lab, gain, torch.zeros_like(gain)).to(S.dtype)
    xs = torch.where(lab, xd, torch.zeros_like(xd))
    slot = torch.arange(M, device=S.device)
    first = (slot[None, :] < slot[:, None])[None]                                                   # [1, i, j]: j < i
    both = lab[:, :, None] & lab[:, None, :]
    r = (both & ((xs[:, None, :] > xs[:, :, None]) | ((xs[:, None, :] == xs[:, :, None]) & first))).sum(dim=2)
    t = (both & ((gv[:, None, :] > gv[:, :, None]) | ((gv[:, None, :] == gv[:, :, None]) & first))).sum(dim=2)
    Dr, Dt = disc[r], disc[t]
    idcg, dcg = (gv * Dt * lab).sum(dim=1), (gv * Dr * lab).sum(dim=1)
    valid = idcg > 0
    safe = torch.where(valid, idcg, torch.ones_like(idcg))
    dG = gv[:, :, None] - gv[:, None, :]
    W = torch.where(both & (dG > 0) & valid[:, None, None], (dG * (Dr[:, :, None] - Dr[:, None, :]).abs()) / safe[:, None, None],
                    torch.zeros_like(dG))
    live = W != 0
    xm = torch.where(lab, x, torch.zeros_like(x))                     # no gradient reaches a slot without a label
    T = torch.where(live, xm[:, :, None] - xm[:, None, :], torch.zeros_like(W))
    sp = torch.logaddexp(torch.zeros_like(T), -T)                    # softplus(-T); its derivative at a tie, T = 0, is the right -1/2
    loss = torch.where(live, W * sp, torch.zeros_like(W)).sum(dim=(1, 2))
    return loss, torch.where(valid, dcg / safe, torch.zeros_like(dcg))


def _list_pairwise_functions():
    import torch
    from . import _lib

    class ListPairwise(torch.autograd.Function):
        """``digat_list_pairwise_fwd`` / ``digat_list_pairwise_bwd``; lambda is saved, and the sorted entry keys of the rows kernel are
        built here, in the forward: the ids carry no gradient."""

        @staticmethod
        def forward(ctx, users, rows, ids, cnt, gain, disc, scale):
            u, v = users.detach().float().contiguous(), rows.detach().float().contiguous()
            G, M, P, d = int(u.shape[0]), int(ids.shape[1]), int(v.shape[0]), int(u.shape[1])
            f = dict(dtype=torch.float32, device=u.device)
            per_list, per_slot = torch.empty((2, G), **f), torch.empty((2, G, M), **f)
            valid = torch.empty(G, dtype=torch.int32, device=u.device)
            _lib.check(_lib.lib().digat_list_pairwise_fwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(cnt), gain.data_ptr(),
                                                          disc.data_ptr(), G, P, M, d, float(scale), per_list[0].data_ptr(),
                                                          per_list[1].data_ptr(), valid.data_ptr(), per_slot[0].data_ptr(),
                                                          per_slot[1].data_ptr(), _lib.stream_ptr()), "digat_list_pairwise_fwd")
            keys = None
            if ctx.needs_input_grad[1]:
                elem = list_elements(ids, cnt, P).view(-1)
                flat = torch.arange(G * M, device=u.device)
                keys = torch.sort(ids.view(-1)[elem] * (G * M) + flat[elem]).values.contiguous()
            loss, ndcg, scores, lam = per_list[0], per_list[1], per_slot[0], per_slot[1]
            ctx.save_for_backward(u, v, ids, lam)
            ctx.cnt, ctx.keys, ctx.dtypes = cnt, keys, (users.dtype, rows.dtype)
            ctx.mark_non_differentiable(ndcg, scores)
            return loss, ndcg, scores

        @staticmethod
        def backward(ctx, grad_loss, _ndcg, _scores):
            u, v, ids, lam = ctx.saved_tensors
            G, d, P, M = int(u.shape[0]), int(u.shape[1]), int(v.shape[0]), int(ids.shape[1])
            f = dict(dtype=torch.float32, device=u.device)
            want_rows = ctx.needs_input_grad[1] and ctx.keys is not None
            d_users = torch.empty((G, d), **f)
            d_rows = torch.empty((P, d), **f) if want_rows else None
            gl = grad_loss.float().contiguous()
            L = _lib.lib()
            need = int(L.digat_list_pairwise_workspace_bytes(G, M))
            ws = _lib.workspace(need, u.device, "list_pairwise")
            keys = ctx.keys if want_rows else None
            _lib.check(L.digat_list_pairwise_bwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(ctx.cnt), G, P, M, d, lam.data_ptr(),
                                                 gl.data_ptr(), _lib.ptr(keys) if keys is not None and keys.numel() else None,
                                                 0 if keys is None else int(keys.numel()), d_users.data_ptr(), _lib.ptr(d_rows),
                                                 ws.data_ptr(), need, _lib.stream_ptr()), "digat_list_pairwise_bwd")
            return (d_users.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None), (None if d_rows is None else d_rows.to(ctx.dtypes[1])), \
                None, None, None, None, None

    class PairwiseScores(torch.autograd.Function):
        """``digat_list_pairwise_scores_fwd``; the backward is ``grad_loss[:, None] * lambda``."""

        @staticmethod
        def forward(ctx, scores, cnt, gain, disc, scale):
            s = scores.detach().float().contiguous()
            G, M = int(s.shape[0]), int(s.shape[1])
            f = dict(dtype=torch.float32, device=s.device)
            per_list, lam = torch.empty((2, G), **f), torch.empty((G, M), **f)
            valid = torch.empty(G, dtype=torch.int32, device=s.device)
            _lib.check(_lib.lib().digat_list_pairwise_scores_fwd(s.data_ptr(), _lib.ptr(cnt), gain.data_ptr(), disc.data_ptr(), G, M,
                                                                 float(scale), per_list[0].data_ptr(), per_list[1].data_ptr(),
                                                                 valid.data_ptr(), lam.data_ptr(), _lib.stream_ptr()),
                       "digat_list_pairwise_scores_fwd")
            loss, ndcg = per_list[0], per_list[1]
            ctx.save_for_backward(lam)
            ctx.dtype = scores.dtype
            ctx.mark_non_differentiable(ndcg)
            return loss, ndcg

        @staticmethod
        def backward(ctx, grad_loss, _ndcg):
            lam, = ctx.saved_tensors
            return (grad_loss.float()[:, None] * lam).to(ctx.dtype), None, None, None, None

    return ListPairwise, PairwiseScores


_ListPairwise = None


def list_pairwise(users, rows, ids, count, gain, scale=1.0, discount=None):
    """The pairwise nDCG loss (LambdaRank) of every user's OWN list: ``(loss [G], ndcg [G], scores [G, M])``.  ``users`` [G, d],
    ``rows`` [P, d], ``ids`` [G, M] integer rows of ``rows`` and ``count`` [G] (None: M) as in ``list_softmax``; ``gain`` [G, M], the
    relevance of every slot — finite and >= 0; NaN, an infinity or a negative value means "no label", and such an element takes part
    in nothing —; ``discount`` a float64 numpy table [M] of the 0-based rank, finite, non-negative and non-increasing (None:
    ``ndcg_discount(M)``; ``ndcg_discount(M, k)`` trains for nDCG@k).  With ``x = scale * <users[g], rows[ids[g, j]]>``, ranks among
    the labelled elements by (x descending, slot ascending), ``idcg`` the list's best possible ``sum gain discount[rank]``: for every
    pair with ``gain_i > gain_j`` a logistic loss ``softplus(-(x_i - x_j))`` weighted by what swapping the two would do to nDCG,
    ``(gain_i - gain_j) |discount[r_i] - discount[r_j]| / idcg`` — a constant: no gradient flows through the ranks.  ``ndcg`` is the
    list's nDCG under the current scores; a list with ``idcg`` 0 (no positive gain) has loss 0 and ndcg 0.  ``scores`` = the inner
    products at elements, NaN elsewhere.  ``loss`` is differentiable in ``users`` and ``rows``; ``ndcg`` and ``scores`` are not, and
    ``gain`` gets no gradient.  M <= ``SHORTLIST_MAX_K`` = 1024, d <= ``LIST_SOFTMAX_MAX_D`` = 512, G M < 2^31.

    On CUDA tensors: ``digat_list_pairwise_fwd`` / ``_bwd`` under autograd — no [G, M, M] tensor and no [G, M, d] gather in memory, fp64
    pair arithmetic, no float atomics: two calls give the same bits in every output and gradient; float32 outputs.  On CPU tensors: the
    stock [G, M, M] composition in the dtype of ``users``, differentiable by autograd."""
    import torch
    global _ListPairwise
    cnt = None if count is None else torch.as_tensor(count)
    G, P, M, d = _check_list_pairwise_args(users, rows, ids, cnt, gain)
    D = _check_discount(discount, M)
    dev = users.device
    if any(t.device != dev for t in (rows, ids, gain) + (() if cnt is None else (cnt,))):
        raise ValueError("users, rows, ids, count and gain must live on one device")
    ids = ids.to(torch.int64).contiguous()
    gain = gain.detach()
    if dev.type == "cuda":
        if _ListPairwise is None:
            _ListPairwise = _list_pairwise_functions()
        if G == 0 or P == 0:                                          # nothing is an element: no launch, a zero gradient
            z = users.new_zeros(G, dtype=torch.float32) + 0.0 * (users.float().sum() + rows.float().sum())
            return z, users.new_zeros(G, dtype=torch.float32), users.new_full((G, M), float("nan"), dtype=torch.float32)
        return _ListPairwise[0].apply(users, rows, ids, None if cnt is None else cnt.to(torch.int32).contiguous(), gain.float().contiguous(),
                                      _device_discount(D, dev), float(scale))
    elem = list_elements(ids, cnt, P)
    gathered = rows.index_select(0, torch.where(elem, ids, torch.zeros_like(ids)).view(-1)).view(G, M, d)        # [G, M, d]
    S = torch.bmm(gathered, users.unsqueeze(2)).squeeze(2)
    loss, ndcg = _pairwise_stock(S, elem, gain, scale, torch.from_numpy(D).to(S.dtype))
    return loss, ndcg.detach(), torch.where(elem, S.detach(), S.new_full((G, M), float("nan")))


def pairwise_scores(scores, count, gain, scale=1.0, discount=None):
    """``list_pairwise``'s loss on GIVEN scores ``scores`` [G, M] — a model whose score is no inner product, through autograd on its own
    logits: ``(loss [G], ndcg [G])``.  A slot is an element when ``j < clip(count[g], 0, M)`` (``count`` None: M) and its score is no
    NaN; ``gain``, ``scale`` and ``discount`` as in ``list_pairwise``.  ``loss`` is differentiable in ``scores`` — its gradient is
    ``grad_loss[:, None] * lambda``, exactly 0 at every slot that is no labelled element —; ``ndcg`` is not.  On CUDA tensors
    ``digat_list_pairwise_scores_fwd`` (the pair stage of ``list_pairwise``: the same bits on the same scores); on CPU tensors the
    stock [G, M, M] composition in the dtype of ``scores``."""
    import torch
    global _ListPairwise
    cnt = None if count is None else torch.as_tensor(count)
    G, _, M, _ = _check_list_pairwise_args(scores, None, None, cnt, gain)
    D = _check_discount(discount, M)
    dev = scores.device
    if gain.device != dev or (cnt is not None and cnt.device != dev):
        raise ValueError("scores, count and gain must live on one device")
    gain = gain.detach()
    if dev.type == "cuda":
        if _ListPairwise is None:
            _ListPairwise = _list_pairwise_functions()
        if G == 0:
            z = scores.new_zeros(0, dtype=torch.float32) + 0.0 * scores.float().sum()
            return z, scores.new_zeros(0, dtype=torch.float32)
        return _ListPairwise[1].apply(scores, None if cnt is None else cnt.to(torch.int32).contiguous(), gain.float().contiguous(),
                                      _device_discount(D, dev), float(scale))
    slot = torch.arange(M, device=dev)
    elem = ~torch.isnan(scores.detach())
    if cnt is not None:
        elem = elem & (slot[None, :] < cnt.to(torch.int64).clamp(0, M)[:, None])
    loss, ndcg = _pairwise_stock(torch.where(elem, scores, torch.zeros_like(scores)), elem, gain, scale, torch.from_numpy(D).to(scores.dtype))
    return loss, ndcg.detach()


MMR_MAX_LIST = TOPK_MAX_K    # include/digat_hip.h: digat_mmr_select takes lists of at most this many entries


def mmr_weights(lam):
    """``(lam, mu)`` as float32 — what ``digat_mmr_select`` is handed: ``mu = float32(1) - float32(lam)``, computed once."""
    if not 0.0 <= float(lam) <= 1.0:                                # a NaN fails both comparisons
        raise ValueError(f"lam must lie in [0, 1], got {lam}")
    lam32 = np.float32(lam)
    return lam32, np.float32(1) - lam32


def _check_select_shapes(ids_shape, scores_shape, count_shape, k, max_list):
    """What every greedy re-rank asks of its lists: ``ids`` / ``scores`` [G, 1 <= M <= max_list], ``count`` [G] or None, ``k``."""
    if len(ids_shape) != 2 or tuple(scores_shape) != tuple(ids_shape) or not 1 <= ids_shape[1] <= max_list:
        raise ValueError(f"ids and scores must both be [G, M] with 1 <= M <= {max_list}, got {tuple(ids_shape)} and {tuple(scores_shape)}")
    if count_shape is not None and tuple(count_shape) != (ids_shape[0],):
        raise ValueError(f"count must have one entry per list ({ids_shape[0]}), got shape {tuple(count_shape)}")
    if not 1 <= int(k) <= TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {TOPK_MAX_K}], got {k}")


def _check_cap(category_shape, max_per_category):
    if int(max_per_category) < 0:
        raise ValueError(f"max_per_category must be >= 0 (0: no cap), got {max_per_category}")
    if int(max_per_category) > 0 and category_shape is None:
        raise ValueError("max_per_category needs category")


def _check_target_shape(target_shape, G):
    if len(target_shape) != 2 or target_shape[0] != G or not 1 <= target_shape[1] <= CAL_MAX_CATEGORIES:
        raise ValueError(f"target must be [G, C] = [{G}, 1 <= C <= {CAL_MAX_CATEGORIES}], got {tuple(target_shape)}")


def _shape(x):
    return None if x is None else tuple(x.shape if hasattr(x, "shape") else np.shape(x))


def _host_lists(ids, scores, category):
    """``(ids int64, scores float32, category int64 or None)``: the arrays a host contract works on."""
    return (np.asarray(ids, dtype=np.int64), np.ascontiguousarray(scores, dtype=np.float32),
            None if category is None else np.asarray(category, dtype=np.int64))


def _host_sim(sim, G, M):
    S = np.asarray(sim, dtype=np.float32)
    if S.shape != (G, M, M):
        raise ValueError(f"sim must be [G, M, M] = {(G, M, M)}, got {S.shape}")
    return S


def _select_on_device(ids, scores, count, k, others, with_kl, workspace_bytes, tag):
    """What the device wrappers of the greedy re-ranks share, behind their argument checks: all tensors on one device, the lists
    as int64 / float32 / int32, the outputs ``(scores [G,k], ids [G,k], count [G])`` and with ``with_kl`` ``kl [G]``, and the
    workspace of ``workspace_bytes(lib, G, M, k)`` bytes.  Returns ``(ids, scores, count, outputs, workspace, bytes)``; the
    workspace is None where G == 0: there is nothing to launch and the empty outputs are the answer."""
    import torch
    from . import _lib
    dev = _lib.require_device(*[t for t in (ids, scores, count) + tuple(others) if t is not None])
    idt = ids.to(torch.int64).contiguous()
    sc = _lib.f32(scores.detach())
    ct = None if count is None else count.to(torch.int32).contiguous()
    G, M, k = int(idt.shape[0]), int(idt.shape[1]), int(k)
    outs = (torch.empty((G, k), dtype=torch.float32, device=dev), torch.empty((G, k), dtype=torch.int64, device=dev),
            torch.empty((G,), dtype=torch.int32, device=dev))
    if with_kl:
        outs += (torch.empty((G,), dtype=torch.float32, device=dev),)
    if G == 0:
        return idt, sc, ct, outs, None, 0
    need = int(workspace_bytes(_lib.lib(), G, M, k))
    return idt, sc, ct, outs, _lib.workspace(need, dev, tag), need


def _check_mmr_args(ids_shape, scores_shape, count_shape, k, category_shape, max_per_category):
    _check_select_shapes(ids_shape, scores_shape, count_shape, k, MMR_MAX_LIST)
    _check_cap(category_shape, max_per_category)
    if category_shape is not None and len(category_shape) != 1:
        raise ValueError(f"category must be [N], got shape {tuple(category_shape)}")


def mmr_select_host(ids, scores, count, sim, k: int, lam, category=None, max_per_category: int = 0, news_num=None):
    """The contract of ``digat_mmr_select`` in numpy — the yardstick of the kernel — on given similarities ``sim`` [G, M, M]
    float32 (``sim[g, i, j]``: list positions i and j of user g).  ``ids`` / ``scores`` [G, M], ``count`` [G] or None (M): position p
    is an element when ``p < count[g]`` and ``0 <= id < N`` (``news_num``; None: ``len(category)``, or no upper bound).  Greedy,
    k steps: ``value = float32(lam) * s - float32(mu) * pen`` with every operation rounded, the winner is the eligible element with
    the largest ``topk_keys(value)``, ties to the lowest position; then ``pen = np.fmax(pen, sim[winner])``.  Eligible: not selected,
    and with ``max_per_category`` q > 0 fewer than q selected elements of its ``category[id]``.  Returns ``(scores [G,k] float32 —
    the INPUT score bits —, ids [G,k] int64, count [G] int32)``; slots at or beyond ``count`` hold ``-inf`` / ``-1``.

    This is ``rerank_select_host``'s greedy pass (``_greedy_select_host``) with weights ``(lam, mu, 0)`` and the diversity term
    ALWAYS formed: at ``lam = 1`` the value is still ``rel - fl(0 * pen)``, a NaN where a similarity is infinite — as the kernel's."""
    idv, sc, cat = _host_lists(ids, scores, category)
    _check_mmr_args(idv.shape, sc.shape, _shape(count), k, _shape(cat), max_per_category)
    S = _host_sim(sim, *idv.shape)
    lam32, mu32 = mmr_weights(lam)
    q = int(max_per_category)
    N = news_num if news_num is not None else (len(cat) if cat is not None else None)
    return _greedy_select_host(idv, sc, count, S, int(k), lam32, mu32, np.float32(0), True, False, cat=cat if q > 0 else None, q=q, N=N)[:3]


def mmr_select(ids, scores, count, vectors, k: int, lam, category=None, max_per_category: int = 0):
    """Diversified top-k on the GPU (``digat_mmr_select``): per user, k greedy maximal-marginal-relevance picks from a short list.

    ``ids`` [G, M <= 128] int64, ``scores`` [G, M] float32 and ``count`` [G] int32 (None: M) are device tensors — what
    ``topk_segments``, ``dot_topk`` and both ``recommend``s return; ``vectors`` [N, d] float32 holds the rows the similarity is the
    inner product of (pass unit rows: ``util.unit_rows``); ``lam`` in [0, 1] weighs the score against the largest similarity to
    what is already picked (1: the plain order by score); ``category`` [N] and ``max_per_category`` q >= 1 cap the picks per
    category (0: no cap).  The contract is ``mmr_select_host``'s, exactly.  Returns ``(scores [G,k] float32, ids [G,k] int64, count
    [G] int32)`` on the device — the picked entries' input scores; slots at or beyond ``count`` hold ``-inf`` / ``-1``.
    Stream-ordered: one launch, nothing is read back."""
    import torch
    from . import _lib
    _check_mmr_args(_shape(ids), _shape(scores), _shape(count), k, _shape(category), max_per_category)
    if vectors.dim() != 2 or vectors.shape[1] < 1:
        raise ValueError(f"vectors must be [N, d] with d >= 1, got {tuple(vectors.shape)}")
    if category is not None and int(category.shape[0]) != int(vectors.shape[0]):
        raise ValueError(f"category must have one entry per row of vectors ({int(vectors.shape[0])}), got {int(category.shape[0])}")
    lam32, mu32 = mmr_weights(lam)
    idt, sc, ct, outs, ws, need = _select_on_device(ids, scores, count, k, (vectors, category), False,
                                                    lambda L, G, M, k: L.digat_mmr_select_workspace_bytes(G, M, k), "mmr")
    v = _lib.f32(vectors.detach())
    if ws is None:
        return outs
    q = int(max_per_category)
    cat = None if category is None or q == 0 else category.to(torch.int32).contiguous()
    out_s, out_i, out_c = outs
    _lib.check(_lib.lib().digat_mmr_select(idt.data_ptr(), sc.data_ptr(), _lib.ptr(ct), *idt.shape, v.data_ptr(), int(v.shape[0]), int(v.shape[1]),
                                           _lib.ptr(cat), q, float(lam32), float(mu32), int(k), out_i.data_ptr(), out_s.data_ptr(),
                                           out_c.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()),
               "digat_mmr_select")
    return outs


def mmr_gram_stock(ids, vectors):
    """``sim`` [G, M, M] of ``mmr_select_host`` on stock PyTorch, for lists and vectors on any device: the Gram of the gathered rows
    (an id outside [0, N) gathers row 0: no element, its similarities are never used)."""
    import torch
    N = int(vectors.shape[0])
    safe = torch.where((ids >= 0) & (ids < N), ids, torch.zeros_like(ids))
    rows = vectors[safe] if N else vectors.new_zeros(tuple(ids.shape) + (int(vectors.shape[1]),))
    return torch.bmm(rows, rows.transpose(1, 2))


# ---- calibrated top-k: lists that keep the reader's own category mix ----------------------------------------------------------------
CAL_MAX_LIST = SHORTLIST_MAX_K     # include/digat_hip.h: DIGAT_CALIBRATE_MAX_LIST, the longest list digat_calibrated_select takes
CAL_MAX_CATEGORIES = 64            # ... DIGAT_CALIBRATE_MAX_CATEGORIES, the widest target
CAL_ROBUST_ULPS = 8                # a robust step's winner leads by this many float32 ulps (calibrated_select_host)


def _check_alpha(alpha) -> float:
    if not 0.0 < float(alpha) < 1.0:                                # a NaN fails both comparisons
        raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
    return float(alpha)


def _check_calibrate_args(ids_shape, scores_shape, count_shape, category_shape, target_shape, k):
    _check_select_shapes(ids_shape, scores_shape, count_shape, k, CAL_MAX_LIST)
    if category_shape is None or len(category_shape) != 1:
        raise ValueError(f"category must be [N], one entry per news, got {None if category_shape is None else tuple(category_shape)}")
    _check_target_shape(target_shape, ids_shape[0])


def calibrated_select_host(ids, scores, count, category, target, k: int, lam, alpha=0.01, return_robust: bool = False):
    """The contract of ``digat_calibrated_select`` in numpy — the yardstick of the kernel.  ``ids`` / ``scores`` [G, M <= 1024],
    ``count`` [G] or None (M): position p is an element when ``p < clip(count[g], 0, M)`` and ``0 <= id < N = len(category)``
    (``mmr_select_host``'s rule; a repeated id is one element per position).  ``target`` [G, C <= 64] float32: ``p_c =
    float64(target[g, c])`` where that is finite and > 0, else 0 — nothing is normalised.  An element whose ``category[id]`` lies
    outside [0, C) is uncategorised: its gain is 0 and it is never counted.

    Greedy, steps t = 0 .. k-1 with T = t + 1 and ``n_c`` the picked elements of category c: in float64, every operation rounded,
    ``q_c(n) = ((1 - alpha) n) / T + alpha p_c`` and ``gain64_c = p_c (log q_c(n_c + 1) - log q_c(n_c))`` (0 where ``p_c = 0``);
    ``gain32_c = float32(gain64_c)``; ``value = float32(lam) * s + float32(mu) * gain32[cat]`` with both products and the sum
    rounded (``mmr_weights``); the winner is the unpicked element with the largest ``topk_keys(value)``, ties to the lowest
    position; selection stops when no element is left.  That is the greedy step of ``lam sum(s) - mu KL(p || q)`` with the term all
    candidates share dropped.  Returns ``(scores [G,k] float32 — the INPUT score bits —, ids [G,k] int64, count [G] int32, kl [G]
    float32)``: slots at or beyond ``count`` hold ``-inf`` / ``-1``; ``kl = float32(sum over p_c > 0 of p_c (log p_c - log
    q_c(n_c)))`` at ``T = max(count, 1)``, summed in float64.  ``lam = 1`` and an all-zero target row give the plain top-k.

    ``return_robust``: a fifth array [G] bool.  A list is robust when at every step the winner's value leads every other unpicked
    element's by at least ``CAL_ROBUST_ULPS`` = 8 float32 ulps of the largest of ``|value|``, ``|lam s|`` and ``|mu gain|`` of the
    two — or the two are a true tie: equal scores and the same gain inputs (the same ``p_c`` bits and ``n_c``, or both
    gain-free), or one of the two scores is not finite (then neither value depends on a gain).  Two correct float64 logarithms
    may differ by one float32 step in ``gain32``, about 2 ulps of a value: on a robust list every such implementation picks
    the same elements.

    This is ``rerank_select_host``'s greedy pass (``_greedy_select_host``) with weights ``(lam, 0, mu)`` and the calibration term
    ALWAYS formed, ``mu = 0`` included — so the certificate is computed at every ``lam``."""
    idv, sc, cat = _host_lists(ids, scores, category)
    tgt = np.asarray(target, dtype=np.float32)
    _check_calibrate_args(idv.shape, sc.shape, _shape(count), _shape(cat), tgt.shape, k)
    lam32, mu32 = mmr_weights(lam)
    out = _greedy_select_host(idv, sc, count, None, int(k), lam32, np.float32(0), mu32, False, True, cat=cat, tgt=tgt,
                              alpha=_check_alpha(alpha), N=len(cat), want_robust=return_robust)
    return out if return_robust else out[:4]


def calibrated_select(ids, scores, count, category, target, k: int, lam, alpha=0.01):
    """Calibrated top-k on the GPU (``digat_calibrated_select``): per user, k greedy picks from a shortlist that weigh an entry's
    score against what it does for the KL divergence between ``target`` — the category mix the list should have, e.g.
    ``category_share`` of the user's history — and the list's own mix.

    ``ids`` [G, M <= 1024] int64, ``scores`` [G, M] float32 and ``count`` [G] int32 (None: M) are device tensors — what
    ``shortlist_segments``, ``dot_shortlist``, ``topk_segments`` and both ``recommend``s return; ``category`` [N] int, ``target``
    [G, C <= 64] float32; ``lam`` in [0, 1] (1: the plain order by score), ``alpha`` in (0, 1) smooths the list's mix towards the
    target.  The contract is ``calibrated_select_host``'s, exactly.  Returns ``(scores [G,k] float32, ids [G,k] int64, count [G]
    int32, kl [G] float32)`` on the device — the picked entries' input scores and the divergence of the finished list; slots at
    or beyond ``count`` hold ``-inf`` / ``-1``.  Stream-ordered: one launch, nothing is read back."""
    import torch
    from . import _lib
    _check_calibrate_args(_shape(ids), _shape(scores), _shape(count), _shape(category), _shape(target), k)
    lam32, mu32 = mmr_weights(lam)
    alpha = _check_alpha(alpha)
    C = int(target.shape[1])
    idt, sc, ct, outs, ws, need = _select_on_device(ids, scores, count, k, (category, target), True,
                                                    lambda L, G, M, k: L.digat_calibrated_select_workspace_bytes(G, M, C, k), "calibrate")
    cat = category.to(torch.int32).contiguous()
    tg = _lib.f32(target.detach())
    if ws is None:
        return outs
    out_s, out_i, out_c, out_kl = outs
    dummy = ws if int(cat.shape[0]) == 0 else cat                    # an empty tensor has no storage to point at
    _lib.check(_lib.lib().digat_calibrated_select(idt.data_ptr(), sc.data_ptr(), _lib.ptr(ct), *idt.shape, dummy.data_ptr(), int(cat.shape[0]),
                                                  tg.data_ptr(), C, float(lam32), float(mu32), alpha, int(k), out_i.data_ptr(),
                                                  out_s.data_ptr(), out_c.data_ptr(), out_kl.data_ptr(), ws.data_ptr(), need,
                                                  _lib.stream_ptr()),
               "digat_calibrated_select")
    return outs


# ---- joint re-rank: diversity, calibration and a cap per category in one greedy pass over up to 1024 entries -----------------------
RERANK_MAX_LIST = SHORTLIST_MAX_K  # include/digat_hip.h: DIGAT_RERANK_MAX_LIST, the longest list digat_rerank_select takes
RERANK_MAX_D = 512                 # ... DIGAT_LIST_SOFTMAX_MAX_D: the widest vectors a diversity term takes (w_div != 0)


def rerank_weights(diversity, calibration):
    """``(w_rel, w_div, w_cal)`` as float32 — what ``digat_rerank_select`` is handed — for the public knob ``rerank=(diversity,
    calibration)``: both in [0, 1], their sum at most 1; ``w_rel = float32(1 - diversity - calibration)``."""
    d, c = float(diversity), float(calibration)
    if not (0.0 <= d <= 1.0 and 0.0 <= c <= 1.0):                    # a NaN fails the comparisons
        raise ValueError(f"rerank's diversity and calibration must each lie in [0, 1], got {(diversity, calibration)}")
    if not d + c <= 1.0:
        raise ValueError(f"rerank's diversity and calibration must add up to at most 1, got {(diversity, calibration)}")
    return np.float32(max(0.0, 1.0 - d - c)), np.float32(d), np.float32(c)


def _check_rerank_weights(w_rel, w_div, w_cal):
    w = tuple(np.float32(x) for x in (w_rel, w_div, w_cal))
    if not all(np.isfinite(x) and x >= 0 for x in w):
        raise ValueError(f"w_rel, w_div and w_cal must be finite and >= 0, got {(w_rel, w_div, w_cal)}")
    return w


def _check_rerank_args(ids_shape, scores_shape, count_shape, k, category_shape, target_shape, max_per_category, w_cal):
    _check_select_shapes(ids_shape, scores_shape, count_shape, k, RERANK_MAX_LIST)
    _check_cap(category_shape, max_per_category)
    if category_shape is not None and len(category_shape) != 1:
        raise ValueError(f"category must be [N], one entry per news, got shape {tuple(category_shape)}")
    if w_cal != 0 and (category_shape is None or target_shape is None):
        raise ValueError("a calibration weight needs category [N] and target [G, C]")
    if target_shape is not None:
        if category_shape is None:
            raise ValueError("target needs category [N]")
        _check_target_shape(target_shape, ids_shape[0])


def _greedy_select_host(idv, sc, count, S, k, wr, wd, wc, form_div, form_cal, cat=None, tgt=None, alpha=0.01, q=0, N=None,
                        want_robust=False):
    """The one greedy pass behind ``mmr_select_host``, ``calibrated_select_host`` and ``rerank_select_host``, on checked and
    converted arrays (``_host_lists``; ``S`` [G, M, M] float32 where ``form_div``; ``tgt`` [G, C] float32 or None) and float32
    weights.  ``form_div`` / ``form_cal`` say whether the diversity / calibration term is FORMED: ``rerank_select_host`` forms a
    term where its weight is not zero, the two reductions form their own term at every weight.  A cap ``q`` > 0 needs ``cat``;
    ``N`` bounds the ids (None: no upper bound).  Returns ``(scores, ids, count, kl, robust)``; ``robust`` is the certificate
    where ``want_robust`` and the calibration term is formed, all True otherwise."""
    alpha = np.float64(alpha)
    oma = np.float64(1.0) - alpha
    G, M = idv.shape
    C = 0 if tgt is None else tgt.shape[1]
    cnt = np.full(G, M, dtype=np.int64) if count is None else np.clip(np.asarray(count, dtype=np.int64), 0, M)
    out_s = np.full((G, k), -np.inf, dtype=np.float32)
    out_i = np.full((G, k), -1, dtype=np.int64)
    out_c = np.zeros(G, dtype=np.int32)
    out_kl = np.zeros(G, dtype=np.float32)
    robust = np.ones(G, dtype=bool)
    pos = np.arange(M)
    zero = np.float32(0)
    for g in range(G):
        elem = (pos < cnt[g]) & (idv[g] >= 0)
        if N is not None:
            elem &= idv[g] < N
        cg = cat[np.where(elem, idv[g], 0)] if cat is not None and elem.any() else np.zeros(M, dtype=np.int64)
        cated = elem & (cg >= 0) & (cg < C)
        ci = np.where(cated, cg, 0)
        if C:
            pbits = np.where(np.isfinite(tgt[g]) & (tgt[g] > 0), tgt[g], zero).astype(np.float32)
        else:
            pbits = np.zeros(1, dtype=np.float32)
        p = pbits.astype(np.float64)
        live = p > 0
        pl, apl = p[live], alpha * p[live]
        free = ~(cated & live[ci])                                  # elements no gain reaches
        n = np.zeros(max(C, 1), dtype=np.int64)
        chosen = np.zeros(M, dtype=bool)
        same = np.zeros(M, dtype=np.int64)
        pen = np.zeros(M, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            rel = (wr * sc[g]).astype(np.float32)
        red = np.zeros(M, dtype=np.float32)
        dp = np.zeros(M, dtype=np.float32)
        t_end = 0
        for t in range(k):
            ok = elem & ~chosen
            if q > 0:
                ok &= same < q
            if not ok.any():
                break
            with np.errstate(invalid="ignore", over="ignore"):
                value = rel
                if form_div:
                    dp = (wd * pen).astype(np.float32)
                    value = (rel - dp).astype(np.float32)
                if form_cal:
                    T = np.float64(t + 1)
                    gain64 = np.zeros(C, dtype=np.float64)
                    nl = n[:C][live].astype(np.float64)
                    gain64[live] = pl * (np.log((oma * (nl + 1.0)) / T + apl) - np.log((oma * nl) / T + apl))
                    mg = (wc * gain64.astype(np.float32)).astype(np.float32)
                    red = np.where(cated, mg[ci], zero)
                    value = (value + red).astype(np.float32)
            keys = np.where(ok, topk_keys(value).astype(np.int64), -1)
            j = int(np.argmax(keys))                                # the first (lowest position) of the largest key
            if want_robust and robust[g] and form_cal:
                others = ok.copy()
                others[j] = False
                with np.errstate(invalid="ignore", over="ignore"):
                    mag = np.maximum(np.maximum(np.maximum(np.abs(value), np.abs(rel)), np.abs(red)), np.abs(dp))
                    ulp = np.spacing(np.maximum(mag, mag[j]).astype(np.float32)).astype(np.float64)
                    lead = np.float64(value[j]) - value.astype(np.float64)
                    fixed = ~np.isfinite(rel) | ~np.isfinite(rel[j])
                    same_gain = (free & free[j]) | (~free & ~free[j] & (pbits[ci].view(np.uint32) == pbits[ci[j]].view(np.uint32))
                                                    & (n[ci] == n[ci[j]]))
                    tie = (sc[g] == sc[g, j]) & same_gain & (dp.view(np.uint32) == dp[j].view(np.uint32))
                    if np.any(others & ~fixed & ~tie & ~(lead >= CAL_ROBUST_ULPS * ulp)):
                        robust[g] = False
            chosen[j] = True
            out_s[g, t], out_i[g, t] = sc[g, j], idv[g, j]
            t_end = t + 1
            if form_div:
                pen = np.fmax(pen, S[g, j])
            if cated[j]:
                n[cg[j]] += 1
            if q > 0:
                same += elem & (cg == cg[j])
        out_c[g] = t_end
        if live.any():
            qq = (oma * n[:C][live].astype(np.float64)) / np.float64(max(t_end, 1)) + apl
            out_kl[g] = np.float32(np.sum(pl * (np.log(pl) - np.log(qq))))
    return out_s, out_i, out_c, out_kl, robust


def rerank_select_host(ids, scores, count, sim, k: int, w_rel, w_div, w_cal, category=None, target=None, alpha=0.01,
                       max_per_category: int = 0, news_num=None, return_robust: bool = False):
    """The contract of ``digat_rerank_select`` in numpy — the yardstick of the kernel: ``mmr_select_host`` and
    ``calibrated_select_host`` in one greedy pass.  ``ids`` / ``scores`` [G, M <= 1024], ``count`` [G] or None (M): position p is
    an element when ``p < clip(count[g], 0, M)`` and ``0 <= id < N`` (``news_num``; None: ``len(category)``, or no upper bound);
    ``sim`` [G, M, M] float32 as ``mmr_select_host`` takes it (None where ``w_div == 0``).  The weights are float32, finite and
    >= 0, taken as given (``rerank_weights`` makes them from the public knob).

    Step t, every operation a rounded float32 one: ``rel = w_rel * s`` (once); ``a = rel - (w_div * pen)`` if ``w_div != 0`` else
    ``rel``; ``value = a + red`` if ``w_cal != 0`` else ``a`` with ``red = w_cal * gain32[c]`` for an element categorised in
    [0, C) and 0 otherwise — ``calibrated_select_host``'s gains, float64 ``q_c`` and logarithms at the same ``alpha``.  The winner
    is the eligible element with the largest ``topk_keys(value)``, ties to the lowest position; eligible: unpicked and, with
    ``max_per_category`` q > 0, fewer than q picked elements of its raw ``category[id]``.  After a pick ``pen = fmax(pen,
    sim[winner])`` (``w_div != 0``) and ``n_c += 1`` for a categorised winner.  Returns ``(scores [G,k] float32 — the INPUT score
    bits —, ids [G,k] int64, count [G] int32, kl [G] float32)``; ``kl`` is ``calibrated_select_host``'s of the finished list, 0
    without a target.

    ``return_robust``: ``calibrated_select_host``'s certificate as a fifth array; the magnitude also takes ``|w_div * pen|`` and a
    true tie also needs equal ``w_div * pen`` bits.  With ``w_cal == 0`` there is no logarithm and every list is robust."""
    idv, sc, cat = _host_lists(ids, scores, category)
    tgt = None if target is None else np.asarray(target, dtype=np.float32)
    wr, wd, wc = _check_rerank_weights(w_rel, w_div, w_cal)
    _check_rerank_args(idv.shape, sc.shape, _shape(count), k, _shape(cat), _shape(tgt), max_per_category, wc)
    alpha = _check_alpha(alpha)
    S = _host_sim(sim, *idv.shape) if wd != 0 else None
    N = news_num if news_num is not None else (len(cat) if cat is not None else None)
    out = _greedy_select_host(idv, sc, count, S, int(k), wr, wd, wc, bool(wd != 0), bool(wc != 0), cat=cat, tgt=tgt, alpha=alpha,
                              q=int(max_per_category), N=N, want_robust=return_robust)
    return out if return_robust else out[:4]


def rerank_select(ids, scores, count, vectors, k: int, w_rel, w_div, w_cal, category=None, target=None, alpha=0.01,
                  max_per_category: int = 0):
    """The joint re-rank on the GPU (``digat_rerank_select``): per user, k greedy picks from a shortlist of up to 1024 that weigh
    an entry's score against its largest similarity to what is already picked AND against what it does for the KL divergence
    between ``target`` and the list's category mix, under a cap per category — ``mmr_select`` and ``calibrated_select`` in one
    objective, and plain MMR beyond 128 entries (``w_cal = 0``).

    ``ids`` [G, M <= 1024] int64, ``scores`` [G, M] float32 and ``count`` [G] int32 (None: M) are device tensors; ``vectors`` [N,
    d <= 512] float32 holds the rows the similarity is the inner product of (``digat_dot_scores``' bits; None where ``w_div ==
    0``); the weights are float32, finite and >= 0 (``rerank_weights``); ``category`` [N] int and ``target`` [G, C <= 64] as
    ``calibrated_select`` takes them (None where ``w_cal == 0`` — ``category`` then only with a cap); ``max_per_category`` q >= 1
    caps the picks per raw category.  The contract is ``rerank_select_host``'s, exactly.  Returns ``(scores [G,k] float32, ids
    [G,k] int64, count [G] int32, kl [G] float32)`` on the device.  Stream-ordered: one launch, no Gram in memory, nothing is
    read back."""
    import torch
    from . import _lib
    wr, wd, wc = _check_rerank_weights(w_rel, w_div, w_cal)
    _check_rerank_args(_shape(ids), _shape(scores), _shape(count), k, _shape(category), _shape(target), max_per_category, wc)
    alpha = _check_alpha(alpha)
    if wd != 0:
        if vectors is None or vectors.dim() != 2 or not 1 <= int(vectors.shape[1]) <= RERANK_MAX_D:
            raise ValueError(f"a diversity weight needs vectors [N, d] with 1 <= d <= {RERANK_MAX_D}, got "
                             f"{None if vectors is None else tuple(vectors.shape)}")
    elif vectors is not None and vectors.dim() != 2:
        raise ValueError(f"vectors must be [N, d], got {tuple(vectors.shape)}")
    if vectors is not None and category is not None and int(category.shape[0]) != int(vectors.shape[0]):
        raise ValueError(f"category must have one entry per row of vectors ({int(vectors.shape[0])}), got {int(category.shape[0])}")
    if vectors is None and category is None:
        raise ValueError("rerank_select needs vectors or category: the number of news N bounds the ids")
    idt, sc, ct, outs, ws, need = _select_on_device(ids, scores, count, k, (vectors, category, target), True,
                                                    lambda L, G, M, k: L.digat_rerank_select_workspace_bytes(G, M, k), "rerank")
    v = None if vectors is None or wd == 0 else _lib.f32(vectors.detach())
    cat = None if category is None else category.to(torch.int32).contiguous()
    tg = None if target is None else _lib.f32(target.detach())
    if ws is None:
        return outs
    N = int(vectors.shape[0]) if vectors is not None else int(category.shape[0])
    C = 0 if tg is None else int(tg.shape[1])
    if N == 0:                                                      # empty tensors have no storage to point at; no id is an element
        v = None if v is None else ws
        cat = None if cat is None else ws
    out_s, out_i, out_c, out_kl = outs
    _lib.check(_lib.lib().digat_rerank_select(idt.data_ptr(), sc.data_ptr(), _lib.ptr(ct), *idt.shape, _lib.ptr(v), N,
                                              0 if v is None else int(vectors.shape[1]), _lib.ptr(cat), int(max_per_category), _lib.ptr(tg), C,
                                              float(wr), float(wd), float(wc), alpha, int(k), out_i.data_ptr(), out_s.data_ptr(),
                                              out_c.data_ptr(), out_kl.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()),
               "digat_rerank_select")
    return outs


# ---- exposure-capped top-k: the one stage over the BATCH of lists — no news in more than cap[id] of them (deferred acceptance) ------
CAP_MAX_LIST = SHORTLIST_MAX_K     # include/digat_hip.h: DIGAT_CAPPED_MAX_LIST, the longest list the digat_capped_* entries take
CAP_MAX_K = TOPK_MAX_K             # the most entries a list may hold
CAP_ROUNDS_PER_SYNC = 4            # the rounds capped_select enqueues between two reads of the rejection counters
CAP_MAX_ROUNDS = 1024              # the rounds after which capped_select / capped_select_host give up
_CAP_NO_ELEMENT = 0x7fffffffffffffff       # the item word of a pair that is no element: behind every news in the sort
_CAP_KEY_NEG_INF = 0x007fffff              # topk_keys(-inf); a NaN's key is 1: an element's score key lies above both


def _check_capped_args(ids_shape, scores_shape, count_shape, priority_shape, k, pool, rounds_per_sync=1, max_rounds=1) -> int:
    _check_select_shapes(ids_shape, scores_shape, count_shape, k, CAP_MAX_LIST)
    if priority_shape is not None and tuple(priority_shape) != tuple(ids_shape):
        raise ValueError(f"priority must be [G, M] = {tuple(ids_shape)}, got {tuple(priority_shape)}")
    if not 0 <= int(pool) < 2 ** 31:
        raise ValueError(f"pool must be the number of news, in [0, 2^31), got {pool}")
    if ids_shape[0] * ids_shape[1] >= 2 ** 31:
        raise ValueError(f"G M must stay below 2^31, got {tuple(ids_shape)}")
    if int(rounds_per_sync) < 1 or int(max_rounds) < 1:
        raise ValueError(f"rounds_per_sync and max_rounds must be >= 1, got {rounds_per_sync} and {max_rounds}")
    return int(pool)


def capped_caps_host(cap, pool: int) -> np.ndarray:
    """``cap`` of ``capped_select_host`` as an int32 array [P]: an int >= 0 names every news' capacity, an integer array [P] is
    taken as given (an entry <= 0 blocks its news)."""
    P = int(pool)
    if np.ndim(cap) == 0:
        if isinstance(cap, (bool, np.bool_)) or int(cap) != cap or int(cap) < 0:
            raise ValueError(f"cap must be an int >= 0 or an integer array [pool], got {cap!r}")
        return np.full(P, min(int(cap), 2 ** 31 - 1), dtype=np.int32)
    c = np.asarray(cap)
    if c.shape != (P,) or c.dtype.kind not in "iu":
        raise ValueError(f"cap must be an int >= 0 or an integer array [pool = {P}], got shape {c.shape} {c.dtype}")
    return np.clip(c, -1, 2 ** 31 - 1).astype(np.int32)


def capped_select_host(ids, scores, count, k: int, cap, pool: int, priority=None, max_rounds: int = CAP_MAX_ROUNDS):
    """The contract of the ``digat_capped_*`` entries in numpy — the yardstick of ``capped_select``.  Exposure-capped top-k over a
    BATCH of lists: every list keeps at most k of its entries and news ``id`` is kept by at most ``cap[id]`` lists of the call.

    ``ids`` [G, M <= 1024] int64, ``scores`` [G, M] float32, ``count`` [G] or None (M), ``k`` in [1, 128], ``pool`` = P the number of
    news, ``cap`` an int >= 0 for every news or an integer array [P] (``cap[id] <= 0`` blocks a news), ``priority`` [G, M] float32 or
    None (the scores).  Pair (g, j) is an ELEMENT when ``j < clip(count[g], 0, M)``, ``0 <= ids[g, j] < P``, ``scores[g, j]`` is
    neither NaN nor ``-inf`` and ``priority[g, j]`` is no NaN — ``recommend``'s fill (id -1, score ``-inf``) is no element.  A list
    that names one id twice has TWO pairs; each is a pair in its own right, it may be held twice by that list and counts twice
    against the news' capacity.

    Orders, both strict: a list orders its elements by ``topk_keys(score)`` descending, then slot ascending (the rank file's order;
    ``-0`` equals ``+0``); an item orders the pairs that name it by ``topk_keys(priority)`` descending, then g ascending, then slot
    ascending.  The result is the unique set H of elements such that every list holds at most k, every item is held at most
    ``cap[id]`` times, H is STABLE — no element outside H whose list holds fewer than k or prefers it to its worst held entry AND
    whose item has capacity and either room or a worse holder — and among the stable sets H is the one every list likes best
    (deferred acceptance with the lists proposing).  It is a stable assignment, NOT the assignment of largest total score.  No
    floating-point arithmetic takes part, only comparisons of keys: any schedule of proposals gives the same H.

    The round-wise definition the kernels follow: ``rejected`` starts as the non-elements; in a round every list demands its first k
    non-rejected entries in list order, then every item walks its pairs in item order, counts the demanded ones, and from the pair
    behind the ``cap[id]``-th demanded one on (from the start when the capacity is 0) every pair not yet rejected becomes rejected,
    demanded or not — an item's held set only improves, so those can never be accepted.  The first round that rejects nothing ends
    the loop; its demand sets are H and ``rounds`` counts the rounds up to and including it.  More than ``max_rounds``:
    ``RuntimeError``.

    Returns ``(ids [G,k] int64, scores [G,k] float32 — the INPUT bits —, count [G] int32, slots [G,k] int32, rounds)``: the held
    entries in the list's order, behind ``count[g]`` id -1, score ``-inf``, slot -1.  A list comes back with fewer than k entries
    when its shortlist runs out: hand in a deeper shortlist.  ``cap >= G`` everywhere gives the plain top-k of the elements."""
    idv = np.asarray(ids, dtype=np.int64)
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    pr = None if priority is None else np.ascontiguousarray(priority, dtype=np.float32)
    P = _check_capped_args(idv.shape, sc.shape, _shape(count), _shape(pr), k, pool, 1, max_rounds)
    caps = capped_caps_host(cap, P).astype(np.int64)
    G, M = idv.shape
    k = int(k)
    cnt = np.full(G, M, dtype=np.int64) if count is None else np.clip(np.asarray(count, dtype=np.int64), 0, M)
    ks = topk_keys(sc).reshape(G, M).astype(np.int64)
    kp = ks if pr is None else topk_keys(pr).reshape(G, M).astype(np.int64)
    elem = (np.arange(M)[None, :] < cnt[:, None]) & (idv >= 0) & (idv < P) & (ks > _CAP_KEY_NEG_INF) & (kp != 1)
    # a list's order, rank -> slot: elements by key descending, slot ascending; the non-elements behind them
    order = np.argsort(-np.where(elem, ks, -1), axis=1, kind="stable")
    # the items' order: one stable sort of (id, ~priority key) words over the pairs in flat order — g ascending, then slot
    words = np.where(elem, (np.where(elem, idv, 0) << 32) | (~kp & 0xffffffff), _CAP_NO_ELEMENT).reshape(-1)
    perm = np.argsort(words, kind="stable")[:int(elem.sum())]
    sid = idv.reshape(-1)[perm]
    first = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]]) if len(sid) else np.zeros(0, dtype=np.int64)
    seg = np.cumsum(np.r_[True, sid[1:] != sid[:-1]]) - 1 if len(sid) else np.zeros(0, dtype=np.int64)
    cap_of = caps[sid]
    rejected = ~elem.reshape(-1)
    rounds = 0
    while True:
        if rounds == int(max_rounds):
            raise RuntimeError(f"capped_select_host: no fixed point within max_rounds = {max_rounds} rounds")
        rounds += 1
        alive = ~np.take_along_axis(rejected.reshape(G, M), order, axis=1)                # rank space
        ahead = np.cumsum(alive, axis=1)
        wanted = alive & (ahead <= k)
        demand = np.zeros((G, M), dtype=bool)
        np.put_along_axis(demand, order, wanted, axis=1)
        d = demand.reshape(-1)[perm].astype(np.int64)
        before = np.cumsum(d) - d                                                       # demanded pairs in front, in the whole sort ...
        before = before - before[first][seg] if len(d) else before                      # ... and in the pair's own segment
        new = (before >= cap_of) & ~rejected[perm]
        if not new.any():
            break
        rejected[perm[new]] = True
    out_i = np.full((G, k), -1, dtype=np.int64)
    out_s = np.full((G, k), -np.inf, dtype=np.float32)
    out_p = np.full((G, k), -1, dtype=np.int32)
    gi, ri = np.nonzero(wanted)
    at, slot = ahead[gi, ri] - 1, order[gi, ri]
    out_i[gi, at] = idv[gi, slot]
    out_s[gi, at] = sc[gi, slot]
    out_p[gi, at] = slot
    return out_i, out_s, wanted.sum(axis=1).astype(np.int32), out_p, rounds


def capped_select(ids, scores, count, k: int, cap, pool: int, priority=None, rounds_per_sync: int = CAP_ROUNDS_PER_SYNC,
                  max_rounds: int = CAP_MAX_ROUNDS):
    """Exposure-capped top-k on the GPU (``digat_capped_prepare`` / ``digat_capped_rounds`` / ``digat_capped_emit``): every list keeps
    at most k of its entries, news ``id`` is kept by at most ``cap[id]`` lists of the call — the list-optimal stable assignment.

    ``ids`` [G, M <= 1024] int64, ``scores`` [G, M] float32 and ``count`` [G] int32 (None: M) are device tensors — what
    ``shortlist_segments``, ``dot_shortlist`` and both ``recommend``s return; ``pool`` the number of news, ``cap`` an int >= 0 or an
    integer tensor [pool] (an entry <= 0 blocks its news), ``priority`` [G, M] float32 orders the lists that contend for a news
    (None: by score).  The contract is ``capped_select_host``'s, exactly: ids, score bits, counts, slots, fill and ``rounds``; it is
    a stable assignment, not the one of largest total score, and a list whose shortlist runs out comes back short — hand in a deeper
    one.  Returns ``(ids [G,k] int64, scores [G,k] float32, count [G] int32, slots [G,k] int32, rounds)``, the tensors on the device.

    Not stream-only: one stable ``torch.sort`` of the item words, one read of how many news can bind at all, and then blocks of
    ``rounds_per_sync`` rounds, each followed by a read of its rejection counters — the loop stops at the first round that rejected
    nothing.  Neither the result nor ``rounds`` depends on ``rounds_per_sync``.  More than ``max_rounds`` rounds: ``RuntimeError``,
    nothing is returned."""
    import torch
    from . import _lib
    P = _check_capped_args(_shape(ids), _shape(scores), _shape(count), _shape(priority), k, pool, rounds_per_sync, max_rounds)
    cap_t = cap if torch.is_tensor(cap) else None
    dev = _lib.require_device(*[t for t in (ids, scores, count, priority, cap_t) if t is not None])
    if cap_t is None:
        caps = torch.from_numpy(capped_caps_host(cap, P)).to(dev)
    else:
        if tuple(cap_t.shape) != (P,) or cap_t.is_floating_point() or cap_t.dtype == torch.bool:
            raise ValueError(f"cap must be an int >= 0 or an integer tensor [pool = {P}], got {tuple(cap_t.shape)} {cap_t.dtype}")
        caps = cap_t.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
    idt = ids.to(torch.int64).contiguous()
    sc = _lib.f32(scores.detach())
    pr = None if priority is None else _lib.f32(priority.detach())
    ct = None if count is None else count.to(torch.int32).contiguous()
    G, M, k = int(idt.shape[0]), int(idt.shape[1]), int(k)
    out_i = torch.empty((G, k), dtype=torch.int64, device=dev)
    out_s = torch.empty((G, k), dtype=torch.float32, device=dev)
    out_c = torch.empty((G,), dtype=torch.int32, device=dev)
    out_p = torch.empty((G, k), dtype=torch.int32, device=dev)
    if G == 0:
        return out_i, out_s, out_c, out_p, 1
    L = _lib.lib()
    need = int(L.digat_capped_select_workspace_bytes(G, M))
    ws = _lib.workspace(need, dev, "capped")
    tail = (ws.data_ptr(), need, _lib.stream_ptr())
    _lib.check(L.digat_capped_prepare(idt.data_ptr(), sc.data_ptr(), _lib.ptr(pr), _lib.ptr(ct), G, M, P, *tail), "digat_capped_prepare")
    # the inverted index in item order: one stable sort of the item words (ties keep flat order: g, then slot), then every news' run
    # and the runs longer than their capacity — no other can ever reject
    words, perm = torch.sort(ws[:G * M * 8].view(torch.int64), stable=True)
    perm = perm.to(torch.int32)
    bounds = torch.searchsorted(words >> 32, torch.arange(P + 1, dtype=torch.int64, device=dev))
    length = bounds[1:] - bounds[:-1]
    binding = torch.nonzero(length > caps).view(-1)                  # the one read-back before the rounds: it sizes the item grid
    n_seg = int(binding.shape[0])
    seg_begin = bounds[:-1][binding].to(torch.int32)
    seg_cap = caps[binding].contiguous()
    seg_live = length[binding].to(torch.int32)
    segs = (seg_begin, seg_cap, seg_live) if n_seg else (None, None, None)
    done, rounds = 0, 0
    while not rounds:
        if done >= int(max_rounds):
            raise RuntimeError(f"capped_select: no fixed point within max_rounds = {max_rounds} rounds")
        n = min(int(rounds_per_sync), int(max_rounds) - done)
        counter = torch.zeros((n,), dtype=torch.int32, device=dev)
        _lib.check(L.digat_capped_rounds(G, M, k, perm.data_ptr(), *(_lib.ptr(t) for t in segs), n_seg, counter.data_ptr(), n, *tail),
                   "digat_capped_rounds")
        still = np.flatnonzero(counter.cpu().numpy() == 0)
        if len(still):
            rounds = done + int(still[0]) + 1
        done += n
    _lib.check(L.digat_capped_emit(idt.data_ptr(), sc.data_ptr(), G, M, k, out_i.data_ptr(), out_s.data_ptr(), out_c.data_ptr(),
                                   out_p.data_ptr(), *tail), "digat_capped_emit")
    return out_i, out_s, out_c, out_p, rounds


def _check_share_args(history_shape, category_shape, C):
    if len(history_shape) != 2:
        raise ValueError(f"history must be [G, H], got shape {tuple(history_shape)}")
    if len(category_shape) != 1:
        raise ValueError(f"category must be [N], got shape {tuple(category_shape)}")
    if not 1 <= int(C) <= CAL_MAX_CATEGORIES:
        raise ValueError(f"C must be in [1, {CAL_MAX_CATEGORIES}], got {C}")


def category_share_host(history, category, C: int, pad_id: int = 0) -> np.ndarray:
    """``category_share`` in numpy: [G, C] float32."""
    hist = np.asarray(history, dtype=np.int64)
    cat = np.asarray(category, dtype=np.int64)
    _check_share_args(hist.shape, cat.shape, C)
    G, C = hist.shape[0], int(C)
    inside = (hist != pad_id) & (hist >= 0) & (hist < len(cat))
    c = cat[np.where(inside, hist, 0)] if inside.any() else np.zeros_like(hist)
    ok = inside & (c >= 0) & (c < C)
    counts = np.zeros((G, C), dtype=np.int64)
    np.add.at(counts, (np.nonzero(ok)[0], c[ok]), 1)
    total = counts.sum(axis=1, keepdims=True)
    return np.where(total > 0, counts.astype(np.float32) / np.maximum(total, 1).astype(np.float32), np.float32(0)).astype(np.float32)


def category_share(history, category, C: int, pad_id: int = 0):
    """The category mix of every user's history, the usual ``target`` of ``calibrated_select``: row g of the result [G, C] float32
    is the share of each category among the slots of ``history`` [G, H] (news ids) whose id is not ``pad_id``, lies in [0, N) and
    whose ``category`` [N] lies in [0, C).  Integer counts (``scatter_add``: exact), then one float32 division; a history without
    such a slot gives a zero row — the plain top-k for that user.  Stock PyTorch on the tensors' device: not a hot path."""
    import torch
    _check_share_args(tuple(history.shape), tuple(category.shape), C)
    hist = history.to(torch.int64)
    cat = category.to(hist.device, torch.int64)
    G, C, N = int(hist.shape[0]), int(C), int(cat.shape[0])
    inside = (hist != pad_id) & (hist >= 0) & (hist < N)
    c = cat[torch.where(inside, hist, torch.zeros_like(hist))] if N else torch.zeros_like(hist)
    ok = inside & (c >= 0) & (c < C)
    counts = torch.zeros((G, C), dtype=torch.int64, device=hist.device)
    counts.scatter_add_(1, torch.where(ok, c, torch.zeros_like(c)), ok.to(torch.int64))
    total = counts.sum(dim=1, keepdim=True)
    share = counts.to(torch.float32) / torch.clamp(total, min=1).to(torch.float32)
    return torch.where(total > 0, share, torch.zeros_like(share))


# ---- list quality: what finished lists look like ----------------------------------------------------------------------------------
def _check_list_quality_args(ids_shape, count_shape, category_shape, base_shape, base_count_shape):
    if len(ids_shape) != 2 or not 1 <= ids_shape[1] <= MMR_MAX_LIST:
        raise ValueError(f"ids must be [G, k] with 1 <= k <= {MMR_MAX_LIST}, got {tuple(ids_shape)}")
    if count_shape is not None and tuple(count_shape) != (ids_shape[0],):
        raise ValueError(f"count must have one entry per list ({ids_shape[0]}), got shape {tuple(count_shape)}")
    if category_shape is not None and len(category_shape) != 1:
        raise ValueError(f"category must be [N], got shape {tuple(category_shape)}")
    if base_shape is None and base_count_shape is not None:
        raise ValueError("base_count needs base_ids")
    if base_shape is not None:
        if len(base_shape) != 2 or base_shape[0] != ids_shape[0] or not 1 <= base_shape[1] <= MMR_MAX_LIST:
            raise ValueError(f"base_ids must be [G, kb] = [{ids_shape[0]}, 1 .. {MMR_MAX_LIST}], got {tuple(base_shape)}")
        if base_count_shape is not None and tuple(base_count_shape) != (ids_shape[0],):
            raise ValueError(f"base_count must have one entry per list ({ids_shape[0]}), got shape {tuple(base_count_shape)}")


def _news_num(named) -> Optional[int]:
    """The one N that the per-news arrays ``[(name, length or None)]`` agree on, or None when none is given."""
    given = [(name, int(n)) for name, n in named if n is not None]
    if len({n for _, n in given}) > 1:
        raise ValueError("the per-news arrays must have one entry per news, all of one N: got " + ", ".join(f"{name} {n}" for name, n in given))
    return given[0][1] if given else None


def list_quality_host(ids, count=None, sim=None, category=None, base_ids=None, base_count=None, news_num=None, exposure=None):
    """The contract of ``digat_list_quality`` in numpy — the yardstick of the kernel — on given similarities ``sim`` [G, k, k]
    float32 (as for ``mmr_select_host``).  ``ids`` [G, k], ``count`` [G] or None (k): position p is an element when
    ``p < clip(count[g], 0, k)`` and ``0 <= id < N`` (``news_num``; None: the length of ``category`` / ``exposure``, or no upper
    bound) — ``mmr_select_host``'s rule; a repeated id is one element per position it holds.  Returns a dict of numpy arrays, [G]
    each: ``elements`` int32; with ``sim``: ``sim_sum`` float64 — ``math.fsum`` of ``sim[g, p, q]`` over the element pairs p < q,
    the exactly rounded sum, 0.0 without a pair — and ``sim_max`` float32 — ``np.fmax`` over the same pairs from ``-inf`` (NaNs are
    passed over; a maximum of zero is ``+0.0``) —; with ``category`` [N] (any integers): ``categories`` and ``category_max`` int32,
    the distinct ``category[id]`` over the elements and the count of the most frequent one; with ``base_ids`` [G, kb] and
    ``base_count`` (elements by the same rule): ``overlap`` int32, the element positions whose id some element position of the
    user's base list holds; with ``exposure`` [N]: ``exposure``, a NEW int64 array — the input plus one per element position."""
    import math
    idv = np.asarray(ids, dtype=np.int64)
    cat = None if category is None else np.asarray(category, dtype=np.int64)
    base = None if base_ids is None else np.asarray(base_ids, dtype=np.int64)
    _check_list_quality_args(idv.shape, None if count is None else np.shape(count), None if cat is None else cat.shape,
                             None if base is None else base.shape, None if base_count is None else np.shape(base_count))
    G, k = idv.shape
    S = None if sim is None else np.asarray(sim, dtype=np.float32)
    if S is not None and S.shape != (G, k, k):
        raise ValueError(f"sim must be [G, k, k] = {(G, k, k)}, got {S.shape}")
    expo = None if exposure is None else np.array(exposure, dtype=np.int64)
    if expo is not None and expo.ndim != 1:
        raise ValueError(f"exposure must be [N], got shape {expo.shape}")
    N = _news_num([("news_num", news_num), ("category", None if cat is None else len(cat)), ("exposure", None if expo is None else len(expo))])

    def elements(v, c):
        n = v.shape[1]
        cnt = np.full(len(v), n, dtype=np.int64) if c is None else np.clip(np.asarray(c, dtype=np.int64), 0, n)
        el = (np.arange(n)[None, :] < cnt[:, None]) & (v >= 0)
        return el & (v < N) if N is not None else el
    el = elements(idv, count)
    out = {"elements": el.sum(axis=1).astype(np.int32)}
    if S is not None:
        out["sim_sum"], out["sim_max"] = np.zeros(G, dtype=np.float64), np.full(G, -np.inf, dtype=np.float32)
        for g in range(G):
            pair = np.triu(el[g][:, None] & el[g][None, :], 1)
            vals = S[g][pair]
            out["sim_sum"][g] = math.fsum(float(x) for x in vals)
            out["sim_max"][g] = np.fmax.reduce(vals, initial=np.float32(-np.inf)) + np.float32(0)
    if cat is not None:
        out["categories"], out["category_max"] = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
        for g in range(G):
            if el[g].any():
                n = np.unique(cat[idv[g][el[g]]], return_counts=True)[1]
                out["categories"][g], out["category_max"][g] = len(n), n.max()
    if base is not None:
        bel = elements(base, base_count)
        out["overlap"] = np.array([int(np.isin(idv[g][el[g]], base[g][bel[g]]).sum()) for g in range(G)], dtype=np.int32).reshape(G)
    if expo is not None:
        np.add.at(expo, idv[el], 1)
        out["exposure"] = expo
    return out


def list_quality(ids, count=None, vectors=None, category=None, base_ids=None, base_count=None, exposure=None):
    """What finished lists look like, on the GPU (``digat_list_quality``): per list its cosine diversity, category spread and
    overlap with the list before a second stage, and over all lists the catalogue's exposure.

    ``ids`` [G, k <= 128] int64 and ``count`` [G] int32 (None: k) are device tensors — what ``mmr_select``, ``topk_segments``,
    ``dot_topk`` and both ``recommend``s return.  Every part is optional and goes by its input: ``vectors`` [N, d] float32 (pass
    unit rows: ``util.unit_rows``) gives ``sim_sum`` float64 and ``sim_max`` float32 over the element pairs of the Gram
    ``mmr_select`` picks on; ``category`` [N] gives ``categories`` and ``category_max``; ``base_ids`` [G, kb <= 128] with
    ``base_count`` gives ``overlap``; ``exposure`` [N] int32 (contiguous, on the device) gets one more per element position, IN
    PLACE — it accumulates across calls, the caller zeroes it and keeps the counts inside int32 — and is returned too.  At least
    one of ``vectors`` / ``category`` / ``exposure`` is needed: they say how many news there are.  The contract is
    ``list_quality_host``'s: the integers exactly, ``sim_max`` by bits, ``sim_sum`` a double sum of the same float32 entries in a
    fixed order (bit-identical from run to run and in any batch).  Returns a dict of device tensors [G] (``elements`` always; a
    part that was not asked for has no key).  Stream-ordered: one launch, nothing is read back."""
    import torch
    from . import _lib
    given = [t for t in (ids, count, vectors, category, base_ids, base_count, exposure) if t is not None]
    dev = _lib.require_device(*given)
    _check_list_quality_args(tuple(ids.shape), None if count is None else tuple(count.shape), None if category is None else tuple(category.shape),
                             None if base_ids is None else tuple(base_ids.shape), None if base_count is None else tuple(base_count.shape))
    if vectors is not None and (vectors.dim() != 2 or vectors.shape[1] < 1):
        raise ValueError(f"vectors must be [N, d] with d >= 1, got {tuple(vectors.shape)}")
    if exposure is not None and (exposure.dim() != 1 or exposure.dtype != torch.int32 or not exposure.is_contiguous()):
        raise ValueError(f"exposure must be a contiguous [N] int32 tensor (it is updated in place), got {tuple(exposure.shape)} {exposure.dtype}")
    N = _news_num([("vectors", None if vectors is None else vectors.shape[0]), ("category", None if category is None else category.shape[0]),
                   ("exposure", None if exposure is None else exposure.shape[0])])
    if N is None:
        raise ValueError("list_quality needs vectors, category or exposure: one of them says how many news there are")
    idt = ids.to(torch.int64).contiguous()
    ct = None if count is None else count.to(torch.int32).contiguous()
    v = None if vectors is None else _lib.f32(vectors.detach())
    cat = None if category is None else category.to(torch.int32).contiguous()
    bt = None if base_ids is None else base_ids.to(torch.int64).contiguous()
    bc = None if base_count is None else base_count.to(torch.int32).contiguous()
    G, k, kb = int(idt.shape[0]), int(idt.shape[1]), 0 if bt is None else int(bt.shape[1])
    new = lambda dtype: torch.empty((G,), dtype=dtype, device=dev)
    out = {"elements": new(torch.int32)}
    if v is not None:
        out["sim_sum"], out["sim_max"] = new(torch.float64), new(torch.float32)
    if cat is not None:
        out["categories"], out["category_max"] = new(torch.int32), new(torch.int32)
    if bt is not None:
        out["overlap"] = new(torch.int32)
    if exposure is not None:
        out["exposure"] = exposure
    if G == 0:
        return out
    L = _lib.lib()
    need = int(L.digat_list_quality_workspace_bytes(G, k, kb))
    ws = _lib.workspace(need, dev, "list_quality")
    _lib.check(L.digat_list_quality(idt.data_ptr(), _lib.ptr(ct), G, k, N, _lib.ptr(v), 0 if v is None else int(v.shape[1]), _lib.ptr(cat),
                                    _lib.ptr(bt), _lib.ptr(bc), kb, _lib.ptr(exposure), out["elements"].data_ptr(), _lib.ptr(out.get("sim_sum")),
                                    _lib.ptr(out.get("sim_max")), _lib.ptr(out.get("categories")), _lib.ptr(out.get("category_max")),
                                    _lib.ptr(out.get("overlap")), ws.data_ptr(), need, _lib.stream_ptr()),
               "digat_list_quality")
    return out


def quality_summary(q, exposure=None, pool=None):
    """The figures of a ``list_quality`` / ``list_quality_host`` dict ``q`` over all its lists, in float64 on the host: ``ild`` —
    intra-list diversity, the mean over the lists with at least two elements of ``1 - sim_sum / (n (n - 1) / 2)`` —, ``max_sim`` —
    the mean of ``sim_max`` over the same lists —, ``categories`` — the mean distinct-category count —, ``category_max_share`` —
    the mean of ``category_max / elements`` over the non-empty lists —, ``overlap`` — the mean of ``overlap / elements`` over the
    non-empty lists —, and ``lists``, their number.  From ``exposure`` [N] (None: ``q["exposure"]`` where it has one) over ``pool``
    (ids; None: all N): ``coverage`` — the share of pool ids with exposure > 0 — and ``gini`` — on the ascending counts
    ``x_1 .. x_n``, ``2 sum(i x_i) / (n sum(x)) - (n + 1) / n``: 0 for equal exposure, ``(n - 1) / n`` when one id has it all.  A
    part ``q`` does not carry, and anything with nothing to average over, is NaN — as in ``rank_metrics``."""
    import torch
    host = lambda x: None if x is None else np.asarray(x.cpu() if torch.is_tensor(x) else x)
    nan = float("nan")
    mean = lambda x: float(np.mean(x)) if len(x) else nan
    el = host(q["elements"]).astype(np.float64)
    some, two = el > 0, el > 1
    out = {"lists": int(len(el)), "ild": nan, "max_sim": nan, "categories": nan, "category_max_share": nan, "overlap": nan,
           "coverage": nan, "gini": nan}
    if q.get("sim_sum") is not None:
        n = el[two]
        out["ild"] = mean(1.0 - host(q["sim_sum"]).astype(np.float64)[two] / (n * (n - 1.0) / 2.0))
        out["max_sim"] = mean(host(q["sim_max"]).astype(np.float64)[two])
    if q.get("categories") is not None:
        out["categories"] = mean(host(q["categories"]).astype(np.float64))
        out["category_max_share"] = mean(host(q["category_max"]).astype(np.float64)[some] / el[some])
    if q.get("overlap") is not None:
        out["overlap"] = mean(host(q["overlap"]).astype(np.float64)[some] / el[some])
    x = host(exposure if exposure is not None else q.get("exposure"))
    if x is not None:
        x = x.astype(np.float64)
        if pool is not None:
            x = x[np.unique(host(pool).astype(np.int64))]
        x = np.sort(x)
        n = len(x)
        if n:
            out["coverage"] = float((x > 0).sum()) / n
            if x.sum() > 0:
                out["gini"] = float(2.0 * (np.arange(1, n + 1) * x).sum() / (n * x.sum()) - (n + 1.0) / n)
    return out


BOOTSTRAP_MAX_COLUMNS = 16     # include/digat_hip.h: DIGAT_BOOTSTRAP_MAX_COLUMNS
BOOTSTRAP_SLICE = 8192         # ... DIGAT_BOOTSTRAP_SLICE, the draws one workgroup of digat_bootstrap_sums adds
BOOTSTRAP_MAX_REPLICATE = 1 << 31      # first_replicate + replicates may reach this
_BOOTSTRAP_WORKSPACE = 1 << 28         # bootstrap_sums splits a call whose slice partials would need more bytes than this
_M32 = np.uint64(0xFFFFFFFF)
METRIC_NAMES = ("auc", "mrr", "ndcg5", "ndcg10")      # the columns of impression_metrics


def _hash32(x: np.ndarray) -> np.ndarray:
    """csrc/digat_kernels.hip: hash32, on the low 32 bits of a uint64 array."""
    x = x & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def _is_tensor(x) -> bool:
    return hasattr(x, "detach") and hasattr(x, "is_cuda")         # a torch tensor, without importing torch


def _on_device(x) -> bool:
    return _is_tensor(x) and bool(x.is_cuda)


def _host(x) -> np.ndarray:
    return np.asarray(x.detach().cpu() if _is_tensor(x) else x)


def _check_bootstrap_args(n, c, replicates, first_replicate):
    if int(n) < 1:
        raise ValueError(f"values must have at least one row (a resampling unit), got n = {n}")
    if int(n) > (1 << 31) - 1:
        raise ValueError(f"values must have at most 2^31 - 1 rows, got n = {n}")
    if c is not None and not 1 <= int(c) <= BOOTSTRAP_MAX_COLUMNS:
        raise ValueError(f"values must have between 1 and BOOTSTRAP_MAX_COLUMNS = {BOOTSTRAP_MAX_COLUMNS} columns, got {c}")
    if int(replicates) != replicates or int(replicates) < 1:
        raise ValueError(f"replicates must be a positive integer, got {replicates}")
    if int(first_replicate) != first_replicate or int(first_replicate) < 0:
        raise ValueError(f"first_replicate must be a non-negative integer, got {first_replicate}")
    if int(first_replicate) + int(replicates) > BOOTSTRAP_MAX_REPLICATE:
        raise ValueError(f"first_replicate + replicates must not exceed 2^31, got {first_replicate} + {replicates}")


def bootstrap_draws_host(n: int, replicates: int, seed: int = 0, first_replicate: int = 0) -> np.ndarray:
    """The draws of ``digat_bootstrap_sums`` in numpy, bit for bit: ``idx`` [replicates, n] int64.  Replicate ``r = first_replicate
    + b`` draws n units with replacement; draw j has the 64-bit counter ``e = r n + j``, the word ``w = hash32((uint32)e *
    0x9E3779B9 + hash32(seed + (uint32)(e >> 32)))`` (``drop_keep``'s construction, the low 32 bits of ``seed`` used as given) and
    the unit ``(w n) >> 32``: uniform on [0, n) up to a bias of at most ``n / 2^32``."""
    _check_bootstrap_args(n, None, replicates, first_replicate)
    n64 = np.uint64(int(n))
    r = np.arange(int(first_replicate), int(first_replicate) + int(replicates), dtype=np.uint64)
    e = r[:, None] * n64 + np.arange(int(n), dtype=np.uint64)[None, :]
    inner = _hash32(np.uint64(int(seed) & 0xFFFFFFFF) + (e >> np.uint64(32)))
    w = _hash32((((e & _M32) * np.uint64(0x9E3779B9)) & _M32) + inner)
    return ((w * n64) >> np.uint64(32)).astype(np.int64)


def _value_matrix(values, name="values"):
    """``values`` as float64 [n, c] (a 1-D input is one column): a CUDA tensor stays one, everything else becomes numpy."""
    if _on_device(values):
        import torch
        v = values.detach()
        v = v.reshape(-1, 1) if v.dim() == 1 else v
        if v.dim() != 2 or not (v.is_floating_point() or v.dtype in (torch.int32, torch.int64, torch.uint8, torch.bool)):
            raise ValueError(f"{name} must be a real [n, c] array, got {tuple(values.shape)} {values.dtype}")
        return v if v.dtype == torch.float64 else v.to(torch.float64)
    v = _host(values)
    if v.dtype.kind not in "fiub":
        raise ValueError(f"{name} must be a real [n, c] array, got dtype {v.dtype}")
    v = v.astype(np.float64, copy=False)
    v = v.reshape(-1, 1) if v.ndim == 1 else v
    if v.ndim != 2:
        raise ValueError(f"{name} must be [n, c], got shape {v.shape}")
    return v


def bootstrap_sums_host(values, replicates: int, seed: int = 0, first_replicate: int = 0) -> np.ndarray:
    """The yardstick of ``bootstrap_sums``: ``sums`` [replicates, c] float64, ``sums[b, k]`` the CORRECTLY ROUNDED sum
    (``math.fsum``) of ``values[idx, k]`` over replicate b's draws ``bootstrap_draws_host`` gives.  ``values``: [n, c] (or [n])."""
    import math
    v = np.ascontiguousarray(_value_matrix(_host(values)))
    n, c = v.shape
    _check_bootstrap_args(n, c, replicates, first_replicate)
    B = int(replicates)
    out = np.empty((B, c), dtype=np.float64)
    per = max(1, (1 << 22) // n)
    for b0 in range(0, B, per):
        idx = bootstrap_draws_host(n, min(per, B - b0), seed, int(first_replicate) + b0)
        for b in range(idx.shape[0]):
            rows = v[idx[b]]
            for k in range(c):
                out[b0 + b, k] = math.fsum(rows[:, k].tolist())
    return out


def bootstrap_sums(values, replicates: int, seed: int = 0, first_replicate: int = 0):
    """Bootstrap sums on the GPU (``digat_bootstrap_sums``): ``sums`` [replicates, c] float64 on the device of ``values`` [n, c]
    (or [n]: one column), ``sums[b, :]`` the sum of the n rows replicate ``first_replicate + b`` draws with replacement —
    ``bootstrap_draws_host``'s draws, one index per draw for every column.  ``values``: a device tensor of any real dtype and any
    strides, converted to contiguous float64 once (exactly, from float32 and the integers).  1 <= c <= 16, ``first_replicate +
    replicates <= 2^31``.  A column's sums depend on that column, n, ``seed`` and the replicate alone: the same bits from run to
    run, from a call split by ``first_replicate`` and from the columns split over two calls; against ``bootstrap_sums_host`` an
    entry is off by at most ``n 2^-53 sum |terms|`` and exact on integer-valued data below 2^53.  Stream-ordered: nothing is read
    back (a call whose slice partials would pass 256 MiB is split by replicates)."""
    import torch
    from . import _lib
    dev = _lib.require_device(values)
    v = _value_matrix(values).contiguous()
    n, c = int(v.shape[0]), int(v.shape[1])
    _check_bootstrap_args(n, c, replicates, first_replicate)
    B, r0 = int(replicates), int(first_replicate)
    sums = torch.empty((B, c), dtype=torch.float64, device=dev)
    L = _lib.lib()
    per_replicate = int(L.digat_bootstrap_workspace_bytes(n, c, 1))
    per = B if per_replicate == 0 else max(1, min(B, _BOOTSTRAP_WORKSPACE // per_replicate))
    need = per * per_replicate
    ws = _lib.workspace(need, dev, "bootstrap")
    for b0 in range(0, B, per):
        nb = min(per, B - b0)
        _lib.check(L.digat_bootstrap_sums(v.data_ptr(), n, c, nb, r0 + b0, int(seed) & 0xFFFFFFFF, sums.data_ptr() + b0 * c * 8,
                                          ws.data_ptr(), need, _lib.stream_ptr()),
                   "digat_bootstrap_sums")
    return sums


def _check_units(units, rows: int) -> np.ndarray:
    """``units`` — a CSR ``start`` over contiguous rows — as a host int64 array: [U + 1] offsets from 0 to ``rows`` that never decrease."""
    st = _host(units)
    if st.ndim != 1 or st.shape[0] < 1 or st.dtype.kind not in "iu":
        raise ValueError(f"start must be a 1-D integer array of units + 1 row offsets, got shape {st.shape} {st.dtype}")
    st = st.astype(np.int64)
    if st[0] != 0 or np.any(np.diff(st) < 0) or int(st[-1]) != rows:
        raise ValueError(f"start must begin at 0, never decrease and end at the number of rows ({rows})")
    return st


def segment_sums_host(values, start) -> np.ndarray:
    """``out`` [U, c] float64: ``out[u, :]`` the sum of the rows ``start[u] .. start[u+1] - 1`` of ``values`` [rows, c] (or [rows]),
    added left to right from 0.0 — the order of ``segment_sums``, so the same bits.  An empty unit gives 0."""
    v = _value_matrix(_host(values))
    st = _check_units(start, v.shape[0])
    length = np.diff(st)
    out = np.zeros((len(length), v.shape[1]), dtype=np.float64)
    for p in range(int(length.max()) if len(length) else 0):
        live = np.flatnonzero(length > p)
        out[live] += v[st[live] + p]
    return out


def segment_sums(values, start):
    """Row-level values turned into resampling units on the GPU (``digat_segment_sums_f64``): ``out`` [U, c] float64 on the device
    of ``values`` [rows, c] (or [rows]; any real dtype), ``out[u, :]`` the sum of the rows ``start[u] .. start[u+1] - 1`` added left
    to right (bit-identical to ``segment_sums_host``), 0 for an empty unit.  ``start`` [U + 1] is checked on the host (an array, or
    a tensor that is read back), then uploaded.  Stream-ordered otherwise: one launch."""
    import torch
    from . import _lib
    dev = _lib.require_device(values)
    v = _value_matrix(values).contiguous()
    rows, c = int(v.shape[0]), int(v.shape[1])
    if c < 1:
        raise ValueError("values must have at least one column")
    st = _check_units(start, rows)
    U = len(st) - 1
    out = torch.empty((U, c), dtype=torch.float64, device=dev)
    if U == 0:
        return out
    std = torch.from_numpy(st).to(dev)
    _lib.check(_lib.lib().digat_segment_sums_f64(v.data_ptr() if rows else None, rows, c, std.data_ptr(), U, out.data_ptr(), _lib.stream_ptr()),
               "digat_segment_sums_f64")
    return out


def impression_metrics(scores, row_impression, labels):
    """``[I, 4]`` float64: AUC, MRR, nDCG@5 and nDCG@10 of every impression (``METRIC_NAMES``) — the resampling units of a dev run.
    For CUDA ``scores`` [R] this is ``digat_rank_metrics``' own per-impression output, the array whose mean
    ``device_ranks_and_metrics`` reports, and it stays on the device; for host scores (an array or a CPU tensor) it is
    ``impression_metric_rows``, the values ``scoring`` averages.  Rows are impression-major; an impression without a positive or
    without a negative has a row that is not finite (``metric_intervals`` refuses it by its index)."""
    imp = np.asarray(row_impression, dtype=np.int64)
    if not _on_device(scores):
        return impression_metric_rows(labels, impression_ranks(_host(scores), imp), imp)
    import torch
    from . import _lib
    dev = _lib.require_device(scores)
    R = len(imp)
    if int(scores.shape[0]) != R or len(labels) != R:
        raise ValueError(f"scores, row_impression and labels must have one entry per row, got {int(scores.shape[0])}, {R} and {len(labels)}")
    if np.any(np.diff(imp) < 0):
        raise ValueError("rows must be impression-major")
    per = torch.empty((0, 4), dtype=torch.float64, device=dev)
    if R == 0:
        return per
    starts = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, R].astype(np.int64)
    I = len(starts) - 1
    sc = scores.detach().to(torch.float32).contiguous()
    st = torch.from_numpy(starts).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(np.asarray(labels) > 0).view(np.uint8)).to(dev)
    ranks = torch.empty(R, dtype=torch.int32, device=dev)
    per = torch.empty((I, 4), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().digat_rank_metrics(sc.data_ptr(), lab.data_ptr(), st.data_ptr(), I, ranks.data_ptr(), per.data_ptr(), None,
                                             _lib.stream_ptr()),
               "digat_rank_metrics")
    return per


def _check_level(level) -> float:
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie inside (0, 1), got {level}")
    return float(level)


def _check_finite(m, name):
    if _on_device(m):
        import torch
        bad = torch.nonzero(~torch.isfinite(m).all(dim=1))
        first = int(bad[0, 0]) if bad.numel() else None
    else:
        bad = np.flatnonzero(~np.isfinite(m).all(axis=1))
        first = int(bad[0]) if len(bad) else None
    if first is not None:
        raise ValueError(f"{name} must be finite: row {first} is not (an impression without a positive or without a negative has no "
                         "AUC / MRR / nDCG; leave such rows out)")


def _statistic_columns(values, denominators, units, name="values"):
    """What one set of columns hands the resampling: ``(matrix [n, cv + cd], cv, cd)`` — the value columns, then cd = 0 (the
    statistic divides by n), 1 (one denominator for every column) or cv denominator columns —, rows summed into ``units`` first;
    under ``units`` without ``denominators`` the unit's row count is the denominator."""
    v = _value_matrix(values, name)
    _check_finite(v, name)
    rows, cv = int(v.shape[0]), int(v.shape[1])
    dev = _on_device(v)
    parts, cd = [v], 0
    if denominators is not None:
        dname = "denominators" + name[len("values"):]
        d = _value_matrix(denominators, dname)
        if dev != _on_device(d):
            import torch
            d = torch.from_numpy(np.ascontiguousarray(d)).to(v.device) if dev else _host(d)
        cd = int(d.shape[1])
        if int(d.shape[0]) != rows or cd not in (1, cv):
            raise ValueError(f"{dname} must be [n] or [n, c] for {name} [{rows}, {cv}], got shape {tuple(d.shape)}")
        _check_finite(d, dname)
        parts.append(d)
    if dev:
        import torch
        m = torch.cat(parts, dim=1) if len(parts) > 1 else v
    else:
        m = np.concatenate(parts, axis=1) if len(parts) > 1 else v
    if units is not None:
        st = _check_units(units, rows)
        m = segment_sums(m, st) if dev else segment_sums_host(m, st)
        if denominators is None:
            count = np.diff(st).astype(np.float64)[:, None]
            if dev:
                import torch
                m = torch.cat([m, torch.from_numpy(count).to(m.device)], dim=1)
            else:
                m = np.concatenate([m, count], axis=1)
            cd = 1
    return m, cv, cd


def _resample(m, replicates, seed):
    """``(totals [c], sums [B, c])`` of a matrix, as host float64 arrays: device tensors through the kernel, numpy through its host twin."""
    if _on_device(m):
        total = m.sum(dim=0).cpu().numpy()
        return total, bootstrap_sums(m, replicates, seed).cpu().numpy()
    return np.array([np.sum(np.ascontiguousarray(m[:, k])) for k in range(m.shape[1])], dtype=np.float64), bootstrap_sums_host(m, replicates, seed)


def _statistics(total, sums, n, cv, cd):
    """The statistic of the data ([cv]) and of every replicate ([B, cv]) from the column totals and the replicate sums of one set."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if cd == 0:
            return total[:cv] / np.float64(n), sums[:, :cv] / np.float64(n)
        den, dens = (total[cv:cv + 1], sums[:, cv:cv + 1]) if cd == 1 else (total[cv:2 * cv], sums[:, cv:2 * cv])
        return total[:cv] / den, sums[:, :cv] / dens


def interval_fields(value, stats, level):
    """One column's entry of ``metric_intervals`` from its replicate statistics ``stats`` [B]: the percentile interval —
    ``numpy.quantile(stats, q, method="linear")`` at ``(1 - level) / 2`` and ``1 - (1 - level) / 2`` — and ``se``, their
    ``std(ddof=1)`` (NaN for one replicate)."""
    stats = np.asarray(stats, dtype=np.float64)
    alpha = (1.0 - _check_level(level)) / 2.0
    lo, hi = np.quantile(stats, [alpha, 1.0 - alpha], method="linear")
    se = float(np.std(stats, ddof=1)) if len(stats) > 1 else float("nan")
    return {"value": float(value), "lo": float(lo), "hi": float(hi), "se": se, "replicates": int(len(stats)), "level": float(level)}


def paired_fields(a, b, diffs, level):
    """One column's entry of ``compare_metrics`` from the replicate differences ``diffs`` [B] = ``stat_a* - stat_b*``: the
    percentile interval and ``se`` of ``interval_fields``, ``p = min(1, 2 min((#{d* <= 0} + 1) / (B + 1), (#{d* >= 0} + 1) /
    (B + 1)))`` — two-sided, never 0 — and ``wins``, the share of replicates with ``d* > 0``."""
    diffs = np.asarray(diffs, dtype=np.float64)
    B = len(diffs)
    f = interval_fields(float(a) - float(b), diffs, level)
    p = min(1.0, 2.0 * min((int((diffs <= 0).sum()) + 1) / (B + 1), (int((diffs >= 0).sum()) + 1) / (B + 1)))
    return {"a": float(a), "b": float(b), "diff": f["value"], "lo": f["lo"], "hi": f["hi"], "se": f["se"], "p": float(p),
            "wins": float((diffs > 0).sum()) / B}


def _column_names(names, c):
    names = tuple("column%d" % k for k in range(c)) if names is None else tuple(names)
    if len(names) != c or len(set(names)) != c:
        raise ValueError(f"names must give {c} different names, one per column, got {names}")
    return names


def metric_intervals(values, names=None, replicates: int = 2000, level: float = 0.95, seed: int = 0, denominators=None, units=None):
    """Bootstrap PERCENTILE intervals of the means this library reports: ``name -> {value, lo, hi, se, replicates, level}``.

    ``values`` [n, c] (or [n]) holds one row per resampling unit — ``impression_metrics``' rows, ``rank_metric_columns``' users —
    and the statistic of column k is ``sum(values[:, k]) / n``; with ``denominators`` ([n], shared, or [n, c]) it is
    ``sum(values[:, k]) / sum(denominators)``, a ratio of sums (recall over all targets).  ``units`` — a CSR ``start`` [U + 1] over
    contiguous rows — resamples whole units (a reader's impressions) instead of rows: the rows are summed per unit first
    (``segment_sums``), and without ``denominators`` a unit's row count is its denominator, so the statistic stays the mean over
    rows.  The unit is what the caller hands in: rows that belong to one reader are only kept together by ``units``.
    Each of the ``replicates`` draws n units with replacement (``bootstrap_draws_host``, ``seed``) and gives one replicate
    statistic; ``lo`` / ``hi`` are ``numpy.quantile(..., method="linear")`` of them at ``(1 - level) / 2`` and ``1 - (1 - level) /
    2``, ``se`` their ``std(ddof=1)``, ``value`` the statistic of the data itself.  CUDA tensors go through the kernel
    (``bootstrap_sums``), numpy arrays and CPU tensors through its host twin (``bootstrap_sums_host``) — the same draws, so the same
    result to the rounding of the sums.  Value and denominator columns together are at most 16.  Non-finite input is a
    ``ValueError`` that names the first bad row."""
    _check_level(level)
    m, cv, cd = _statistic_columns(values, denominators, units)
    names = _column_names(names, cv)
    n, c = int(m.shape[0]), int(m.shape[1])
    _check_bootstrap_args(n, c, replicates, 0)
    total, sums = _resample(m, int(replicates), seed)
    value, stats = _statistics(total, sums, n, cv, cd)
    return {name: interval_fields(value[k], stats[:, k], level) for k, name in enumerate(names)}


def compare_metrics(values_a, values_b, names=None, replicates: int = 2000, level: float = 0.95, seed: int = 0,
                    denominators_a=None, denominators_b=None, units=None):
    """Is the difference real?  The PAIRED bootstrap of two models scored on the same units: ``name -> {a, b, diff, lo, hi, se, p,
    wins}``.  ``values_a`` and ``values_b`` [n, c] hold the same units in the same order (``impression_metrics`` of two models on
    one dev set); both go through ONE resampling as ``[a | b]`` — one index per draw serves every column, so each replicate
    compares the two models on the same resampled units — and the replicate statistic is ``stat_a* - stat_b*``, the statistics
    being ``metric_intervals``' (``denominators_a`` / ``denominators_b`` and ``units`` as there).  ``a``, ``b``: the statistics of
    the data; ``diff = a - b``; ``lo`` / ``hi`` / ``se``: the percentile interval and standard error of the replicate differences;
    ``p``: the two-sided bootstrap p-value ``min(1, 2 min((#{d* <= 0} + 1) / (B + 1), (#{d* >= 0} + 1) / (B + 1)))``; ``wins``: the
    share of replicates with ``d* > 0``.  All columns of both sets together are at most 16 (c <= 8 each without denominators)."""
    _check_level(level)
    sa, sb = tuple(np.shape(values_a)), tuple(np.shape(values_b))
    if sa != sb:
        raise ValueError(f"values_a and values_b must have the same shape (the same units in the same order), got {sa} and {sb}")
    ma, cva, cda = _statistic_columns(values_a, denominators_a, units, "values_a")
    mb, cvb, cdb = _statistic_columns(values_b, denominators_b, units, "values_b")
    names = _column_names(names, cva)
    if _on_device(ma) != _on_device(mb):
        raise ValueError("values_a and values_b must both be device tensors or both be host arrays")
    if _on_device(ma):
        import torch
        m = torch.cat([ma, mb.to(ma.device)], dim=1)
    else:
        m = np.concatenate([ma, mb], axis=1)
    n, ca = int(m.shape[0]), int(ma.shape[1])
    if int(m.shape[1]) > BOOTSTRAP_MAX_COLUMNS:
        raise ValueError(f"values_a and values_b with their denominators have {int(m.shape[1])} columns together, at most "
                         f"BOOTSTRAP_MAX_COLUMNS = {BOOTSTRAP_MAX_COLUMNS} go through one resampling")
    _check_bootstrap_args(n, int(m.shape[1]), replicates, 0)
    total, sums = _resample(m, int(replicates), seed)
    a, stat_a = _statistics(total[:ca], sums[:, :ca], n, cva, cda)
    b, stat_b = _statistics(total[ca:], sums[:, ca:], n, cvb, cdb)
    return {name: paired_fields(a[k], b[k], stat_a[:, k] - stat_b[:, k], level) for k, name in enumerate(names)}


def rank_metric_columns(rank, target_start, ks=(10, 50, 100, 128)):
    """The per-user numerators and denominators ``rank_metrics``' averages are made of — what a bootstrap over users resamples.
    A dict of float64 arrays [U], one entry per user of ``target_start`` (a user without targets holds zeros): ``hits@k`` — the
    user's targets with ``0 <= rank < k`` —, ``targets`` — the user's target count —, ``share@k`` — ``hits@k / targets`` (0 without
    targets) —, ``rr`` — ``1 / (1 + best rank)``, 0 when none of the user's targets is ranked — and ``has`` — 1 for a user with a
    target.  ``recall@k = sum(hits@k) / sum(targets)``, ``user_recall@k = sum(share@k) / sum(has)`` and ``mrr = sum(rr) / sum(has)``
    reproduce ``rank_metrics`` to float64 rounding."""
    r = _host(rank).astype(np.int64)
    if r.ndim != 1:
        raise ValueError("rank must be 1-D")
    st = _host(target_start)
    if st.size == 0:
        st = np.zeros(1, dtype=np.int64)
    st = _check_target_start(st, len(st) - 1 if st.ndim == 1 else 0, len(r))
    per_user = np.diff(st)
    U = len(per_user)
    owner = np.repeat(np.arange(U), per_user)
    ranked = r >= 0
    have = per_user > 0
    out = {"targets": per_user.astype(np.float64), "has": have.astype(np.float64)}
    for k in ks:
        if int(k) != k or k < 1:
            raise ValueError(f"every k must be a positive integer, got {k}")
        hits = np.bincount(owner, weights=(ranked & (r < int(k))).astype(np.float64), minlength=U)
        out[f"hits@{int(k)}"] = hits
        out[f"share@{int(k)}"] = np.where(have, hits / np.maximum(per_user, 1), 0.0)
    best = np.full(U, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(best, owner[ranked], r[ranked])
    found = best != np.iinfo(np.int64).max
    out["rr"] = np.where(found, 1.0 / (1.0 + np.where(found, best, 0).astype(np.float64)), 0.0)
    return out


def rank_metrics_intervals(rank, target_start, ks=(10, 50, 100, 128), replicates: int = 2000, level: float = 0.95, seed: int = 0, device=None):
    """Percentile intervals of ``rank_metrics``' averages by a bootstrap over USERS (those with at least one target):
    ``{"recall@k", "user_recall@k", "mrr"} -> {value, lo, hi, se, replicates, level}`` — ``metric_intervals``' fields, every metric
    from the same draws (one resampling of ``rank_metric_columns``: ``recall@k`` as the ratio of summed hits to summed targets,
    the other two as means over users).  ``median_rank`` is not a sum over users and gets NO interval, nor do the counts.  At most 7
    values of k (2 k + 2 columns).  ``device``: a CUDA device runs the resampling on the GPU, None the host twin."""
    _check_level(level)
    ks = tuple(int(k) for k in ks)
    col = rank_metric_columns(rank, target_start, ks)
    keep = col["has"] > 0
    if 2 * len(ks) + 2 > BOOTSTRAP_MAX_COLUMNS:
        raise ValueError(f"ks: at most {(BOOTSTRAP_MAX_COLUMNS - 2) // 2} values of k go through one resampling, got {len(ks)}")
    m = np.stack([col[f"hits@{k}"][keep] for k in ks] + [col[f"share@{k}"][keep] for k in ks] + [col["rr"][keep], col["targets"][keep]], axis=1)
    n, K = int(m.shape[0]), len(ks)
    _check_bootstrap_args(n, int(m.shape[1]), replicates, 0)
    if device is not None:
        import torch
        m = torch.from_numpy(np.ascontiguousarray(m)).to(device)
    total, sums = _resample(m, int(replicates), seed)
    out = {}
    for i, k in enumerate(ks):
        out[f"recall@{k}"] = interval_fields(total[i] / total[-1], sums[:, i] / sums[:, -1], level)
        out[f"user_recall@{k}"] = interval_fields(total[K + i] / n, sums[:, K + i] / n, level)
    out["mrr"] = interval_fields(total[2 * K] / n, sums[:, 2 * K] / n, level)
    return out


# ---- stochastic lists: Plackett-Luce slates with their propensities ------------------------------------------------------------------
PL_MAX_LIST = SHORTLIST_MAX_K      # include/digat_hip.h: DIGAT_PL_MAX_LIST, the longest list digat_pl_sample / digat_pl_log_prob take
PL_MAX_K = TOPK_MAX_K              # ... DIGAT_PL_MAX_K, the longest slate
PL_MAX_SAMPLE = 1 << 22            # ... DIGAT_PL_MAX_SAMPLE: first_sample + samples may reach this (the sample shares a word with the position)
PL_CLAMP = -700.0                  # ... DIGAT_PL_CLAMP: a weight is exp(max(a - a_max, PL_CLAMP)), never 0
PL_ROBUST_GAP = 2.0 ** -40         # a robust slate's adjacent keys differ by this much of max(1, |key|) (pl_sample_host)
_FLT_MAX = float(np.finfo(np.float32).max)


def _check_pl_args(scores_shape, count_shape, k, temperature, samples=1, first_sample=0, streams_shape=None, picks_shape=None) -> float:
    """The argument checks ``pl_sample``, ``pl_log_prob`` and their host twins share; returns ``inv_t = 1.0 / float64(temperature)``."""
    if len(scores_shape) != 2 or not 1 <= scores_shape[1] <= PL_MAX_LIST:
        raise ValueError(f"scores must be [G, M] with 1 <= M <= PL_MAX_LIST = {PL_MAX_LIST}, got {tuple(scores_shape)}")
    G = int(scores_shape[0])
    if count_shape is not None and tuple(count_shape) != (G,):
        raise ValueError(f"count must have one entry per list ({G}), got shape {tuple(count_shape)}")
    if int(k) != k or not 1 <= int(k) <= PL_MAX_K:
        raise ValueError(f"k must be an integer in [1, {PL_MAX_K}], got {k}")
    t = float(temperature)
    if not 0.0 < t < float("inf"):                                  # a NaN fails both comparisons
        raise ValueError(f"temperature must be positive and finite, got {temperature}")
    inv_t = float(np.float64(1.0) / np.float64(t))
    if not inv_t * _FLT_MAX < float("inf"):
        raise ValueError(f"temperature {temperature} is too small: score / temperature must stay finite in float64")
    if int(samples) != samples or int(samples) < 1:
        raise ValueError(f"samples must be a positive integer, got {samples}")
    if int(first_sample) != first_sample or int(first_sample) < 0:
        raise ValueError(f"first_sample must be a non-negative integer, got {first_sample}")
    if int(first_sample) + int(samples) > PL_MAX_SAMPLE:
        raise ValueError(f"first_sample + samples must not exceed PL_MAX_SAMPLE = 2^22, got {first_sample} + {samples}")
    if streams_shape is not None and tuple(streams_shape) != (G,):
        raise ValueError(f"streams must have one entry per list ({G}), got shape {tuple(streams_shape)}")
    if picks_shape is not None and (len(picks_shape) != 3 or picks_shape[0] != G or picks_shape[2] != int(k) or picks_shape[1] < 1):
        raise ValueError(f"picks must be [G = {G}, S >= 1, k = {int(k)}], got {tuple(picks_shape)}")
    return inv_t


def _check_streams_host(streams, G: int) -> np.ndarray:
    if streams is None:
        return np.arange(G, dtype=np.uint64)
    st = np.asarray(_host(streams))
    if st.dtype.kind not in "iu" or st.ndim != 1:
        raise ValueError(f"streams must be a 1-D integer array, got {st.dtype} {st.shape}")
    if st.size and (int(st.min()) < 0 or int(st.max()) >= 1 << 32):
        raise ValueError("every stream must lie in [0, 2^32)")
    return st.astype(np.uint64)


def pl_draws_host(streams, samples: int, M: int, seed: int = 0, first_sample: int = 0) -> np.ndarray:
    """The uniform word behind every (list, sample, position) of ``digat_pl_sample``, bit for bit: ``w`` [G, S, M] uint32.  The 64-bit
    counter is ``e = (streams[g] << 32) | ((first_sample + s) << 10 | p)`` and the word ``hash32((uint32)e * 0x9E3779B9 +
    hash32(seed + (uint32)(e >> 32)))`` — ``bootstrap_draws_host``'s construction —: a pure function of (seed, stream, sample,
    position), the same for a list alone or in a batch and in a call split by ``first_sample``.  ``streams`` [G]: 32-bit ids the
    caller gives (an impression, a user); ``M <= 1024``, ``first_sample + samples <= 2^22``."""
    st = np.asarray(_host(streams))
    _check_pl_args((len(st), int(M)), None, 1, 1.0, samples, first_sample, st.shape)
    st = _check_streams_host(st, len(st))
    s = np.arange(int(first_sample), int(first_sample) + int(samples), dtype=np.uint64)
    low = (s[:, None] << np.uint64(10)) | np.arange(int(M), dtype=np.uint64)[None, :]                 # [S, M] < 2^32
    inner = _hash32(np.uint64(int(seed) & 0xFFFFFFFF) + st)                                         # [G]
    w = _hash32((((low * np.uint64(0x9E3779B9)) & _M32)[None, :, :] + inner[:, None, None]))
    return w.astype(np.uint32)


def _pl_lists_host(scores, count, inv_t):
    """``(scores float32 [G, M], live bool [G, M], a float64 [G, M])`` of the host twins: ``a = float64(x) * inv_t`` where live."""
    sc = np.ascontiguousarray(_host(scores), dtype=np.float32)
    G, M = sc.shape
    cnt = np.full(G, M, dtype=np.int64) if count is None else np.clip(np.asarray(_host(count), dtype=np.int64), 0, M)
    live = (np.arange(M)[None, :] < cnt[:, None]) & np.isfinite(sc)
    a = np.where(live, sc, np.float32(0)).astype(np.float64) * np.float64(inv_t)
    return sc, live, a


def _pl_slate_host(a, live, picks, k, values=None):
    """The probability stage of one list for one slate: ``(logp, step64 [k], logZ [k], length)`` — the slate is ``picks`` up to its
    first entry that is negative, out of range, not live or repeated.  With ``values`` [M] float64 (``pl_expect_host``) three
    arrays [k] follow: ``mean[t] = fsum(w v over what is left at t) / Z_t``, every product rounded once, ``absolute[t]`` the same
    over ``|v|``, and ``used[t]`` the value of pick t."""
    import math
    M = len(a)
    step, logz = np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
    extra = () if values is None else tuple(np.zeros(k, dtype=np.float64) for _ in range(3))
    if not live.any():
        return (0.0, step, logz, 0) + extra
    d = np.maximum(a - a[live].max(), PL_CLAMP)
    w = np.exp(d)
    left = live.copy()
    n = 0
    for p in picks[:k]:
        p = int(p)
        if p < 0 or p >= M or not left[p]:
            break
        z = np.float64(math.fsum(w[left].tolist()))
        logz[n] = np.log(z)
        step[n] = d[p] - logz[n]
        if values is not None:
            wv = w[left] * values[left]
            extra[0][n] = np.float64(math.fsum(wv.tolist())) / z
            extra[1][n] = np.float64(math.fsum(np.abs(wv).tolist())) / z
            extra[2][n] = values[p]
        left[p] = False
        n += 1
    return (math.fsum(step[:n].tolist()), step, logz, n) + extra


def pl_sample_host(scores, count, k: int, temperature, seed: int = 0, samples: int = 1, first_sample: int = 0, streams=None,
                   return_robust: bool = False, parts: bool = False):
    """The contract of ``digat_pl_sample`` in numpy — the sampler's yardstick.  ``scores`` [G, M <= 1024] float32, ``count`` [G] or
    None (M): position p of list g is LIVE when ``p < clip(count[g], 0, M)`` and ``scores[g, p]`` is finite; ``-inf``, ``+inf`` and
    NaN carry no mass and are never drawn.  In float64, every operation rounded: ``inv_t = 1.0 / float64(temperature)``, ``a_p =
    float64(x_p) * inv_t``, ``u = (w + 0.5) * 2^-32`` (exact) with ``w`` the word of ``pl_draws_host``, ``key_p = a_p +
    (-log(-log(u)))`` — a Gumbel key: the live positions in descending key order are a draw without replacement from
    ``softmax(score / temperature)``, a Plackett-Luce slate.  Ties go to the lowest position; the slate is cut to ``n_out = min(k,
    live)``, ``1 <= k <= 128``.  Its probability: ``a_max`` the largest live ``a``, ``w_p = exp(max(a_p - a_max, -700))`` (the clamp
    keeps every ``Z`` positive whatever the spread; while an unpicked entry lies within 700 of ``a_max`` its effect on a step is
    below e^-700 — once the slate has used up all of those, the entries left sit on the clamp together and the step reported is
    the uniform one over them: keep ``k`` gaps of ``score / temperature`` below 700 where the tail's propensity matters), ``Z_t`` the sum (``math.fsum``) of
    ``w`` over the live positions not picked before step t, ``step[t] = max(a_pick(t) - a_max, -700) - log(Z_t)`` and ``logp`` the
    ``fsum`` of the steps.

    Returns ``(picks [G, S, k] int32 — positions, -1 beyond n_out —, n_out [G] int32, logp [G, S] float64, step_logp [G, S, k]
    float32 — 0 beyond n_out)``; the ``logp`` of an empty slate is 0.  ``streams`` [G] (None: ``g``), ``seed``, ``samples`` and
    ``first_sample`` are ``pl_draws_host``'s.

    ``return_robust`` adds [G] bool: a list is robust when, in every sample, every adjacent pair among its top ``n_out + 1`` keys
    is separated by at least ``2^-40 max(1, |key|)``.  Two float64 logarithms correct to 1 ulp move a key by at most a few
    ``2^-52 max(1, |key|)``, so on a robust list every such implementation draws the same slate.  ``parts`` adds a dict with the
    float64 ``step`` and ``logZ`` [G, S, k] and ``live`` [G] (what ``pl_bound`` takes)."""
    inv_t = _check_pl_args(np.shape(scores), None if count is None else np.shape(count), k, temperature, samples, first_sample,
                           None if streams is None else np.shape(streams))
    sc, live, a = _pl_lists_host(scores, count, inv_t)
    (G, M), k, S = sc.shape, int(k), int(samples)
    words = pl_draws_host(_check_streams_host(streams, G), S, M, seed, first_sample)
    with np.errstate(divide="ignore"):
        gumbel = -np.log(-np.log((words.astype(np.float64) + 0.5) * 2.0 ** -32))
    key = a[:, None, :] + gumbel
    picks = np.full((G, S, k), -1, dtype=np.int32)
    n_out = np.minimum(live.sum(axis=1), k).astype(np.int32)
    logp = np.zeros((G, S), dtype=np.float64)
    step = np.zeros((G, S, k), dtype=np.float64)
    logz = np.zeros((G, S, k), dtype=np.float64)
    robust = np.ones(G, dtype=bool)
    for g in range(G):
        pos = np.flatnonzero(live[g])
        n = int(n_out[g])
        for s in range(S):
            kg = key[g, s, pos]
            order = np.argsort(-kg, kind="stable")                  # descending key, equal keys by position
            picks[g, s, :n] = pos[order[:n]]
            top = kg[order[:n + 1]]
            if len(top) > 1 and np.any(top[:-1] - top[1:] < PL_ROBUST_GAP * np.maximum(1.0, np.maximum(np.abs(top[:-1]), np.abs(top[1:])))):
                robust[g] = False
            logp[g, s], step[g, s], logz[g, s], _ = _pl_slate_host(a[g], live[g], picks[g, s], k)
    out = (picks, n_out, logp, step.astype(np.float32))
    if return_robust:
        out += (robust,)
    if parts:
        out += ({"step": step, "logZ": logz, "live": live.sum(axis=1)},)
    return out


def pl_log_prob_host(scores, count, picks, temperature, parts: bool = False):
    """``pl_sample_host``'s ``logp`` [G, S] float64 and ``step_logp`` [G, S, k] float32 for GIVEN slates — the probability of a logged
    slate under another model's scores.  ``picks`` [G, S, k] holds positions; a slate ends at its first entry that is negative, out
    of range, not live or repeated (``step_logp`` is 0 from there on).  ``parts`` adds the dict of ``pl_sample_host`` with the
    slates' lengths ``length`` [G, S]."""
    pk = np.asarray(_host(picks))
    if pk.dtype.kind not in "iu":
        raise ValueError(f"picks must hold integer positions, got {pk.dtype}")
    k = int(pk.shape[2]) if pk.ndim == 3 else 0
    inv_t = _check_pl_args(np.shape(scores), None if count is None else np.shape(count), k, temperature, picks_shape=pk.shape)
    sc, live, a = _pl_lists_host(scores, count, inv_t)
    G, S = sc.shape[0], int(pk.shape[1])
    logp = np.zeros((G, S), dtype=np.float64)
    step = np.zeros((G, S, k), dtype=np.float64)
    logz = np.zeros((G, S, k), dtype=np.float64)
    length = np.zeros((G, S), dtype=np.int32)
    for g in range(G):
        for s in range(S):
            logp[g, s], step[g, s], logz[g, s], length[g, s] = _pl_slate_host(a[g], live[g], pk[g, s], k)
    out = (logp, step.astype(np.float32))
    return out + ({"step": step, "logZ": logz, "live": live.sum(axis=1), "length": length},) if parts else out


def pl_bound(n, logZ, value=None, float32: bool = False, total: bool = False):
    """The comparison bound of ``pl_sample`` / ``pl_log_prob`` against their host twins (derived in csrc/digat_pl_sample.inc).  Per
    step: ``(n + 16) 2^-53 (1 + |log Z_t|)`` — n the live elements of the list: the order of the n positive terms of ``Z_t`` and the
    few ulps of ``exp`` and ``log`` on either side — plus, with the step's ``value``, ``2^-52 |value|``: both sides round the final
    difference, and two numbers that close may round to neighbours; ``float32`` adds ``2^-23 |value|`` for a ``step_logp`` compared
    as float32 (one float32 rounding on either side).  ``total``: the bound of ``logp`` — the step bounds summed over the last axis
    plus ``(k + 1) 2^-53 sum |value|``, the device adding the steps in slate order where the twin adds them exactly."""
    n = np.asarray(n, dtype=np.float64)
    lz = np.abs(np.asarray(logZ, dtype=np.float64))
    b = (n + 16.0) * 2.0 ** -53 * (1.0 + lz)
    if value is None:
        return b
    v = np.abs(np.asarray(value, dtype=np.float64))
    b = b + 2.0 ** -52 * v + (2.0 ** -23 * v if float32 else 0.0)
    if total:
        return b.sum(axis=-1) + (b.shape[-1] + 1) * 2.0 ** -53 * v.sum(axis=-1)
    return b


def _pl_device_args(scores, count, streams=None):
    import torch
    from . import _lib
    given = [t for t in (scores, count, streams) if t is not None]
    dev = _lib.require_device(*given)
    sc = _lib.f32(scores.detach())
    ct = None if count is None else count.to(torch.int32).contiguous()
    st = None if streams is None else streams.to(torch.int64).contiguous()
    return dev, sc, ct, st


def pl_sample(scores, count, k: int, temperature, seed: int = 0, samples: int = 1, first_sample: int = 0, streams=None):
    """Plackett-Luce slates on the GPU (``digat_pl_sample``): per list and sample, k positions drawn without replacement from
    ``softmax(scores / temperature)`` over the list's live positions, and the probability of what was drawn.  ``scores`` [G, M <=
    1024] float32 and ``count`` [G] int32 (None: M) are device tensors — what ``shortlist_segments``, ``dot_shortlist``,
    ``score_lists`` and both ``recommend``s return —, ``streams`` [G] an integer device tensor of 32-bit ids (its low 32 bits are
    used; None: the list's index).  The contract is ``pl_sample_host``'s: the same picks on its robust lists, ``logp`` and
    ``step_logp`` within ``pl_bound``.  Returns ``(picks [G, S, k] int32, n_out [G] int32, logp [G, S] float64, step_logp [G, S, k]
    float32)`` on the device.  A draw is a pure function of (seed, stream, sample, position) and every order of addition is fixed by
    the list and the slate: the same bits from run to run, for a list alone or in a batch, and from a call split by
    ``first_sample``.  Stream-ordered: nothing is read back."""
    import torch
    from . import _lib
    dev, sc, ct, st = _pl_device_args(scores, count, streams)
    inv_t = _check_pl_args(tuple(sc.shape), None if ct is None else tuple(ct.shape), k, temperature, samples, first_sample,
                           None if st is None else tuple(st.shape))
    G, M, k, S = int(sc.shape[0]), int(sc.shape[1]), int(k), int(samples)
    picks = torch.empty((G, S, k), dtype=torch.int32, device=dev)
    n_out = torch.empty((G,), dtype=torch.int32, device=dev)
    logp = torch.empty((G, S), dtype=torch.float64, device=dev)
    step = torch.empty((G, S, k), dtype=torch.float32, device=dev)
    if G == 0:
        return picks, n_out, logp, step
    L = _lib.lib()
    need = int(L.digat_pl_sample_workspace_bytes(G, M, k, S))
    ws = _lib.workspace(need, dev, "pl_sample")
    _lib.check(L.digat_pl_sample(sc.data_ptr(), _lib.ptr(ct), G, M, k, inv_t, int(seed) & 0xFFFFFFFF, S, int(first_sample), _lib.ptr(st),
                                 picks.data_ptr(), n_out.data_ptr(), logp.data_ptr(), step.data_ptr(), ws.data_ptr(), need,
                                 _lib.stream_ptr()), "digat_pl_sample")
    return picks, n_out, logp, step


def pl_log_prob(scores, count, picks, temperature):
    """The probability of GIVEN slates on the GPU (``digat_pl_log_prob``): ``(logp [G, S] float64, step_logp [G, S, k] float32)`` of
    ``picks`` [G, S, k] (integer positions; a slate ends at its first entry that is negative, out of range, not live or repeated)
    under ``softmax(scores / temperature)`` — ``pl_log_prob_host``'s contract within ``pl_bound``.  The kernel runs the sampler's own
    probability stage: on ``pl_sample``'s picks, with its scores and temperature, both outputs are the sampler's bit for bit."""
    import torch
    from . import _lib
    dev, sc, ct, _ = _pl_device_args(scores, count)
    _lib.require_device(sc, picks)
    if picks.is_floating_point() or picks.dtype == torch.bool:
        raise ValueError(f"picks must hold integer positions, got {picks.dtype}")
    k = int(picks.shape[2]) if picks.dim() == 3 else 0
    inv_t = _check_pl_args(tuple(sc.shape), None if ct is None else tuple(ct.shape), k, temperature, picks_shape=tuple(picks.shape))
    pk = torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()       # any position outside the list ends the slate
    G, M, S = int(sc.shape[0]), int(sc.shape[1]), int(pk.shape[1])
    logp = torch.empty((G, S), dtype=torch.float64, device=dev)
    step = torch.empty((G, S, k), dtype=torch.float32, device=dev)
    if G == 0:
        return logp, step
    L = _lib.lib()
    need = int(L.digat_pl_sample_workspace_bytes(G, M, k, S))
    ws = _lib.workspace(need, dev, "pl_sample")
    _lib.check(L.digat_pl_log_prob(sc.data_ptr(), _lib.ptr(ct), G, M, k, inv_t, S, pk.data_ptr(), logp.data_ptr(), step.data_ptr(),
                                   ws.data_ptr(), need, _lib.stream_ptr()), "digat_pl_log_prob")
    return logp, step


# ---- the per-step expectation behind a doubly robust off-policy value: csrc/digat_pl_expect.inc ----------------------------------
def _check_values_shape(values_shape, scores_shape) -> None:
    if tuple(values_shape) != tuple(scores_shape):
        raise ValueError(f"values must hold one value per item of every list, {tuple(scores_shape)}, got {tuple(values_shape)}")


def pl_expect_host(scores, count, picks, values, temperature, parts: bool = False):
    """The contract of ``digat_pl_expect`` in numpy float64 — ``pl_log_prob_host`` with, for every step t of a slate, the expectation
    of a per-item value under the conditional distribution that step draws from.  ``values`` [G, M] float32: ``v_p =
    float64(values[g, p])`` where that is finite, else 0.  With ``w`` and ``Z_t`` as in ``pl_sample_host`` and ``left`` the live
    positions not picked before step t: ``step_mean[t] = fsum(w[left] * v[left]) / Z_t``, every product rounded once, and
    ``step_value[t]`` the float32 value used at pick t.  Returns ``(logp [G, S] float64, step_logp [G, S, k] float32, step_mean
    [G, S, k] float64, step_value [G, S, k] float32, length [G, S] int32)`` — the first two are ``pl_log_prob_host``'s, ``length``
    is the slate's cut, and everything is 0 at and beyond it.  ``parts`` adds ``pl_log_prob_host``'s dict with ``absolute`` [G, S, k]:
    ``A_t = fsum(w[left] * |v[left]|) / Z_t``, what ``pl_expect_bound`` takes."""
    pk = np.asarray(_host(picks))
    if pk.dtype.kind not in "iu":
        raise ValueError(f"picks must hold integer positions, got {pk.dtype}")
    k = int(pk.shape[2]) if pk.ndim == 3 else 0
    inv_t = _check_pl_args(np.shape(scores), None if count is None else np.shape(count), k, temperature, picks_shape=pk.shape)
    _check_values_shape(np.shape(values), np.shape(scores))
    sc, live, a = _pl_lists_host(scores, count, inv_t)
    v32 = np.ascontiguousarray(_host(values), dtype=np.float32)
    v32 = np.where(np.isfinite(v32), v32, np.float32(0))
    v = v32.astype(np.float64)
    G, S = sc.shape[0], int(pk.shape[1])
    logp = np.zeros((G, S), dtype=np.float64)
    length = np.zeros((G, S), dtype=np.int32)
    step, logz, mean, absolute, used = (np.zeros((G, S, k), dtype=np.float64) for _ in range(5))
    for g in range(G):
        for s in range(S):
            logp[g, s], step[g, s], logz[g, s], length[g, s], mean[g, s], absolute[g, s], used[g, s] = _pl_slate_host(
                a[g], live[g], pk[g, s], k, v[g])
    out = (logp, step.astype(np.float32), mean, used.astype(np.float32), length)
    if parts:
        out += ({"step": step, "logZ": logz, "live": live.sum(axis=1), "length": length, "absolute": absolute},)
    return out


def pl_expect_bound(n, absolute, mean):
    """The comparison bound of ``pl_expect``'s ``step_mean`` against ``pl_expect_host`` (derived in csrc/digat_pl_expect.inc): ``(2 n +
    12) 2^-53 A_t + 2^-52 |mean|`` with n the live elements of the list and ``A_t = sum w |v| / Z_t`` (``absolute`` of the twin's
    parts).  ``(n + 6) 2^-53 A_t`` is the numerator — the 1-ulp ``exp`` on either side, one rounding per product on either side,
    the twin's ``fsum`` and the order of the device's at most n signed terms —, ``(n + 4) 2^-53 |mean| <= (n + 4) 2^-53 A_t`` the sum
    in ``Z_t`` (``pl_bound``'s), 2 of the 12 cover every term of second order at n <= 1024, and ``2^-52 |mean|`` is the division
    rounded on either side.  It holds while every non-zero product ``w |v|`` is a normal float64: ``|v| >= 2^-12`` or 0 is enough
    whatever the spread of the scores (a weight is at least e^-700)."""
    n = np.asarray(n, dtype=np.float64)
    return (2.0 * n + 12.0) * 2.0 ** -53 * np.abs(np.asarray(absolute, dtype=np.float64)) + 2.0 ** -52 * np.abs(np.asarray(mean, dtype=np.float64))


def pl_expect(scores, count, picks, values, temperature):
    """The per-step expectation of a per-item value under the target policy on the GPU (``digat_pl_expect``) — the control variate
    of a doubly robust off-policy value (``off_policy_steps``).  ``scores`` [G, M <= 1024], ``count`` and ``picks`` [G, S, k] as in
    ``pl_log_prob``; ``values`` [G, M] a floating-point device tensor (read as float32; a non-finite value counts as 0).  Returns
    ``(logp [G, S] float64, step_logp [G, S, k] float32, step_mean [G, S, k] float64, step_value [G, S, k] float32, length [G, S]
    int32)`` on the device: ``logp`` and ``step_logp`` are ``pl_log_prob``'s bit for bit (the same device function on the same
    image), ``length`` the slate's cut, ``step_value`` the value used at every pick and ``step_mean[t]`` the expectation of the
    value over what is left of the list at step t — ``pl_expect_host``'s contract, within ``pl_expect_bound``; 0 at and beyond
    ``length``.  One workgroup per (list, slate), one more suffix sum beside ``Z_t``: the same bits from run to run and for a list
    alone or in a batch.  Stream-ordered: nothing is read back."""
    import torch
    from . import _lib
    dev, sc, ct, _ = _pl_device_args(scores, count)
    _lib.require_device(sc, picks, values)
    if picks.is_floating_point() or picks.dtype == torch.bool:
        raise ValueError(f"picks must hold integer positions, got {picks.dtype}")
    if not values.is_floating_point():
        raise ValueError(f"values must be a floating-point tensor, got {values.dtype}")
    k = int(picks.shape[2]) if picks.dim() == 3 else 0
    inv_t = _check_pl_args(tuple(sc.shape), None if ct is None else tuple(ct.shape), k, temperature, picks_shape=tuple(picks.shape))
    _check_values_shape(tuple(values.shape), tuple(sc.shape))
    pk = torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()       # any position outside the list ends the slate
    vl = values.detach().to(torch.float32).contiguous()
    G, M, S = int(sc.shape[0]), int(sc.shape[1]), int(pk.shape[1])
    logp = torch.empty((G, S), dtype=torch.float64, device=dev)
    step = torch.empty((G, S, k), dtype=torch.float32, device=dev)
    mean = torch.empty((G, S, k), dtype=torch.float64, device=dev)
    used = torch.empty((G, S, k), dtype=torch.float32, device=dev)
    length = torch.empty((G, S), dtype=torch.int32, device=dev)
    if G == 0:
        return logp, step, mean, used, length
    L = _lib.lib()
    need = int(L.digat_pl_sample_workspace_bytes(G, M, k, S))
    ws = _lib.workspace(need, dev, "pl_sample")
    _lib.check(L.digat_pl_expect(sc.data_ptr(), _lib.ptr(ct), G, M, k, inv_t, S, pk.data_ptr(), vl.data_ptr(), logp.data_ptr(), step.data_ptr(),
                                 mean.data_ptr(), used.data_ptr(), length.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()),
               "digat_pl_expect")
    return logp, step, mean, used, length


# ---- the differentiable Plackett-Luce slate likelihood over a user's own list: csrc/digat_list_pl.inc -----------------------------
def _pl_inv_t(scale, temperature) -> float:
    """``inv_t = fl(float64(scale) * fl(1.0 / float64(temperature)))`` of ``list_pl``, checked: what the kernels multiply a score by."""
    t, s = float(temperature), float(scale)
    if not 0.0 < t < float("inf"):                                  # a NaN fails both comparisons
        raise ValueError(f"temperature must be positive and finite, got {temperature}")
    if not 0.0 < s < float("inf"):
        raise ValueError(f"scale must be positive and finite, got {scale}")
    with np.errstate(over="ignore"):
        inv_t = float(np.float64(s) * (np.float64(1.0) / np.float64(t)))
    if not (inv_t > 0.0 and inv_t * _FLT_MAX < float("inf")):
        raise ValueError(f"scale / temperature = {scale} / {temperature} must stay positive and keep score * scale / temperature finite in float64")
    return inv_t


def _list_pl_host_parts(scores, ids, count, picks, rows_num, inv_t):
    sc = np.array(_host(scores), dtype=np.float32)
    if sc.ndim != 2:
        raise ValueError("scores must be [G, M]")
    G, M = sc.shape
    pk = np.asarray(_host(picks))
    if pk.dtype.kind not in "iu":
        raise ValueError(f"picks must hold integer positions, got {pk.dtype}")
    k = int(pk.shape[2]) if pk.ndim == 3 else 0
    _check_pl_args(sc.shape, None if count is None else np.shape(count), k, 1.0, picks_shape=pk.shape)
    if ids is not None:
        I = np.asarray(_host(ids))
        if I.shape != (G, M) or I.dtype.kind not in "iu":
            raise ValueError(f"ids must be an integer array of shape {(G, M)}, got {I.shape} {I.dtype}")
        sc[~((I >= 0) & (I < int(rows_num)))] = np.nan                # no element: no mass
    sc, live, a = _pl_lists_host(sc, count, inv_t)
    return sc, live, a, pk, k


def _pl_slate_grad_host(a, live, picks, n):
    """``(dlogp / da [M], 1[j in the slate] + w_j H_n [M])`` of one slate of length ``n`` (``_pl_slate_host``'s), float64."""
    import math
    M = len(a)
    dl, ab = np.zeros(M), np.zeros(M)
    if n == 0:
        return dl, ab
    w = np.where(live, np.exp(np.maximum(a - a[live].max(), PL_CLAMP)), 0.0)
    left = live.copy()
    recip = []
    for t in range(n):
        p = int(picks[t])
        recip.append(1.0 / np.float64(math.fsum(w[left].tolist())))
        dl[p] = 1.0 - w[p] * np.float64(math.fsum(recip))
        ab[p] = 1.0
        left[p] = False
    Hn = np.float64(math.fsum(recip))
    dl[left] = -(w[left] * Hn)
    ab += w * Hn
    return dl, ab


def list_pl_host(scores, ids, count, picks, rows_num, scale=1.0, temperature=1.0, grad_logp=None, parts: bool = False):
    """The contract of ``digat_list_pl_fwd`` and of the coefficient kernel on given scores ``scores`` [G, M] float32 (slot (g, j) holds
    the inner product of user g with row ``ids[g, j]``), in numpy float64 with ``math.fsum`` — the yardstick of the kernels.  A slot
    is an element when ``j < clip(count[g], 0, M)`` and ``0 <= ids[g, j] < rows_num`` (``ids`` None: the first condition alone —
    ``pl_scores``' rule); a position is LIVE when it is an element and its score is finite.  ``a = float64(score) * inv_t`` with
    ``inv_t = float64(scale) * (1.0 / float64(temperature))``; from there on ``logp`` [G, S] float64 and ``step_logp`` [G, S, k]
    float32 are ``pl_log_prob_host``'s on ``a`` — the slates' cut rule, the clamp at -700, the ``fsum`` suffix sums, 0 for an empty
    slate.  With ``grad_logp`` [G, S] the float64 ``coef`` [G, M] is returned too: ``w_j = exp(max(a_j - a_max, -700))``, ``Z_t`` the
    ``fsum`` of ``w`` over the live positions not picked before step t, ``H_t = sum_{u < t} 1 / Z_u``, n the slate's length,
    ``dlogp / da_j = -w_j H_n`` (live, not in the slate), ``1 - w_j H_{t+1}`` (``j = picks[t]``), 0 (not live) — ``a_max`` and the
    clamp held constant — and ``coef[g, j] = inv_t * fsum_s(grad_logp[g, s] * dlogp_s / da_j)``; a slate that is empty or whose
    ``grad_logp`` is 0 adds nothing.  ``parts`` adds a dict: ``logZ`` and ``step`` [G, S, k] float64, ``live`` [G], ``length`` [G, S]
    and, with ``grad_logp``, ``absolute`` [G, M] = ``|inv_t| sum_s |grad_logp[g, s]| (1[j in slate s] + w_j H_n)``, what
    ``list_pl_bound`` takes."""
    import math
    inv_t = _pl_inv_t(scale, temperature)
    sc, live, a, pk, k = _list_pl_host_parts(scores, ids, count, picks, rows_num, inv_t)
    G, M = sc.shape
    S = int(pk.shape[1])
    gl = None if grad_logp is None else np.asarray(_host(grad_logp), dtype=np.float64)
    if gl is not None and gl.shape != (G, S):
        raise ValueError(f"grad_logp must have one entry per slate {(G, S)}, got {gl.shape}")
    logp, step, logz = np.zeros((G, S)), np.zeros((G, S, k)), np.zeros((G, S, k))
    length = np.zeros((G, S), dtype=np.int32)
    coef, absolute = np.zeros((G, M)), np.zeros((G, M))
    for g in range(G):
        terms, aterms = [], []
        for s in range(S):
            logp[g, s], step[g, s], logz[g, s], length[g, s] = _pl_slate_host(a[g], live[g], pk[g, s], k)
            if gl is not None and length[g, s] > 0 and gl[g, s] != 0.0:
                dl, ab = _pl_slate_grad_host(a[g], live[g], pk[g, s], int(length[g, s]))
                terms.append(gl[g, s] * dl)
                aterms.append(abs(gl[g, s]) * ab)
        if terms:
            coef[g] = [inv_t * math.fsum(col) for col in np.stack(terms, axis=1).tolist()]
            absolute[g] = [abs(inv_t) * math.fsum(col) for col in np.stack(aterms, axis=1).tolist()]
    out = (logp, step.astype(np.float32)) + (() if gl is None else (np.where(live, coef, 0.0),))
    if parts:
        d = {"step": step, "logZ": logz, "live": live.sum(axis=1), "length": length}
        if gl is not None:
            d["absolute"] = np.where(live, absolute, 0.0)
        out += (d,)
    return out


def list_pl_grad_host(users, rows, scores, ids, count, picks, scale=1.0, temperature=1.0, grad_logp=None):
    """The contract of ``digat_list_pl_bwd`` in numpy float64: with ``coef`` of ``list_pl_host`` on ``scores`` (``grad_logp`` None:
    ones), ``d_users[g] = sum_j coef[g, j] rows[ids[g, j]]`` and ``d_rows[p]`` = the sum of ``coef[g, j] users[g]`` over the live slots
    with ``ids[g, j] == p``.  Returns ``(d_users [G, d], d_rows [P, d])``."""
    U, R = np.asarray(users, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    if U.ndim != 2 or R.ndim != 2 or U.shape[1] != R.shape[1]:
        raise ValueError(f"users [G, d] and rows [P, d] must share d, got {U.shape} and {R.shape}")
    pk = np.asarray(_host(picks))
    gl = np.ones(pk.shape[:2]) if grad_logp is None else grad_logp
    coef = list_pl_host(scores, ids, count, pk, R.shape[0], scale, temperature, grad_logp=gl)[2]
    if U.shape[0] != coef.shape[0]:
        raise ValueError(f"users must have one row per list ({coef.shape[0]}), got {U.shape}")
    I = np.asarray(_host(ids)).astype(np.int64)
    g_of, j_of = np.nonzero(coef != 0)
    d_users, d_rows = np.zeros_like(U), np.zeros_like(R)
    np.add.at(d_users, g_of, coef[g_of, j_of][:, None] * R[I[g_of, j_of]])
    np.add.at(d_rows, I[g_of, j_of], coef[g_of, j_of][:, None] * U[g_of])
    return d_users, d_rows


def list_pl_bound(n, k, samples, coef, absolute):
    """The error bound csrc/digat_list_pl.inc derives for the float32 ``coef`` of ``list_pl`` / ``pl_scores`` against ``list_pl_host``
    on the same scores: ``2^-24 |coef| + (n + k + S + 20) 2^-53 A + 2^-149`` — ``n`` [G] the live positions of the list, ``k`` the
    slate length, ``S`` the slates per list (their terms are added one after the other), ``A`` = ``absolute`` of ``list_pl_host``'s
    parts, the sum the cancelling terms are measured against.  ``logp`` and ``step_logp`` carry ``pl_bound`` unchanged."""
    c = np.abs(np.asarray(coef, dtype=np.float64))
    A = np.abs(np.asarray(absolute, dtype=np.float64))
    n = np.asarray(n, dtype=np.float64).reshape(-1, 1)
    return 2.0 ** -24 * c + (n + float(k) + float(samples) + 20.0) * 2.0 ** -53 * A + 2.0 ** -149


def _check_picks(picks, G: int):
    import torch
    if picks.is_floating_point() or picks.dtype == torch.bool:
        raise ValueError(f"picks must hold integer positions, got {picks.dtype}")
    if picks.dim() != 3 or int(picks.shape[0]) != G or int(picks.shape[1]) < 1 or not 1 <= int(picks.shape[2]) <= PL_MAX_K:
        raise ValueError(f"picks must be [G = {G}, S >= 1, k] with 1 <= k <= PL_MAX_K = {PL_MAX_K}, got {tuple(picks.shape)}")
    return int(picks.shape[1]), int(picks.shape[2])


def _pl_stock(S, live, picks, inv_t):
    """The stock composition on scores ``S`` [G, M] (differentiable), in their dtype: a gather of the picks, ``logsumexp`` of the
    unpicked tail and a flipped ``logcumsumexp`` — ``(logp [G, S], step [G, S, k])`` with ``pl_log_prob``'s cut rule for the slates.
    A position without mass holds a huge negative FINITE number in place of -inf: ``logcumsumexp``'s backward divides by its result."""
    import torch
    G, M = int(S.shape[0]), int(S.shape[1])
    Sn, k = int(picks.shape[1]), int(picks.shape[2])
    low = torch.finfo(S.dtype).min / 8
    a = (torch.where(live, S, torch.zeros_like(S)) * inv_t).masked_fill(~live, low)
    pk = picks.to(torch.int64)
    pc = pk.clamp(0, M - 1)
    flat = pc.view(G, Sn * k)
    earlier = torch.ones(k, k, dtype=torch.bool, device=S.device).tril(-1)
    bad = (pk < 0) | (pk >= M) | ~live.gather(1, flat).view(G, Sn, k) | ((pk[:, :, :, None] == pk[:, :, None, :]) & earlier).any(dim=3)
    keep = bad.to(torch.int64).cumsum(dim=2) == 0
    ap = torch.where(keep, a.gather(1, flat).view(G, Sn, k), a.new_full((), low))
    picked = torch.zeros((G, Sn, M), dtype=torch.int32, device=S.device).scatter_add_(2, pc, keep.to(torch.int32)) > 0
    tail = torch.logsumexp(a[:, None, :].expand(G, Sn, M).masked_fill(picked, low), dim=2)
    logZ = torch.logcumsumexp(torch.cat([tail[:, :, None], ap.flip(2)], dim=2), dim=2)[:, :, 1:].flip(2)
    step = torch.where(keep, ap - logZ, torch.zeros_like(ap))
    return step.sum(dim=2), step


def _list_pl_functions():
    import torch
    from . import _lib

    class ListPL(torch.autograd.Function):
        """``digat_list_pl_fwd`` / ``digat_list_pl_bwd``; the scores are saved, and the sorted entry keys of the rows kernel are built
        here, in the forward: the ids carry no gradient."""

        @staticmethod
        def forward(ctx, users, rows, ids, cnt, picks, inv_t):
            u, v = users.detach().float().contiguous(), rows.detach().float().contiguous()
            G, M, P, d = int(u.shape[0]), int(ids.shape[1]), int(v.shape[0]), int(u.shape[1])
            S, k = int(picks.shape[1]), int(picks.shape[2])
            logp = torch.empty((G, S), dtype=torch.float64, device=u.device)
            step = torch.empty((G, S, k), dtype=torch.float32, device=u.device)
            scores = torch.empty((G, M), dtype=torch.float32, device=u.device)
            _lib.check(_lib.lib().digat_list_pl_fwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(cnt), G, P, M, d, picks.data_ptr(),
                                                    S, k, inv_t, logp.data_ptr(), step.data_ptr(), scores.data_ptr(), _lib.stream_ptr()),
                       "digat_list_pl_fwd")
            keys = None
            if ctx.needs_input_grad[1]:
                elem = list_elements(ids, cnt, P).view(-1)
                flat = torch.arange(G * M, device=u.device)
                keys = torch.sort(ids.view(-1)[elem] * (G * M) + flat[elem]).values.contiguous()
            ctx.save_for_backward(u, v, ids, picks, scores)
            ctx.cnt, ctx.keys, ctx.inv_t, ctx.dtypes = cnt, keys, inv_t, (users.dtype, rows.dtype)
            ctx.mark_non_differentiable(step, scores)
            return logp, step, scores

        @staticmethod
        def backward(ctx, grad_logp, _step, _scores):
            u, v, ids, picks, scores = ctx.saved_tensors
            G, d, P, M = int(u.shape[0]), int(u.shape[1]), int(v.shape[0]), int(ids.shape[1])
            f = dict(dtype=torch.float32, device=u.device)
            want_rows = ctx.needs_input_grad[1] and ctx.keys is not None
            d_users = torch.empty((G, d), **f)
            d_rows = torch.empty((P, d), **f) if want_rows else None
            gl = grad_logp.to(torch.float64).contiguous()
            L = _lib.lib()
            need = int(L.digat_list_pl_workspace_bytes(G, M))
            ws = _lib.workspace(need, u.device, "list_pl")
            keys = ctx.keys if want_rows else None
            _lib.check(L.digat_list_pl_bwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(ctx.cnt), G, P, M, d, scores.data_ptr(),
                                           picks.data_ptr(), int(picks.shape[1]), int(picks.shape[2]), ctx.inv_t, gl.data_ptr(),
                                           _lib.ptr(keys) if keys is not None and keys.numel() else None,
                                           0 if keys is None else int(keys.numel()), d_users.data_ptr(), _lib.ptr(d_rows), ws.data_ptr(),
                                           need, _lib.stream_ptr()), "digat_list_pl_bwd")
            return (d_users.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None), (None if d_rows is None else d_rows.to(ctx.dtypes[1])), \
                None, None, None, None

    class PLScores(torch.autograd.Function):
        """``pl_log_prob``'s call as it is; the backward is the coefficient kernel alone (``digat_pl_scores_bwd``)."""

        @staticmethod
        def forward(ctx, scores, cnt, picks, temperature, inv_t):
            sc = scores.detach().float().contiguous()                 # any floating dtype, as list_pl takes users and rows
            logp, step = pl_log_prob(sc, cnt, picks, temperature)
            ctx.save_for_backward(sc, picks)
            ctx.cnt, ctx.inv_t, ctx.dtype = cnt, inv_t, scores.dtype
            ctx.mark_non_differentiable(step)
            return logp, step

        @staticmethod
        def backward(ctx, grad_logp, _step):
            sc, picks = ctx.saved_tensors
            G, M = int(sc.shape[0]), int(sc.shape[1])
            grad = torch.empty((G, M), dtype=torch.float32, device=sc.device)
            gl = grad_logp.to(torch.float64).contiguous()
            _lib.check(_lib.lib().digat_pl_scores_bwd(sc.data_ptr(), _lib.ptr(ctx.cnt), G, M, int(picks.shape[2]), ctx.inv_t,
                                                      int(picks.shape[1]), picks.data_ptr(), gl.data_ptr(), grad.data_ptr(),
                                                      _lib.stream_ptr()), "digat_pl_scores_bwd")
            return grad.to(ctx.dtype), None, None, None, None

    return ListPL, PLScores


_ListPL = None


def list_pl(users, rows, ids, count, picks, scale=1.0, temperature=1.0):
    """The log-probability of GIVEN slates under the Plackett-Luce model of every user's OWN list, differentiable: ``(logp [G, S]
    float64, step_logp [G, S, k] float32, scores [G, M] float32)``.  ``users`` [G, d], ``rows`` [P, d], ``ids`` [G, M] integer rows
    of ``rows`` and ``count`` [G] (None: M) as in ``list_softmax``: slot (g, j) is an element when ``j < clip(count[g], 0, M)`` and
    ``0 <= ids[g, j] < P``; ``scores`` = the inner products at elements (``dot_scores``' bits), NaN elsewhere.  A position is LIVE
    when it is an element and its score is finite.  ``picks`` [G, S, k] are integer positions into the list, ``1 <= k <= PL_MAX_K``;
    a slate ends at its first entry that is negative, out of range, not live or repeated (``pl_log_prob``'s rule).  With ``a =
    float64(score) * inv_t``, ``inv_t = float64(scale) * (1.0 / float64(temperature))``, ``logp`` and ``step_logp`` are
    ``pl_log_prob_host``'s on ``a``: the probability of the slate under ``softmax(scale * <user, news> / temperature)`` drawn without
    replacement — 0 for an empty slate.  At ``scale = 1`` they are ``pl_log_prob``'s bits on ``scores``.

    ``logp`` is differentiable in ``users`` and ``rows``; ``step_logp`` and ``scores`` are not, and ``picks`` gets no gradient.  The
    gradient is the closed form of ``list_pl_host`` — O(M + k) per slate, no [G, S, M] tensor — and treats ``a_max`` and the clamp at
    -700 as constants: it is the exact gradient while no live entry sits on the clamp (keep ``score * scale / temperature`` spreads
    below 700).  Uses: the likelihood of a logged slate (learning from a log), REINFORCE on sampled slates, and ListMLE with ``picks``
    the ground-truth order.  M <= ``SHORTLIST_MAX_K`` = 1024, d <= ``LIST_SOFTMAX_MAX_D`` = 512, G M < 2^31.

    On CUDA tensors: ``digat_list_pl_fwd`` / ``_bwd`` under autograd — no [G, M, d] gather in memory, no float atomics: two calls give
    the same bits in every output and gradient.  On CPU tensors: the stock composition — ``index_select``, ``bmm``, a gather of the
    picks, ``logsumexp`` of the unpicked tail, a flipped ``logcumsumexp`` — in the dtype of ``users``, differentiable by autograd."""
    import torch
    global _ListPL
    cnt = None if count is None else torch.as_tensor(count)
    if users.dim() != 2 or ids.dim() != 2 or not users.is_floating_point() or not rows.is_floating_point():
        raise ValueError(f"users [G, d] and rows [P, d] must be floating-point matrices and ids [G, M], got {tuple(users.shape)} {users.dtype}, "
                         f"{tuple(rows.shape)} {rows.dtype} and {tuple(ids.shape)}")
    G, P, M, d = _check_list_args(users, rows, ids, cnt, "list_pl")
    S, k = _check_picks(picks, G)
    inv_t = _pl_inv_t(scale, temperature)
    dev = users.device
    if any(t.device != dev for t in (rows, ids, picks) + (() if cnt is None else (cnt,))):
        raise ValueError("users, rows, ids, count and picks must live on one device")
    ids = ids.to(torch.int64).contiguous()
    if dev.type == "cuda":
        if _ListPL is None:
            _ListPL = _list_pl_functions()
        if G == 0 or P == 0:                                          # nothing is live: every slate is empty, no launch, a zero gradient
            z = torch.zeros((G, S), dtype=torch.float64, device=dev) + 0.0 * (users.double().sum() + rows.double().sum())
            return z, users.new_zeros((G, S, k), dtype=torch.float32), users.new_full((G, M), float("nan"), dtype=torch.float32)
        pk = torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()
        return _ListPL[0].apply(users, rows, ids, None if cnt is None else cnt.to(torch.int32).contiguous(), pk, inv_t)
    elem = list_elements(ids, cnt, P)
    safe = torch.where(elem, ids, torch.zeros_like(ids)).view(-1)
    if P == 0:
        Sc = users.new_zeros((G, M)) + 0.0 * (users.sum() + rows.sum())
    else:
        gathered = rows.index_select(0, safe).view(G, M, d)                                              # [G, M, d]
        Sc = torch.bmm(gathered, users.unsqueeze(2)).squeeze(2)
    shown = torch.where(elem, Sc.detach(), Sc.new_full((G, M), float("nan")))
    live = elem & torch.isfinite(Sc.detach())
    if P > 0 and not bool(live[elem].all()):                          # a row without mass must not meet the backward: 0 * inf is a NaN
        Sc = torch.bmm(torch.where(live[:, :, None], gathered, torch.zeros_like(gathered)), users.unsqueeze(2)).squeeze(2)
    logp, step = _pl_stock(Sc, live, picks, inv_t)
    return logp, step.detach(), shown


def pl_scores(scores, count, picks, temperature):
    """``list_pl``'s likelihood on GIVEN scores ``scores`` [G, M] — a model whose score is no inner product, through autograd on its
    own logits: ``(logp [G, S] float64, step_logp [G, S, k] float32)``.  A position is live when ``j < clip(count[g], 0, M)``
    (``count`` None: M) and its score is finite; ``picks`` as in ``list_pl``.  The forward is ``pl_log_prob``'s call unchanged — its
    bits —; ``logp`` is differentiable in ``scores``: the gradient is ``list_pl_host``'s coefficient at ``scale = 1`` (``a_max`` and the
    clamp held constant), exactly 0 at every position that is not live.  On CUDA tensors the kernels read float32: ``scores`` of
    another floating dtype are converted first and the gradient comes back in their dtype; ``digat_pl_log_prob`` and
    ``digat_pl_scores_bwd`` (the coefficient kernel of ``list_pl``: the same bits on the same scores); on CPU tensors the stock
    composition in the dtype of ``scores``."""
    import torch
    global _ListPL
    if scores.dim() != 2 or not scores.is_floating_point():
        raise ValueError(f"scores must be a floating-point tensor [G, M], got {tuple(scores.shape)} {scores.dtype}")
    cnt = None if count is None else torch.as_tensor(count)
    G, M = int(scores.shape[0]), int(scores.shape[1])
    k = int(picks.shape[2]) if picks.dim() == 3 else 0
    inv_t = _check_pl_args((G, M), None if cnt is None else tuple(cnt.shape), k, temperature, picks_shape=tuple(picks.shape))
    _check_picks(picks, G)
    dev = scores.device
    if picks.device != dev or (cnt is not None and cnt.device != dev):
        raise ValueError("scores, count and picks must live on one device")
    if dev.type == "cuda":
        if _ListPL is None:
            _ListPL = _list_pl_functions()
        S = int(picks.shape[1])
        if G == 0:
            return torch.zeros((0, S), dtype=torch.float64, device=dev) + 0.0 * scores.double().sum(), scores.new_zeros((0, S, k), dtype=torch.float32)
        pk = torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()
        return _ListPL[1].apply(scores, None if cnt is None else cnt.to(torch.int32).contiguous(), pk, temperature, inv_t)
    live = torch.isfinite(scores.detach())
    if cnt is not None:
        live = live & (torch.arange(M)[None, :] < cnt.to(torch.int64).clamp(0, M)[:, None])
    logp, step = _pl_stock(torch.where(live, scores, torch.zeros_like(scores)), live, picks, inv_t)
    return logp, step.detach()


# ---- the PL-Rank policy gradient of a position-weighted metric over a user's own list: csrc/digat_list_plrank.inc ------------------
def _plrank_discount(discount, k: int) -> np.ndarray:
    """``discount`` (None: ``ndcg_discount(k)``) as a contiguous float64 numpy [k] table: finite and non-negative."""
    if discount is None:
        return ndcg_discount(int(k))
    D = discount.cpu().numpy() if _is_tensor(discount) else np.asarray(discount)
    if D.dtype != np.float64 or D.shape != (int(k),):
        raise ValueError(f"discount must be a float64 table with one value per slate position ({int(k)}), got {D.dtype} {D.shape}")
    if not np.isfinite(D).all() or (D < 0).any():
        raise ValueError("discount must be finite and non-negative")
    return np.ascontiguousarray(D)


def _plrank_list_weight(list_weight, G: int) -> np.ndarray:
    if list_weight is None:
        return np.ones(G, dtype=np.float64)
    w = np.ascontiguousarray(_host(list_weight), dtype=np.float64)
    if w.shape != (G,) or not np.isfinite(w).all():
        raise ValueError(f"list_weight must hold one finite value per list ({G}), got shape {w.shape}")
    return w


def _plrank_gain_host(gain, shape) -> np.ndarray:
    """``gain`` as float64 [G, M] through float32: a NaN, an infinity or a negative value counts as 0 (``nrms.slate_ndcg``'s rule)."""
    g = np.ascontiguousarray(_host(gain), dtype=np.float32)
    if g.shape != tuple(shape):
        raise ValueError(f"gain must hold one value per slot {tuple(shape)}, got {g.shape}")
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(g) & (g > 0), g, np.float32(0)).astype(np.float64)


def _plrank_slate_host(a, live, picks, n, rho, theta):
    """``(c [M], absolute [M], PR_0)`` of one slate of length ``n`` (``_pl_slate_host``'s cut), float64 with ``math.fsum``."""
    import math
    M = len(a)
    c, ab = np.zeros(M), np.zeros(M)
    if n == 0:
        return c, ab, 0.0
    w = np.where(live, np.exp(np.maximum(a - a[live].max(), PL_CLAMP)), 0.0)
    r = [np.float64(theta[t]) * rho[int(picks[t])] for t in range(n)]
    PR = [np.float64(math.fsum(r[t:])) for t in range(n + 1)]
    left = live.copy()
    qa, qb = [], []
    A = B = np.float64(0.0)
    for t in range(n):
        p = int(picks[t])
        z = np.float64(math.fsum(w[left].tolist()))
        qa.append(np.float64(theta[t]) / z)
        qb.append(PR[t] / z)
        A, B = np.float64(math.fsum(qa)), np.float64(math.fsum(qb))
        c[p] = PR[t + 1] + w[p] * (rho[p] * A - B)
        ab[p] = PR[t + 1] + w[p] * (rho[p] * A + B)
        left[p] = False
    c[left] = w[left] * (rho[left] * A - B)
    ab[left] = w[left] * (rho[left] * A + B)
    return c, ab, float(PR[0])


def plrank_host(scores, ids, count, picks, gain, rows_num, discount=None, list_weight=None, scale=1.0, temperature=1.0, grad_value=None,
                parts: bool = False):
    """The contract of ``digat_list_plrank_fwd`` / ``digat_plrank_scores_fwd`` and of their coefficient kernel on given scores
    ``scores`` [G, M] float32 and GIVEN slates ``picks`` [G, S, k], in numpy float64 with ``math.fsum`` — the yardstick of the kernels.
    Lists, elements, live positions, ``a``, ``inv_t``, ``w`` and ``Z_t`` are ``list_pl_host``'s (``ids`` None: ``plrank_scores``' rule);
    a slate is cut by ``pl_log_prob_host``'s rule, and one cut short is the metric truncated at its length.  ``gain`` [G, M] float32
    (a NaN, an infinity or a negative value counts as 0) is ``rho``, ``discount`` [k] float64 (None: ``ndcg_discount(k)``) is
    ``theta``, ``list_weight`` [G] float64 (None: 1).  For a slate of length n with picks ``p_0 .. p_{n-1}``: ``r_t = theta_t rho_{p_t}``,
    ``PR_t = fsum(r[t:])``, ``A_t = fsum(theta_u / Z_u, u < t)``, ``B_t = fsum(PR_u / Z_u, u < t)`` and the PL-Rank-2 coefficient

        ``c(j) = w_j (rho_j A_n - B_n)`` (live, not in the slate), ``c(p_t) = PR_{t+1} + w_{p_t} (rho_{p_t} A_{t+1} - B_{t+1})``, 0 (not live)

    whose mean over the policy's slates is the exact gradient in ``a`` of the expected metric.  Returns ``(value [G], slate_value
    [G, S])``: ``slate_value = PR_0`` and ``value = list_weight * (fsum_s slate_value / S)`` — the SAMPLE MEAN of the metric; with
    ``grad_value`` [G] also ``coef`` [G, M] = ``((inv_t * list_weight) * grad_value) * (fsum_s c_s(j) / S)``, the ESTIMATOR of the
    gradient of the expected metric, not the derivative of that sample mean; an empty slate adds nothing and counts in S.
    ``parts`` adds a dict: ``live`` [G], ``length`` [G, S], ``terms`` [G, S, M] (``c_s(j)``) and, with ``grad_value``, ``absolute``
    [G, M] = ``|f| fsum_s(PR_{t+1} + w_j (rho_j A + B)) / S``, what ``plrank_bound`` takes."""
    import math
    inv_t = _pl_inv_t(scale, temperature)
    sc, live, a, pk, k = _list_pl_host_parts(scores, ids, count, picks, rows_num, inv_t)
    G, M = sc.shape
    S = int(pk.shape[1])
    rho = _plrank_gain_host(gain, (G, M))
    theta = _plrank_discount(discount, k)
    lw = _plrank_list_weight(list_weight, G)
    gv = None if grad_value is None else np.asarray(_host(grad_value), dtype=np.float64)
    if gv is not None and gv.shape != (G,):
        raise ValueError(f"grad_value must have one entry per list ({G}), got {gv.shape}")
    length = np.zeros((G, S), dtype=np.int32)
    slate_value, value = np.zeros((G, S)), np.zeros(G)
    terms, aterms = np.zeros((G, S, M)), np.zeros((G, S, M))
    coef, absolute = np.zeros((G, M)), np.zeros((G, M))
    for g in range(G):
        for s in range(S):
            length[g, s] = _pl_slate_host(a[g], live[g], pk[g, s], k)[3]
            terms[g, s], aterms[g, s], slate_value[g, s] = _plrank_slate_host(a[g], live[g], pk[g, s], int(length[g, s]), rho[g], theta)
        value[g] = lw[g] * (np.float64(math.fsum(slate_value[g].tolist())) / np.float64(S))
        if gv is not None and gv[g] != 0.0:
            f = (np.float64(inv_t) * lw[g]) * gv[g]
            coef[g] = [f * (np.float64(math.fsum(col)) / np.float64(S)) for col in terms[g].T.tolist()]
            absolute[g] = [abs(f) * (np.float64(math.fsum(col)) / np.float64(S)) for col in aterms[g].T.tolist()]
    out = (value, slate_value) + (() if gv is None else (np.where(live, coef, 0.0),))
    if parts:
        d = {"live": live.sum(axis=1), "length": length, "terms": terms}
        if gv is not None:
            d["absolute"] = np.where(live, absolute, 0.0)
        out += (d,)
    return out


def plrank_grad_host(users, rows, scores, ids, count, picks, gain, discount=None, list_weight=None, scale=1.0, temperature=1.0,
                     grad_value=None):
    """The contract of ``digat_list_plrank_bwd`` in numpy float64: with ``coef`` of ``plrank_host`` on ``scores`` (``grad_value`` None:
    ones), ``list_pl_grad_host``'s two sums: ``(d_users [G, d], d_rows [P, d])``."""
    U, R = np.asarray(users, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    if U.ndim != 2 or R.ndim != 2 or U.shape[1] != R.shape[1]:
        raise ValueError(f"users [G, d] and rows [P, d] must share d, got {U.shape} and {R.shape}")
    gv = np.ones(U.shape[0]) if grad_value is None else grad_value
    coef = plrank_host(scores, ids, count, picks, gain, R.shape[0], discount, list_weight, scale, temperature, grad_value=gv)[2]
    I = np.asarray(_host(ids)).astype(np.int64)
    g_of, j_of = np.nonzero(coef != 0)
    d_users, d_rows = np.zeros_like(U), np.zeros_like(R)
    np.add.at(d_users, g_of, coef[g_of, j_of][:, None] * R[I[g_of, j_of]])
    np.add.at(d_rows, I[g_of, j_of], coef[g_of, j_of][:, None] * U[g_of])
    return d_users, d_rows


def plrank_bound(n, k, samples, coef=None, absolute=None, value=None):
    """The error bounds csrc/digat_list_plrank.inc derives against ``plrank_host`` on the same scores and picks.  With ``coef`` and
    ``absolute`` [G, M] (the twin's coefficient and the ``absolute`` of its parts), ``n`` [G] the live positions of the list, ``k``
    the slate length and ``S`` the slates per list: ``2^-24 |coef| + (n + 2 k + S + 24) 2^-53 A + 2^-149`` — the float32 rounding
    leads; ``rho_j A - B`` cancels, so the float64 terms are relative to the ABSOLUTE sum.  With ``value`` (``value`` [G] or
    ``slate_value`` [G, S]): ``(k + S + 6) 2^-53 |value|``, the order of at most k + S positive additions."""
    if value is not None:
        return (float(k) + float(samples) + 6.0) * 2.0 ** -53 * np.abs(np.asarray(value, dtype=np.float64))
    c = np.abs(np.asarray(coef, dtype=np.float64))
    A = np.abs(np.asarray(absolute, dtype=np.float64))
    n = np.asarray(n, dtype=np.float64).reshape(-1, 1)
    return 2.0 ** -24 * c + (n + 2.0 * float(k) + float(samples) + 24.0) * 2.0 ** -53 * A + 2.0 ** -149


def _pl_draw_host(sc, count, inv_t, k, seed, samples, first_sample, streams):
    """``pl_sample_host``'s picks [G, S, k] int32 under a given ``inv_t`` (at ``inv_t = 1 / temperature`` they are its picks): the
    draw ``list_plrank`` makes inside its kernel."""
    sc, live, a = _pl_lists_host(sc, count, inv_t)
    (G, M), k, S = sc.shape, int(k), int(samples)
    words = pl_draws_host(_check_streams_host(streams, G), S, M, seed, first_sample)
    with np.errstate(divide="ignore"):
        key = a[:, None, :] + -np.log(-np.log((words.astype(np.float64) + 0.5) * 2.0 ** -32))
    picks = np.full((G, S, k), -1, dtype=np.int32)
    for g in range(G):
        pos = np.flatnonzero(live[g])
        n = min(len(pos), k)
        for s in range(S):
            picks[g, s, :n] = pos[np.argsort(-key[g, s, pos], kind="stable")[:n]]
    return picks


def _plrank_functions():
    import torch
    from . import _lib

    class ListPLRank(torch.autograd.Function):
        """``digat_list_plrank_fwd`` / ``_bwd``; the scores and the slates are saved, the sorted entry keys of the rows kernel are built
        in the forward.  ``out_picks`` is filled in place when the slates are drawn (``picks`` None)."""

        @staticmethod
        def forward(ctx, users, rows, ids, cnt, gain, disc, lw, picks, out_picks, S, k, inv_t, seed, first_sample, streams):
            u, v = users.detach().float().contiguous(), rows.detach().float().contiguous()
            G, M, P, d = int(u.shape[0]), int(ids.shape[1]), int(v.shape[0]), int(u.shape[1])
            value = torch.empty((G,), dtype=torch.float64, device=u.device)
            slate_value = torch.empty((G, S), dtype=torch.float64, device=u.device)
            scores = torch.empty((G, M), dtype=torch.float32, device=u.device)
            _lib.check(_lib.lib().digat_list_plrank_fwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(cnt), G, P, M, d, gain.data_ptr(),
                                                        disc.data_ptr(), _lib.ptr(lw), _lib.ptr(picks), S, k, inv_t, seed, first_sample,
                                                        _lib.ptr(streams), _lib.ptr(out_picks), slate_value.data_ptr(), value.data_ptr(),
                                                        scores.data_ptr(), _lib.stream_ptr()), "digat_list_plrank_fwd")
            keys = None
            if ctx.needs_input_grad[1]:
                elem = list_elements(ids, cnt, P).view(-1)
                flat = torch.arange(G * M, device=u.device)
                keys = torch.sort(ids.view(-1)[elem] * (G * M) + flat[elem]).values.contiguous()
            ctx.save_for_backward(u, v, ids, out_picks if picks is None else picks, scores, gain, disc)
            ctx.cnt, ctx.lw, ctx.keys, ctx.inv_t, ctx.dtypes = cnt, lw, keys, inv_t, (users.dtype, rows.dtype)
            ctx.mark_non_differentiable(slate_value, scores)
            return value, slate_value, scores

        @staticmethod
        def backward(ctx, grad_value, _sv, _scores):
            u, v, ids, picks, scores, gain, disc = ctx.saved_tensors
            G, d, P, M = int(u.shape[0]), int(u.shape[1]), int(v.shape[0]), int(ids.shape[1])
            f = dict(dtype=torch.float32, device=u.device)
            want_rows = ctx.needs_input_grad[1] and ctx.keys is not None
            d_users = torch.empty((G, d), **f)
            d_rows = torch.empty((P, d), **f) if want_rows else None
            gv = grad_value.to(torch.float64).contiguous()
            L = _lib.lib()
            need = int(L.digat_list_plrank_workspace_bytes(G, M))
            ws = _lib.workspace(need, u.device, "list_pl")
            keys = ctx.keys if want_rows else None
            _lib.check(L.digat_list_plrank_bwd(u.data_ptr(), v.data_ptr(), ids.data_ptr(), _lib.ptr(ctx.cnt), G, P, M, d, scores.data_ptr(),
                                               gain.data_ptr(), disc.data_ptr(), _lib.ptr(ctx.lw), picks.data_ptr(), int(picks.shape[1]),
                                               int(picks.shape[2]), ctx.inv_t, gv.data_ptr(),
                                               _lib.ptr(keys) if keys is not None and keys.numel() else None,
                                               0 if keys is None else int(keys.numel()), d_users.data_ptr(), _lib.ptr(d_rows), ws.data_ptr(),
                                               need, _lib.stream_ptr()), "digat_list_plrank_bwd")
            return ((d_users.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None), (None if d_rows is None else d_rows.to(ctx.dtypes[1]))) \
                + (None,) * 13

    class PLRankScores(torch.autograd.Function):
        """``digat_plrank_scores_fwd``; the backward is the coefficient kernel alone (``digat_plrank_scores_bwd``)."""

        @staticmethod
        def forward(ctx, scores, cnt, gain, disc, lw, picks, out_picks, S, k, inv_t, seed, first_sample, streams):
            sc = scores.detach().float().contiguous()
            G, M = int(sc.shape[0]), int(sc.shape[1])
            value = torch.empty((G,), dtype=torch.float64, device=sc.device)
            slate_value = torch.empty((G, S), dtype=torch.float64, device=sc.device)
            _lib.check(_lib.lib().digat_plrank_scores_fwd(sc.data_ptr(), _lib.ptr(cnt), G, M, gain.data_ptr(), disc.data_ptr(), _lib.ptr(lw),
                                                          _lib.ptr(picks), S, k, inv_t, seed, first_sample, _lib.ptr(streams), _lib.ptr(out_picks),
                                                          slate_value.data_ptr(), value.data_ptr(), _lib.stream_ptr()), "digat_plrank_scores_fwd")
            ctx.save_for_backward(sc, out_picks if picks is None else picks, gain, disc)
            ctx.cnt, ctx.lw, ctx.inv_t, ctx.dtype = cnt, lw, inv_t, scores.dtype
            ctx.mark_non_differentiable(slate_value)
            return value, slate_value

        @staticmethod
        def backward(ctx, grad_value, _sv):
            sc, picks, gain, disc = ctx.saved_tensors
            G, M = int(sc.shape[0]), int(sc.shape[1])
            grad = torch.empty((G, M), dtype=torch.float32, device=sc.device)
            gv = grad_value.to(torch.float64).contiguous()
            _lib.check(_lib.lib().digat_plrank_scores_bwd(sc.data_ptr(), _lib.ptr(ctx.cnt), G, M, gain.data_ptr(), disc.data_ptr(), _lib.ptr(ctx.lw),
                                                          picks.data_ptr(), int(picks.shape[1]), int(picks.shape[2]), ctx.inv_t, gv.data_ptr(),
                                                          grad.data_ptr(), _lib.stream_ptr()), "digat_plrank_scores_bwd")
            return (grad.to(ctx.dtype),) + (None,) * 12

    return ListPLRank, PLRankScores


_ListPLRank = None


def _plrank_args(G, M, dev, gain, k, samples, discount, list_weight, scale, temperature, first_sample, streams, picks):
    """The checks ``list_plrank`` and ``plrank_scores`` share: ``(k, S, inv_t, theta numpy [k], list_weight numpy [G] or None)``."""
    import torch
    inv_t = _pl_inv_t(scale, temperature)
    if picks is not None:
        S, kk = _check_picks(picks, G)
        if int(k) != kk:
            raise ValueError(f"picks must hold slates of k = {int(k)} positions, got {tuple(picks.shape)}")
    else:
        S = int(samples)
    _check_pl_args((G, M), None, k, 1.0, S, first_sample, None if streams is None else tuple(streams.shape))
    if not torch.is_tensor(gain) or not gain.is_floating_point() or tuple(gain.shape) != (G, M):
        raise ValueError(f"gain must be a floating-point tensor with one value per slot {(G, M)}")
    given = [t for t in (gain, streams, picks) if t is not None]
    if any(t.device != dev for t in given):
        raise ValueError("users, rows, ids, count, gain, streams and picks must live on one device")
    return int(k), S, inv_t, _plrank_discount(discount, k), None if list_weight is None else _plrank_list_weight(list_weight, G)


def _plrank_cpu(Sc, live, cnt, gain, k, S, theta, lw, scale, temperature, inv_t, seed, first_sample, streams, picks):
    """The CPU branch on differentiable scores ``Sc`` [G, M] (0 where not live): the slates by ``_pl_draw_host``, the coefficient from
    ``plrank_host`` on the detached scores, and ``value`` with the surrogate ``sum_j coef_j score_j`` attached so that autograd carries
    the estimator."""
    import torch
    G, M = int(Sc.shape[0]), int(Sc.shape[1])
    sc32 = np.where(live.numpy(), Sc.detach().to(torch.float32).numpy(), np.float32("nan"))
    cn = None if cnt is None else cnt.numpy()
    if picks is None:
        pk = _pl_draw_host(sc32, cn, inv_t, k, seed, S, first_sample, None if streams is None else streams.numpy())
    else:
        pk = np.clip(picks.numpy(), -1, PL_MAX_LIST).astype(np.int32)
    value, slate_value, coef = plrank_host(sc32, None, cn, pk, gain.detach().numpy(), 0, theta, lw, scale, temperature, grad_value=np.ones(G))
    sur = (torch.from_numpy(coef).to(Sc.dtype) * Sc).sum(dim=1).to(torch.float64)
    return torch.from_numpy(value) + (sur - sur.detach()), torch.from_numpy(slate_value), torch.from_numpy(pk)


def list_plrank(users, rows, ids, count, gain, k, samples=1, discount=None, list_weight=None, scale=1.0, temperature=1.0, seed=0,
                first_sample=0, streams=None, picks=None):
    """The PL-Rank policy gradient of a position-weighted metric under the Plackett-Luce policy of every user's OWN list, in one pass:
    ``(value [G] float64, slate_value [G, S] float64, picks [G, S, k] int32, scores [G, M] float32)``.  ``users``, ``rows``, ``ids``
    and ``count`` are ``list_pl``'s, with its elements, live positions and ``inv_t``.  The metric of a slate is ``sum_t discount[t]
    gain[g, picks[t]]``: ``gain`` [G, M] floating point (read as float32; a NaN, an infinity or a negative value counts as 0),
    ``discount`` [k] float64 (None: ``ndcg_discount(k)``, DCG@k), ``list_weight`` [G] (None: 1; ``1 / IDCG@k`` makes it nDCG@k).
    With ``picks`` None, ``samples`` slates of ``k`` are DRAWN per list from ``softmax(scale * <user, news> / temperature)`` without
    replacement inside the kernel that scored the list — ``pl_sample``'s draw exactly (seed, ``streams`` [G], ``first_sample + s``,
    the Gumbel key, the tie rule, ``min(k, live)`` entries, -1 behind them): at ``scale = 1`` they are ``pl_sample``'s picks on the
    returned scores — and returned.  With ``picks`` [G, S, k] given, every slate is cut by ``pl_log_prob``'s rule; one cut short is the
    metric truncated at its length; they come back as int32, a position outside the list held at -1 or ``PL_MAX_LIST`` (the same cut).  ``slate_value`` is the metric of every slate and ``value = list_weight * mean_s slate_value``.

    Only ``value`` is differentiable, and only in ``users`` and ``rows``.  ``value`` is the SAMPLE MEAN of the metric; its backward is
    the PL-Rank-2 ESTIMATOR of the gradient of the EXPECTED metric (``plrank_host``: every position is credited with the reward that
    comes after it, an item's own reward enters through its conditional expectation; no baseline) — not the derivative of that sample
    mean, which is zero.  O(M + k) per slate, no [G, S, M] tensor, ``a_max`` and the clamp at -700 held constant.

    On CUDA tensors: ``digat_list_plrank_fwd`` / ``_bwd`` — one scoring pass, no float atomics: two calls give the same bits.  On CPU
    tensors: ``index_select`` + ``bmm`` scores, the slates of ``pl_sample_host``'s draw, the coefficient from ``plrank_host`` on the
    detached scores and ``value`` with the surrogate ``sum_j coef_j score_j`` attached, so that autograd carries the same gradient."""
    import torch
    global _ListPLRank
    cnt = None if count is None else torch.as_tensor(count)
    if users.dim() != 2 or ids.dim() != 2 or not users.is_floating_point() or not rows.is_floating_point():
        raise ValueError(f"users [G, d] and rows [P, d] must be floating-point matrices and ids [G, M], got {tuple(users.shape)} {users.dtype}, "
                         f"{tuple(rows.shape)} {rows.dtype} and {tuple(ids.shape)}")
    G, P, M, d = _check_list_args(users, rows, ids, cnt, "list_plrank")
    dev = users.device
    if any(t.device != dev for t in (rows, ids) + (() if cnt is None else (cnt,))):
        raise ValueError("users, rows, ids, count, gain, streams and picks must live on one device")
    k, S, inv_t, theta, lw = _plrank_args(G, M, dev, gain, k, samples, discount, list_weight, scale, temperature, first_sample, streams, picks)
    ids = ids.to(torch.int64).contiguous()
    if dev.type == "cuda":
        if _ListPLRank is None:
            _ListPLRank = _plrank_functions()
        pk = None if picks is None else torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()
        if G == 0 or P == 0:                                          # nothing is live: every slate is empty, no launch, a zero gradient
            z = torch.zeros((G,), dtype=torch.float64, device=dev) + 0.0 * (users.double().sum() + rows.double().sum())
            return z, torch.zeros((G, S), dtype=torch.float64, device=dev), \
                (torch.full((G, S, k), -1, dtype=torch.int32, device=dev) if pk is None else pk), \
                users.new_full((G, M), float("nan"), dtype=torch.float32)
        out = torch.empty((G, S, k), dtype=torch.int32, device=dev) if pk is None else None
        value, slate_value, scores = _ListPLRank[0].apply(
            users, rows, ids, None if cnt is None else cnt.to(torch.int32).contiguous(), gain.detach().to(torch.float32).contiguous(),
            _device_discount(theta, dev), None if lw is None else torch.from_numpy(lw).to(dev), pk, out, S, k, inv_t, int(seed) & 0xFFFFFFFF,
            int(first_sample), None if streams is None else streams.to(torch.int64).contiguous())
        return value, slate_value, (out if pk is None else pk), scores
    elem = list_elements(ids, cnt, P)
    safe = torch.where(elem, ids, torch.zeros_like(ids)).view(-1)
    if P == 0:
        Sc = users.new_zeros((G, M)) + 0.0 * (users.sum() + rows.sum())
    else:
        gathered = rows.index_select(0, safe).view(G, M, d)                                              # [G, M, d]
        Sc = torch.bmm(gathered, users.unsqueeze(2)).squeeze(2)
    shown = torch.where(elem, Sc.detach(), Sc.new_full((G, M), float("nan")))
    live = elem & torch.isfinite(Sc.detach()) & torch.isfinite(Sc.detach().to(torch.float32))
    if P > 0 and not bool(live.all()):                                # a row without mass must not meet the backward: 0 * inf is a NaN
        Sc = torch.bmm(torch.where(live[:, :, None], gathered, torch.zeros_like(gathered)), users.unsqueeze(2)).squeeze(2)
    value, slate_value, pk = _plrank_cpu(Sc, live, cnt, gain, k, S, theta, lw, scale, temperature, inv_t, seed, first_sample, streams, picks)
    return value, slate_value, pk, shown


def plrank_scores(scores, count, gain, k, samples=1, discount=None, list_weight=None, temperature=1.0, seed=0, first_sample=0, streams=None,
                  picks=None):
    """``list_plrank`` on GIVEN scores ``scores`` [G, M] — a model whose score is no inner product, through autograd on its own logits,
    and the use without a graph: ``(value [G] float64, slate_value [G, S] float64, picks [G, S, k] int32)``.  A position is live when
    ``j < clip(count[g], 0, M)`` (``count`` None: M) and its score is finite; ``inv_t = 1 / temperature``.  ``value`` is differentiable
    in ``scores``: the gradient is ``plrank_host``'s coefficient — the PL-Rank-2 estimator of the gradient of the EXPECTED metric, not
    the derivative of the sample mean ``value`` holds —, exactly 0 at every position that is not live.  On CUDA tensors
    ``digat_plrank_scores_fwd`` / ``_bwd`` read float32 (the coefficient kernel of ``list_plrank``: the same bits on the same scores and
    slates); on CPU tensors the host twin with the surrogate attached."""
    import torch
    global _ListPLRank
    if scores.dim() != 2 or not scores.is_floating_point():
        raise ValueError(f"scores must be a floating-point tensor [G, M], got {tuple(scores.shape)} {scores.dtype}")
    cnt = None if count is None else torch.as_tensor(count)
    G, M = int(scores.shape[0]), int(scores.shape[1])
    dev = scores.device
    if cnt is not None and (cnt.device != dev or tuple(cnt.shape) != (G,)):
        raise ValueError(f"count must hold one entry per list ({G}) on the scores' device")
    k, S, inv_t, theta, lw = _plrank_args(G, M, dev, gain, k, samples, discount, list_weight, 1.0, temperature, first_sample, streams, picks)
    if dev.type == "cuda":
        if _ListPLRank is None:
            _ListPLRank = _plrank_functions()
        pk = None if picks is None else torch.clamp(picks, min=-1, max=PL_MAX_LIST).to(torch.int32).contiguous()
        if G == 0:
            return torch.zeros((0,), dtype=torch.float64, device=dev) + 0.0 * scores.double().sum(), \
                torch.zeros((0, S), dtype=torch.float64, device=dev), torch.zeros((0, S, k), dtype=torch.int32, device=dev)
        out = torch.empty((G, S, k), dtype=torch.int32, device=dev) if pk is None else None
        value, slate_value = _ListPLRank[1].apply(
            scores, None if cnt is None else cnt.to(torch.int32).contiguous(), gain.detach().to(torch.float32).contiguous(),
            _device_discount(theta, dev), None if lw is None else torch.from_numpy(lw).to(dev), pk, out, S, k, inv_t, int(seed) & 0xFFFFFFFF,
            int(first_sample), None if streams is None else streams.to(torch.int64).contiguous())
        return value, slate_value, (out if pk is None else pk)
    live = torch.isfinite(scores.detach()) & torch.isfinite(scores.detach().to(torch.float32))
    if cnt is not None:
        live = live & (torch.arange(M)[None, :] < cnt.to(torch.int64).clamp(0, M)[:, None])
    return _plrank_cpu(torch.where(live, scores, torch.zeros_like(scores)), live, cnt, gain, k, S, theta, lw, 1.0, temperature, inv_t, seed,
                       first_sample, streams, picks)


def off_policy_value(reward, logp_target, logp_logging, clip=None, units=None, replicates: int = 2000, level: float = 0.95, seed: int = 0):
    """What a target policy would have earned on a log made by another: one row per logged slate, ``reward`` [n], ``logp_target`` /
    ``logp_logging`` [n] the slate's log-probability under either policy (``pl_log_prob`` / ``pl_sample``), weights ``exp(logp_target
    - logp_logging)`` capped at ``clip`` (None: no cap).  Returns ``{"ips", "snips"}`` — ``metric_intervals``' fields: ``ips`` the
    mean of ``weight * reward``, ``snips`` the ratio of sums ``sum(weight * reward) / sum(weight)`` (its ``denominators=``), both
    from the same draws — and ``ess`` (``sum(w)^2 / sum(w^2)``, the effective sample size), ``max_weight`` and ``n``.  ``units`` (a
    CSR ``start`` over contiguous rows) keeps a user's slates together in the resampling.  Host arrays or tensors; the resampling
    is ``metric_intervals``' own."""
    r, lt, ll = (np.asarray(_host(x), dtype=np.float64).reshape(-1) for x in (reward, logp_target, logp_logging))
    if not len(r) == len(lt) == len(ll) or len(r) < 1:
        raise ValueError(f"reward, logp_target and logp_logging must hold one entry per logged slate, got {len(r)}, {len(lt)} and {len(ll)}")
    if not (np.isfinite(lt).all() and np.isfinite(ll).all() and np.isfinite(r).all()):
        raise ValueError("reward, logp_target and logp_logging must be finite (a slate the target cannot draw has no finite logp: cut it or leave it out)")
    if clip is not None and not float(clip) > 0.0:
        raise ValueError(f"clip must be positive, got {clip}")
    with np.errstate(over="ignore"):
        w = np.exp(lt - ll)
    if clip is not None:
        w = np.minimum(w, float(clip))
    if not np.isfinite(w).all():
        raise ValueError("a weight exp(logp_target - logp_logging) overflows: name clip")
    wr = w * r
    out = {"ips": metric_intervals(wr, ("ips",), replicates, level, seed, units=units)["ips"],
           "snips": metric_intervals(wr, ("snips",), replicates, level, seed, denominators=w, units=units)["snips"]}
    out.update({"ess": float(w.sum() ** 2 / np.sum(w * w)) if w.sum() > 0 else 0.0, "max_weight": float(w.max()), "n": int(len(w))})
    return out


def off_policy_steps(reward, step_logp_target, step_logp_logging, length, step_mean=None, step_value=None, position_weight=None,
                     clip=None, units=None, replicates: int = 2000, level: float = 0.95, seed: int = 0, length_logging=None):
    """Per-position and doubly robust off-policy values of a sequential slate policy: one row per logged slate, ``reward`` [n, k] the
    reward earned at every position, ``step_logp_target`` / ``step_logp_logging`` [n, k] the step log-probabilities under either
    policy (``pl_expect`` / ``pl_log_prob`` and ``pl_sample``), ``length`` [n] the slate's cut under the target (``pl_expect``'s).
    ``rho_t = exp(sum_{u <= t} (lt_u - ll_u))`` capped at ``clip`` (None: no cap), ``rho_{-1} = 1``:

    ``pdis = mean_i sum_{t < length} rho_t r_t`` — a position's reward is weighted by the ratio of the slate's prefix up to it alone;
    ``dr = mean_i sum_{t < length} [rho_t (r_t - D_t step_value_t) + rho_{t-1} D_t step_mean_t]`` with a value model ``D_t v_item``
    of the reward at position t: ``step_value`` [n, k] the model's value of the item shown, ``step_mean`` [n, k] its expectation
    under the target over what was left of the list (both ``pl_expect``'s) and ``D = position_weight`` [k] (None: ones).  Each pair
    of terms has mean zero under the logging policy whatever the model, so ``dr`` is unbiased where ``pdis`` is (``clip`` None) and
    has less variance the better the model is.  Without ``step_mean`` / ``step_value`` the model is 0 and ``dr`` equals ``pdis``.

    Returns ``{"pdis", "dr"}`` — ``metric_intervals``' fields, both from the same draws, ``units`` (a CSR ``start`` over contiguous
    rows) keeping a user's slates together —, ``ess`` and ``max_weight`` [k] per position (``sum(rho_t)^2 / sum(rho_t^2)`` and the
    largest ``rho_t`` over the slates that reach position t; 0 where none does) and ``n``.  ``length_logging`` [n]: the slate's cut
    under the logging policy where it may differ; a slate whose two lengths differ cannot be drawn in full by the target (or was
    not drawn in full by the logger) and is a ``ValueError``: cut it or leave it out.  Non-finite input is a ``ValueError``.  Host
    arrays or tensors; the resampling is ``metric_intervals``' own."""
    r, lt, ll = (np.asarray(_host(x), dtype=np.float64) for x in (reward, step_logp_target, step_logp_logging))
    if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1 or lt.shape != r.shape or ll.shape != r.shape:
        raise ValueError(f"reward, step_logp_target and step_logp_logging must all be [n >= 1, k >= 1], got {r.shape}, {lt.shape} and {ll.shape}")
    n, k = r.shape
    if (step_mean is None) != (step_value is None):
        raise ValueError("step_mean and step_value come together (evaluate.pl_expect returns both)")
    sm, sv = ((np.zeros_like(r), np.zeros_like(r)) if step_mean is None else
              (np.asarray(_host(x), dtype=np.float64) for x in (step_mean, step_value)))
    if sm.shape != r.shape or sv.shape != r.shape:
        raise ValueError(f"step_mean and step_value must be [n, k] = {r.shape}, got {sm.shape} and {sv.shape}")
    D = np.ones(k, dtype=np.float64) if position_weight is None else np.asarray(_host(position_weight), dtype=np.float64)
    if D.shape != (k,):
        raise ValueError(f"position_weight must be [k] = [{k}], got {D.shape}")
    ln = np.asarray(_host(length))
    if ln.shape != (n,) or ln.dtype.kind not in "iu" or (n and (int(ln.min()) < 0 or int(ln.max()) > k)):
        raise ValueError(f"length must hold one integer in [0, k = {k}] per logged slate ({n}), got {ln.dtype} {ln.shape}")
    if length_logging is not None:
        lg = np.asarray(_host(length_logging))
        if lg.shape != (n,) or lg.dtype.kind not in "iu":
            raise ValueError(f"length_logging must hold one integer per logged slate ({n}), got {lg.dtype} {lg.shape}")
        bad = np.flatnonzero(lg.astype(np.int64) != ln.astype(np.int64))
        if len(bad):
            raise ValueError(f"slate {int(bad[0])} has length {int(lg[bad[0]])} under the logging policy and {int(ln[bad[0]])} under the target "
                             f"({len(bad)} such slates): the target cannot draw it in full — cut it or leave it out")
    for name, x in (("reward", r), ("step_logp_target", lt), ("step_logp_logging", ll), ("step_mean", sm), ("step_value", sv),
                    ("position_weight", D)):
        if not np.isfinite(x).all():
            raise ValueError(f"{name} must be finite (a step the target cannot draw has no finite log-probability: cut the slate or leave it out)")
    if clip is not None and not float(clip) > 0.0:
        raise ValueError(f"clip must be positive, got {clip}")
    shown = np.arange(k)[None, :] < ln.astype(np.int64)[:, None]
    with np.errstate(over="ignore"):
        rho = np.exp(np.cumsum(np.where(shown, lt - ll, 0.0), axis=1))
    if clip is not None:
        rho = np.minimum(rho, float(clip))
    rho = np.where(shown, rho, 0.0)
    if not np.isfinite(rho).all():
        raise ValueError("a weight exp(sum of step_logp_target - step_logp_logging) overflows: name clip")
    before = np.concatenate([np.ones((n, 1), dtype=np.float64), rho[:, :-1]], axis=1)
    pdis = np.where(shown, rho * r, 0.0).sum(axis=1)
    dr = np.where(shown, rho * (r - D[None, :] * sv) + before * (D[None, :] * sm), 0.0).sum(axis=1)
    out = metric_intervals(np.stack([pdis, dr], axis=1), ("pdis", "dr"), replicates, level, seed, units=units)
    s1, s2 = rho.sum(axis=0), (rho * rho).sum(axis=0)
    out.update({"ess": np.where(s2 > 0, s1 * s1 / np.where(s2 > 0, s2, 1.0), 0.0), "max_weight": rho.max(axis=0), "n": int(n)})
    return out


class AvgMetric:
    """util.py:100-121: the model-selection average."""

    def __init__(self, auc, mrr, ndcg5, ndcg10):
        self.auc, self.mrr, self.ndcg5, self.ndcg10 = auc, mrr, ndcg5, ndcg10
        self.avg = (auc + mrr + (ndcg5 + ndcg10) / 2) / 3

    def __gt__(self, o): return self.avg > o.avg
    def __ge__(self, o): return self.avg >= o.avg
    def __lt__(self, o): return self.avg < o.avg
    def __le__(self, o): return self.avg <= o.avg

    def __str__(self):
        return '%.4f\nAUC = %.4f\nMRR = %.4f\nnDCG@5  = %.4f\nnDCG@10 = %.4f' % (
            self.avg, self.auc, self.mrr, self.ndcg5, self.ndcg10)
