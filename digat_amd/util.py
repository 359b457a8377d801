"""Dev/test scoring driver: the counterpart of the reference's ``util.compute_scores`` (util.py:10-85).

Same flow — news-representation cache -> SA gather -> c_n0 precompute -> batched
``Model.inference`` -> per-impression stable ranking -> AUC/MRR/nDCG — re-laid for one MI355X:

* every corpus table lives in HBM for the whole run (288 GB: MIND-small's user graphs are 328 MB,
  the SA cache 1 GB); a batch is assembled by on-device ``index_select`` from (impression, candidate)
  ids instead of 32 DataLoader worker processes building ``[1024,67,67]`` bool arrays item by item
  (util.py:51-52, MIND_dataset.py:97-102);
* rows shard across ranks in contiguous impression-aligned blocks (rows are independent, the ranking
  is per impression), one ``all_gather`` of fp32 scores at the end — no collective on the data path.

The graph encoder is the HIP plugin (``digat_amd.graphEncoders.DIGAT``); nothing here falls back to CPU.
"""
from __future__ import annotations

import dataclasses
import functools
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from . import evaluate


NEWS_TABLE_MAX_BYTES = 48 << 30     # layer-0 [h|P|Q] tables of news graphs of more than 16 nodes are kept up to this size (288 GB of HBM per GPU)
NEWS_TABLE_FREE_FRACTION = 0.5      # ... and never beyond this share of the memory that is free when the table is built
SPARSE_ENTRIES_PER_NODE = 20        # the library's own threshold for DIGAT_XATTN_AUTO (digat_kernels.hip); measured at 15.7 entries per node
                                    # (heavy histories, bench.py): sparse 5.34 vs dense 6.11 ms per 4096-row step; break-even extrapolates to ~21


@dataclass
class DeviceCorpus:
    """Device-resident corpus tables with the reference's array names (MIND_corpus.py:189-298)."""
    news_embedding: torch.Tensor         # [news_num, d]   cached_news_representations (util.py:24-33)
    news_node_ID: torch.Tensor           # [news_num, N]   int64
    news_graph: torch.Tensor             # [news_num, N, N] bool
    news_graph_mask: torch.Tensor        # [news_num, N]   bool
    history: torch.Tensor                # [I, H] int64
    user_graph: Optional[torch.Tensor]          # [I, U, U] bool, or None: built per batch from user_category_indices ("derived")
    user_category_mask: Optional[torch.Tensor]  # [I, C+1] bool, or None likewise
    user_category_indices: torch.Tensor  # [I, H] int64
    row_impression: torch.Tensor         # [R] int64
    row_candidate: torch.Tensor          # [R] int64
    SA_news_representations: Optional[torch.Tensor] = None   # [news_num, N, d] (util.py:36)
    c_n0: Optional[torch.Tensor] = None                      # [news_num, d]    (util.py:37-44)
    news_hpq0: Optional[torch.Tensor] = None                 # [3, news_num, N, d]: layer 0's [h|P|Q] of every news graph
    user_hpq0: Optional[torch.Tensor] = None                 # [3, news_num, d]: layer 0's user-graph [h|P|Q] of every news as a history node
    topic_hpq0: Optional[torch.Tensor] = None                # [3, C, d]: ... of the topic nodes
    ctxq0: Optional[torch.Tensor] = None                     # [3, news_num, d]: topic query | user query | layer-0 user K3 of every c_n0
    news_ctx_layers: Optional[torch.Tensor] = None           # [K, news_num, d]: an ablation encoder's per-news contexts c_n^(0..L)
                                                             # (graphEncoders._Ablation.news_side_tables)
    weights_key: Optional[tuple] = None                      # the weight version the six caches above were computed from
    title_text: Optional[torch.Tensor] = None                # [news_num, Lw] int32 token ids (MIND_corpus.py: news_title_text)
    title_mask: Optional[torch.Tensor] = None                # [news_num, Lw] bool                       (news_title_mask)
    news_key: Optional[tuple] = None                         # the news-encoder weight version news_embedding was computed from
    xattn_hint: Optional[dict] = None                        # THIS corpus's sparse / dense choice per graph (prepare_news_side); applied to the
                                                             # encoder whenever this corpus is scored (two corpora may share one encoder)
    range_overflow_at_prepare: bool = False                  # an fp16x3 GEMM left the format's range while the per-news tables were built
    category_num: int = 0                                    # C (without the padding bucket); 0: read off user_category_mask
    news_source: Optional["DeviceCorpus"] = None             # the corpus this one shares its news side with (from_numpy's news_from)
    news_category: Optional[torch.Tensor] = None             # [news_num] int32 category of every news, where the corpus carries one
                                                             # (mind.MindSplit does): recommend's max_per_category reads it

    def __post_init__(self):
        if not self.category_num and self.user_category_mask is not None:
            self.category_num = int(self.user_category_mask.shape[1]) - 1

    @classmethod
    def from_numpy(cls, corpus, device, user_graphs: str = "table", category_num: Optional[int] = None,
                   news_from: Optional["DeviceCorpus"] = None) -> "DeviceCorpus":
        """``user_graphs="table"``: the corpus's ``user_graph`` / ``user_category_mask`` are uploaded and batches gather rows from
        them; a corpus that holds no ``user_graph`` (``mind.MindSplit``: the ``[I, U, U]`` table is never built on the host) gets
        both built on the device from its category indices, in chunks (``user_graph_tables``).  ``"derived"``: neither is uploaded
        (nor read: the corpus need not have them) — both are a pure function of ``user_category_indices`` and are built on the
        device per batch (``user_graphs_from_indices``); ``category_num`` then comes from the argument, the corpus's mask shape or
        its spec.  A corpus with ``news_title_text`` / ``news_title_mask`` has them uploaded as ``title_text`` / ``title_mask``; one
        without ``news_embedding`` (a text encoder produces it) starts with an empty ``[news_num, 0]`` table, which
        ``compute_scores`` / ``recommend`` fill before anything reads it.

        ``news_from``: another corpus of the same news (a second split).  Nothing of the news side is uploaded: its tensors
        (``news_node_ID``, ``news_graph``, ``news_graph_mask``, ``title_text``, ``title_mask``, ``news_embedding``) and the per-news
        caches of ``prepare_news_side`` are the other corpus's own, and later — the weights have moved on and the other corpus has
        been scored since — this one takes the other's newer ones over while ``weights_key`` matches (``adopt_news_side``);
        otherwise it rebuilds its own, as any corpus does."""
        if user_graphs not in ("table", "derived"):
            raise ValueError("user_graphs must be 'table' or 'derived'")

        def t(a, dtype=None):
            x = torch.from_numpy(np.ascontiguousarray(a))
            return (x.to(dtype) if dtype is not None else x).to(device)
        table = user_graphs == "table"
        if category_num is None:
            mask = getattr(corpus, "user_category_mask", None)
            category_num = int(mask.shape[1]) - 1 if mask is not None else int(corpus.spec.category_num)
        cat_idx = t(corpus.user_category_indices, torch.int64)
        host_graph = getattr(corpus, "user_graph", None) if table else None
        if table and host_graph is None:
            user_graph, cat_mask = user_graph_tables(cat_idx, int(category_num))
        else:
            user_graph, cat_mask = (t(host_graph), t(corpus.user_category_mask)) if table else (None, None)
        if news_from is not None:
            if int(news_from.news_node_ID.shape[0]) != int(np.asarray(corpus.news_node_ID).shape[0]):
                raise ValueError("news_from holds another number of news than the corpus")
            news = (news_from.news_embedding, news_from.news_node_ID, news_from.news_graph, news_from.news_graph_mask)
        else:
            emb = getattr(corpus, "news_embedding", None)
            news_num = int(np.asarray(corpus.news_node_ID).shape[0])
            news = (t(emb) if emb is not None else torch.empty((news_num, 0), dtype=torch.float32, device=device),
                    t(corpus.news_node_ID, torch.int64), t(corpus.news_graph), t(corpus.news_graph_mask))
        dc = cls(*news, t(corpus.history, torch.int64), user_graph, cat_mask, cat_idx,
                 t(corpus.row_impression, torch.int64), t(corpus.row_candidate, torch.int64), category_num=int(category_num))
        if news_from is not None:
            dc.news_source = news_from
            dc.title_text, dc.title_mask, dc.news_key = news_from.title_text, news_from.title_mask, news_from.news_key
            adopt_news_side(None, dc, force=True)
        elif getattr(corpus, "news_title_text", None) is not None:
            dc.title_text, dc.title_mask = t(corpus.news_title_text, torch.int32), t(corpus.news_title_mask, torch.bool)
        if news_from is not None:
            dc.news_category = news_from.news_category
        elif getattr(corpus, "news_category", None) is not None:
            dc.news_category = t(corpus.news_category, torch.int32)
        return dc

    @property
    def rows(self) -> int:
        return int(self.row_impression.shape[0])

    @property
    def user_graph_size(self) -> int:
        """U = H + C: nodes of a user graph."""
        return int(self.user_category_indices.shape[1]) + self.category_num


USER_GRAPH_CHUNK_BYTES = 256 << 20      # a corpus-wide build (entries per node) keeps its transient graph buffer below this
USER_GRAPH_CHUNK_ROWS = 4096            # ... and at this many graphs (20 MB at U = 67: enough to fill the chip, never a corpus-sized table)


def user_graphs_from_indices(cat_idx: torch.Tensor, category_num: int, rows: Optional[torch.Tensor] = None, out=None,
                             want_entries: bool = False):
    """User graphs and category masks from category indices, on the device (``digat_user_graph_build``: MIND_corpus.py:145-176 as
    one launch on the current stream).  ``cat_idx`` [I, H] int64; graph g is built from row ``rows[g]`` (``rows`` [G] int64, any
    order, repeats allowed) or from row g.  Returns ``(user_graph [G,U,U] bool, user_category_mask [G,C+1] bool)`` and, with
    ``want_entries``, ``entries`` [G] int32 (set bytes per graph).  ``out``: preallocated contiguous buffers in that order (bool or
    uint8; the third is optional).  GPU tensors only."""
    from . import _lib
    dev = _lib.require_device(*((cat_idx,) if rows is None else (cat_idx, rows)))
    if cat_idx.dim() != 2:
        raise _lib.DigatHipError("user_category_indices must be [rows, max_history_num]")
    ci = cat_idx.to(torch.int64).contiguous()
    H, C = int(ci.shape[1]), int(category_num)
    U = H + C
    if rows is not None:
        rows = rows.to(torch.int64).contiguous()
    G = int(ci.shape[0] if rows is None else rows.shape[0])
    if out is None:
        graph = torch.empty((G, U, U), dtype=torch.bool, device=dev)
        mask = torch.empty((G, C + 1), dtype=torch.bool, device=dev)
        entries = None
    else:
        graph, mask = out[0], out[1]
        entries = out[2] if len(out) > 2 else None
        _lib.require_device(cat_idx, graph, mask)
        for t, shape in ((graph, (G, U, U)), (mask, (G, C + 1))):
            if tuple(t.shape) != shape or t.dtype not in (torch.bool, torch.uint8) or not t.is_contiguous():
                raise _lib.DigatHipError(f"out buffer must be contiguous bool / uint8 {shape}, got {t.dtype} {tuple(t.shape)}")
    if want_entries and entries is None:
        entries = torch.empty((G,), dtype=torch.int32, device=dev)
    if entries is not None and (tuple(entries.shape) != (G,) or entries.dtype != torch.int32 or not entries.is_contiguous()
                                or entries.device != dev):
        raise _lib.DigatHipError("entries must be a contiguous int32 [G] tensor on the same device")
    if G:                                # empty tensors have no storage to point at
        _lib.check(_lib.lib().digat_user_graph_build(ci.data_ptr(), _lib.ptr(rows), G, H, C, graph.data_ptr(), mask.data_ptr(),
                                                     _lib.ptr(entries), _lib.stream_ptr()), "digat_user_graph_build")
    graph, mask = graph.view(torch.bool), mask.view(torch.bool)
    return (graph, mask, entries) if want_entries else (graph, mask)


def user_side_rows(dc: DeviceCorpus, imp: torch.Tensor):
    """``(user_graph, user_category_mask)`` of the impressions ``imp``: rows of the corpus tables, or — a corpus without them —
    built in place from the impressions' category indices."""
    if dc.user_graph is not None:
        return dc.user_graph.index_select(0, imp), dc.user_category_mask.index_select(0, imp)
    return user_graphs_from_indices(dc.user_category_indices, dc.category_num, rows=imp)


def user_graph_entries_per_node(dc: DeviceCorpus) -> Optional[float]:
    """Mean number of adjacency entries per node over the corpus's user graphs (the sparse / dense choice of Eq. 8), or None for a
    corpus without impressions.  Without a table: from ``entries`` of one build over the corpus, in chunks of at most
    ``USER_GRAPH_CHUNK_ROWS`` graphs whose transient buffer stays below ``USER_GRAPH_CHUNK_BYTES``."""
    I, U = int(dc.user_category_indices.shape[0]), dc.user_graph_size
    if I == 0:
        return None
    if dc.user_graph is not None:
        return float(dc.user_graph.sum(dtype=torch.float64) / (I * U))
    dev = dc.user_category_indices.device
    chunk = max(1, min(I, USER_GRAPH_CHUNK_ROWS, (USER_GRAPH_CHUNK_BYTES - 1) // (U * U)))
    graph = torch.empty((chunk, U, U), dtype=torch.bool, device=dev)
    mask = torch.empty((chunk, dc.category_num + 1), dtype=torch.bool, device=dev)
    entries = torch.empty((I,), dtype=torch.int32, device=dev)
    for s in range(0, I, chunk):
        n = min(chunk, I - s)
        user_graphs_from_indices(dc.user_category_indices[s:s + n], dc.category_num, out=(graph[:n], mask[:n], entries[s:s + n]))
    return float(entries.sum(dtype=torch.float64) / (I * U))


def user_graph_tables(cat_idx: torch.Tensor, category_num: int):
    """The whole corpus's ``(user_graph [I,U,U], user_category_mask [I,C+1])`` from its category indices on the device, written
    chunk by chunk into the two tables (chunks as ``user_graph_entries_per_node`` cuts them)."""
    I, U = int(cat_idx.shape[0]), int(cat_idx.shape[1]) + int(category_num)
    graph = torch.empty((I, U, U), dtype=torch.bool, device=cat_idx.device)
    mask = torch.empty((I, category_num + 1), dtype=torch.bool, device=cat_idx.device)
    chunk = max(1, min(I, USER_GRAPH_CHUNK_ROWS, (USER_GRAPH_CHUNK_BYTES - 1) // (U * U)))
    for s in range(0, I, chunk):
        n = min(chunk, I - s)
        user_graphs_from_indices(cat_idx[s:s + n], category_num, out=(graph[s:s + n], mask[s:s + n]))
    return graph, mask


NEWS_SIDE_CACHES = ("SA_news_representations", "c_n0", "news_hpq0", "user_hpq0", "topic_hpq0", "ctxq0", "news_ctx_layers", "weights_key",
                    "range_overflow_at_prepare")


def adopt_news_side(model, dc: DeviceCorpus, force: bool = False) -> bool:
    """A corpus built with ``news_from`` takes over its source's news representations and per-news caches when the source holds
    newer ones for the current weights, so that one process keeps ONE set of news tables however many splits it scores.  The
    sparse / dense hint of the user graph stays this corpus's own (its users differ); the news part is the source's (same news
    graphs).  ``force``: at construction, whatever the source holds.  Returns whether the caches were taken."""
    src = dc.news_source
    if src is None:
        return False
    enc = getattr(model, "graph_encoder", None)
    ne = getattr(model, "news_encoder", None)
    if not force:
        if src.news_key is None or ne is None or src.news_key != tuple((p.data_ptr(), p._version) for p in ne.parameters()):
            return False                                  # the source's news representations are stale too: score_* re-encodes here
    if dc.news_embedding is not src.news_embedding:
        dc.news_embedding, dc.news_key = src.news_embedding, src.news_key
    if src.c_n0 is None or src.weights_key is None or (dc.c_n0 is src.c_n0 and dc.weights_key == src.weights_key):
        return False
    if src.xattn_hint is not None:
        hint = dict(src.xattn_hint)
        hint.pop("user", None)
        user = (dc.xattn_hint or {}).get("user")          # this corpus's users do not change: decided once
        if user is None:
            per_node = user_graph_entries_per_node(dc)
            user = None if per_node is None else "sparse" if per_node <= SPARSE_ENTRIES_PER_NODE else "dense"
        if user is not None:
            hint["user"] = user
        dc.xattn_hint = hint
    if not force:
        apply_corpus_hint(enc, dc)
        if src.weights_key != weights_key(enc, dc):
            return False
    for f in NEWS_SIDE_CACHES:
        setattr(dc, f, getattr(src, f))
    return True


def shard_rows(row_impression: np.ndarray, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous, impression-aligned block [start, end) of rows for ``rank``.

    Boundaries are the impression starts nearest to the even split, so every impression is scored by
    exactly one rank and the blocks concatenate back in row order."""
    imp = np.asarray(row_impression)
    R = len(imp)
    if world_size <= 1:
        return 0, R
    starts = np.r_[0, np.flatnonzero(np.diff(imp)) + 1, R]

    def cut(k):
        if k <= 0:
            return 0
        if k >= world_size:
            return R
        target = (R * k) // world_size
        return int(starts[np.searchsorted(starts, target, side="left")])
    return cut(rank), cut(rank + 1)


def cache_news_representations(news_encoder, title_text: torch.Tensor, title_mask: torch.Tensor, batch_size: int) -> torch.Tensor:
    """util.py:24-33: the representation of every news, computed once per dev/test run in batches.
    ``title_text`` / ``title_mask`` [news_num, max_title_length] on the GPU.  With ``newsEncoders.MSA`` in eval mode this
    runs on the HIP kernels (``digat_msa_fwd``: embedding lookup folded into the bf16x6 projection GEMM, attention on the
    matrix cores)."""
    news_num = title_text.shape[0]
    out = torch.empty((news_num, news_encoder.news_embedding_dim), dtype=torch.float32, device=title_text.device)
    if hasattr(news_encoder, "eval"):
        news_encoder.eval()
    with torch.no_grad():
        for s in range(0, news_num, batch_size):
            e = min(s + batch_size, news_num)
            out[s:e] = news_encoder(title_text[s:e].unsqueeze(1), title_mask[s:e].unsqueeze(1)).squeeze(1)   # :30-32
    return out


def prepare_news_side(encoder, dc: DeviceCorpus, batch_size: int) -> None:
    """util.py:34-44: gather the SA neighbourhood embeddings and precompute c_n0 for every news."""
    news_num, N = dc.news_node_ID.shape
    d = dc.news_embedding.shape[1]
    # Eq. 8 of the user graph: the corpus is known here, so the sparse / dense choice the library would otherwise make on
    # the device per batch (both variants launched, one returning at once) is made once, on the host, from the mean
    # number of adjacency entries per node (MIND user graphs: ~4 of 67).  An explicit "dense" / "sparse" setting wins.
    if hasattr(encoder, "resolved_xattn_mode"):
        hint = {}
        per_node = user_graph_entries_per_node(dc)
        if per_node is not None:
            hint["user"] = "sparse" if per_node <= SPARSE_ENTRIES_PER_NODE else "dense"
        if N > 16 and dc.news_graph.numel() > 0:
            per_node = float(dc.news_graph.sum(dtype=torch.float64) / (news_num * N))
            hint["news"] = "sparse" if per_node <= SPARSE_ENTRIES_PER_NODE else "dense"
        encoder.corpus_xattn_hint = hint          # in force while the encoder's own setting is "auto"
        dc.xattn_hint = dict(hint)                # ... and re-applied whenever THIS corpus is scored (apply_corpus_hint)
    if hasattr(encoder, "corpus_activation_max") and dc.news_embedding.numel() > 0:
        # the range of the node features the projections will see ("auto" projection format: graphEncoders.resolved_projection_mode)
        encoder.corpus_activation_max = float(dc.news_embedding.abs().max())
    dc.SA_news_representations = dc.news_embedding.index_select(0, dc.news_node_ID.flatten()).view(news_num, N, d)
    dc.news_ctx_layers = None
    if hasattr(encoder, "news_side_tables"):
        # an ablation encoder names what of its news side depends on the news alone: c_n0 (a zero table where no news context
        # exists) and, where the news graph never sees the user, the whole chain c_n^(0..L) — 417 MB at MIND-small, depth 3; built
        # here once per dev run, in chunks, never on the pass
        with torch.no_grad():
            dc.c_n0, dc.news_ctx_layers = encoder.news_side_tables(dc.SA_news_representations, dc.news_graph, dc.news_graph_mask, batch_size)
    else:
        c_n0 = torch.empty((news_num, d), dtype=torch.float32, device=dc.news_embedding.device)
        with torch.no_grad():
            for s in range(0, news_num, batch_size):
                e = min(s + batch_size, news_num)
                c_n0[s:e] = encoder.compute_news_graph_context(dc.SA_news_representations[s:e], dc.news_graph_mask[s:e])
        dc.c_n0 = c_n0
    # ... and, in the same spirit, layer 0's projections of the news graph, which depend on the news alone (small news graphs:
    # the kernel that consumes them adds K3 itself).  [3, news_num, N, d] fp32: 3.1 GB for MIND-small at N = 10.
    # Larger news graphs (N = 26, 65) keep the table too when their Eq. 8 runs on the sparse kernel, which reads the candidates' rows
    # in place (round 4: the layer-0 projection GEMM of B N rows was the largest launch of a MIND-large step); 20 GB at MIND-large
    # scale and at MIND-small stress scale, of 288 — bounded by NEWS_TABLE_MAX_BYTES.
    dc.news_hpq0 = None
    table_bytes = 3 * news_num * N * d * 4
    dev = dc.news_embedding.device
    budget = NEWS_TABLE_MAX_BYTES
    if dev.type == "cuda":          # a smaller-HBM part, or a process that also holds training state: stay within what is free
        budget = min(budget, int(NEWS_TABLE_FREE_FRACTION * torch.cuda.mem_get_info(dev)[0]))
    # the table holds fp32 P, Q: under the reduced-precision storage modes ("pq-bf16", "pq-fp8": P', Q of news graphs of more than
    # 16 nodes leave the GEMM epilogue in bf16 / e4m3 at EVERY layer) the in-batch projection stays, so that the configuration
    # measured is the one documented
    pq_low = getattr(encoder, "projection_mode", "") in ("pq-bf16", "pq-bf16-x1", "pq-fp8")
    big_ok = (N > 16 and table_bytes <= budget and hasattr(encoder, "resolved_xattn_mode") and not pq_low
              and encoder.resolved_xattn_mode("news") == "sparse" and news_num < 2 ** 31)
    if (N <= 16 or big_ok) and d % 4 == 0 and d <= 1024 and hasattr(encoder, "project_news_layer0") and getattr(encoder, "graph_depth", 0) > 0:
        try:
            table = torch.empty((3, news_num, N, d), dtype=torch.float32, device=dev)
            chunk = max(batch_size, 4096)
            with torch.no_grad():
                for s in range(0, news_num, chunk):
                    e = min(s + chunk, news_num)
                    table[:, s:e] = encoder.project_news_layer0(dc.SA_news_representations[s:e])
            dc.news_hpq0 = table
        except torch.OutOfMemoryError:          # the in-batch projection needs no table: slower, same bits
            table = None
            dc.news_hpq0 = None
            torch.cuda.empty_cache()
    # the user graph's layer-0 projections are row-wise: per news (a history node is a news) and per topic node
    dc.user_hpq0 = dc.topic_hpq0 = None
    if hasattr(encoder, "project_user_layer0") and getattr(encoder, "graph_depth", 0) > 0 and d % 4 == 0:
        with torch.no_grad():
            dc.user_hpq0 = encoder.project_user_layer0(dc.news_embedding)
            dc.topic_hpq0 = encoder.project_user_layer0(encoder.topic_node_embedding.detach())
    # ... and the first link of the [B,d] chain: the two queries and the user graph's layer-0 K3 are linear maps of c_n0
    dc.ctxq0 = None
    if hasattr(encoder, "news_context_queries") and not getattr(encoder, "training", False) and d % 4 == 0:
        with torch.no_grad():
            dc.ctxq0 = encoder.news_context_queries(dc.c_n0)
    dc.weights_key = weights_key(encoder, dc)
    # the layer-0 projections of news graphs of more than 16 nodes now run HERE, not during scoring: an activation that leaves the
    # fp16x3 range while the tables are built must still reach the scoring run's range check (score_rows clears the flag first)
    dc.range_overflow_at_prepare = bool(hasattr(encoder, "range_overflowed") and encoder.gemm_format() == 1
                                        and encoder.range_overflowed(reset=False))


def apply_corpus_hint(encoder, dc: DeviceCorpus) -> None:
    """Put THIS corpus's sparse / dense choice (made by ``prepare_news_side``) back in force on the encoder: with two corpora on one
    encoder (dev and test) the encoder otherwise keeps the hint of whichever was prepared last, and a kept layer-0 table of news
    graphs of more than 16 nodes would meet an encoder that no longer names the sparse kernel (DIGAT_ERR_ARG) — or the other way."""
    if dc.xattn_hint is not None and hasattr(encoder, "corpus_xattn_hint"):
        encoder.corpus_xattn_hint = dict(dc.xattn_hint)


def weights_key(encoder, dc: DeviceCorpus) -> tuple:
    """What the per-news caches of ``prepare_news_side`` depend on: every encoder parameter's storage and version counter
    (an optimizer step or ``load_state_dict`` bumps them) and the news representations they were computed from."""
    params = tuple((p.data_ptr(), p._version) for p in encoder.parameters()) if hasattr(encoder, "parameters") else ()
    pm = encoder.resolved_projection_mode() if hasattr(encoder, "resolved_projection_mode") else getattr(encoder, "projection_mode", None)
    fmt = encoder.gemm_format() if hasattr(encoder, "gemm_format") else None
    # ... and the kernel that computes the context-query table (the encoder's pass_rows names it: same bits as inside a pass)
    # ... and whether the news graph's Eq. 8 reads the layer-0 table in place (larger news graphs: only the sparse kernel can)
    # — the RESOLVED mode: the explicit setting, or the corpus hint in force (apply_corpus_hint puts the scored corpus's own there)
    news_mode = encoder.resolved_xattn_mode("news") if hasattr(encoder, "resolved_xattn_mode") else None
    return params + (dc.news_embedding.data_ptr(), dc.news_embedding._version, pm, fmt, getattr(encoder, "pass_rows", 0) >= 2048, news_mode)


def gather_batch(dc: DeviceCorpus, start: int, end: int):
    """The 8 inputs of ``Model.inference`` for rows [start, end) (util.py:57-67), all on device."""
    imp = dc.row_impression[start:end]
    cand = dc.row_candidate[start:end]
    H = dc.history.shape[1]
    d = dc.news_embedding.shape[1]
    hist = dc.history.index_select(0, imp)
    user_rep = dc.news_embedding.index_select(0, hist.flatten()).view(end - start, H, d)
    return (user_rep, *user_side_rows(dc, imp),
            dc.user_category_indices.index_select(0, imp), dc.SA_news_representations.index_select(0, cand),
            dc.news_graph.index_select(0, cand), dc.news_graph_mask.index_select(0, cand),
            dc.c_n0.index_select(0, cand))


def gather_batch_grouped(dc: DeviceCorpus, start: int, end: int, row_impression_host: np.ndarray):
    """Like ``gather_batch`` but the user side is gathered once per impression: returns the 9 inputs of
    ``Model.inference_grouped``.  Rows are impression-major, so the groups of a batch are runs of equal
    impression id; the run boundaries are found on the host copy of the ids (no device sync)."""
    imp_host = row_impression_host[start:end]
    first = np.r_[True, imp_host[1:] != imp_host[:-1]]
    dev = dc.news_embedding.device
    uniq = torch.from_numpy(imp_host[first].astype(np.int64)).to(dev, non_blocking=True)
    row_group = torch.from_numpy((np.cumsum(first) - 1).astype(np.int32)).to(dev, non_blocking=True)
    cand = dc.row_candidate[start:end]
    H, d = dc.history.shape[1], dc.news_embedding.shape[1]
    hist = dc.history.index_select(0, uniq)
    user_rep = dc.news_embedding.index_select(0, hist.flatten()).view(uniq.shape[0], H, d)
    return (user_rep, *user_side_rows(dc, uniq),
            dc.user_category_indices.index_select(0, uniq), row_group, dc.SA_news_representations.index_select(0, cand),
            dc.news_graph.index_select(0, cand), dc.news_graph_mask.index_select(0, cand), dc.c_n0.index_select(0, cand))


class GroupedBatchPipeline:
    """Assembles the grouped inputs of batch k+1 on a side stream while batch k is being scored.

    The gathers of a batch are ~10 small kernels (60 us) that would otherwise sit between two encoder calls on the
    same stream.  ``batches`` lists the (start, end) row ranges in the order they will be taken.  The group structure
    of every batch (unique impressions, row -> group index) is computed once on the host and uploaded once; ``nsets`` sets
    of static buffers (user side sized for batch_size // 4 groups, the most the grouped entry takes) take turns, and
    events order gather -> score -> gather on each set.  A set is refilled only once the batch that last used it has been
    scored, so at most ``nsets`` batches are in flight: a driver that alternates over n streams wants nsets = n
    (``score_rows`` passes its lane count; with two sets a third lane only overlapped its prologue)."""

    def __init__(self, dc: DeviceCorpus, batches, row_impression_host: np.ndarray, nsets: int = 2, in_place_tables: bool = True,
                 news_sparse: Optional[bool] = None, reads: Optional[tuple] = None):
        """``reads``: what the encoder reads per row, of "news_graphs" (neighbourhood embeddings, adjacency, mask), "c_n0" and
        "ctx_layers" (the candidates' rows of ``dc.news_ctx_layers``) — an ablation encoder's ``PIPELINE_READS``; what is not named
        is not gathered and ``take`` hands out None in its place.  None (DIGAT): the news graphs and c_n0.
        ``news_sparse``: whether the encoder's Eq. 8 of the NEWS graph resolves to the sparse kernel at call time — the only
        reader that can take layer 0 of news graphs of more than 16 nodes from the per-news table; False leaves the table unused
        (in-batch projection).  None: trust the table's presence (prepare_news_side built it under the sparse mode)."""
        self.dc, self.batches = dc, list(batches)
        self.nsets = nsets = max(2, int(nsets))
        dev = dc.news_embedding.device
        self.dev = dev
        B = max(e - s for s, e in self.batches)
        Gmax = max(1, B // 4)
        H, d = dc.history.shape[1], dc.news_embedding.shape[1]
        U, C1 = dc.user_graph_size, dc.category_num + 1
        N = dc.news_graph.shape[1]
        ug_dtype = dc.user_graph.dtype if dc.user_graph is not None else torch.bool
        cm_dtype = dc.user_category_mask.dtype if dc.user_category_mask is not None else torch.bool

        import os
        in_place_tables = in_place_tables and os.environ.get("DIGAT_IN_PLACE", "1") != "0"          # A/B switch for measurements
        in_place = dc.news_hpq0 is not None and d % 4 == 0 and d <= 1024 and in_place_tables and not (N > 16 and news_sparse is False)
        gathered_tables = dc.news_hpq0 is not None and not in_place and N <= 16        # larger news graphs: in place or not at all
        if reads is not None and "ctx_layers" in reads and dc.news_ctx_layers is None:
            reads = None                          # no per-news context table (prepare_news_side has not run): the encoder computes the chain in-batch
        want_graphs = reads is None or "news_graphs" in reads
        want_c0 = reads is None or "c_n0" in reads
        self.ctx_layers = dc.news_ctx_layers if (reads is not None and "ctx_layers" in reads) else None
        K = 0 if self.ctx_layers is None else int(self.ctx_layers.shape[0])

        def bufs():
            return dict(hist=torch.empty((Gmax, H), dtype=torch.int64, device=dev),
                        user_rep=torch.empty((Gmax, H, d), dtype=torch.float32, device=dev),
                        user_graph=torch.empty((Gmax, U, U), dtype=ug_dtype, device=dev),
                        cat_mask=torch.empty((Gmax, C1), dtype=cm_dtype, device=dev),
                        cat_idx=torch.empty((Gmax, H), dtype=torch.int64, device=dev),
                        sa=(torch.empty((B, N, d), dtype=torch.float32, device=dev) if not in_place and want_graphs else None),
                        news_graph=(torch.empty((B, N, N), dtype=dc.news_graph.dtype, device=dev) if want_graphs else None),
                        news_mask=(torch.empty((B, N), dtype=dc.news_graph_mask.dtype, device=dev) if want_graphs else None),
                        c_n0=(torch.empty((B, d), dtype=torch.float32, device=dev) if want_c0 else None),
                        ctx_layers=(torch.empty((K * B * d,), dtype=torch.float32, device=dev) if K else None),
                        hpq=(torch.empty((3 * B * N * d,), dtype=torch.float32, device=dev) if gathered_tables else None),
                        hist_hpq=(torch.empty((3 * Gmax * H * d,), dtype=torch.float32, device=dev) if dc.user_hpq0 is not None else None),
                        ctxq=(torch.empty((3 * B * d,), dtype=torch.float32, device=dev) if dc.ctxq0 is not None else None))
        # the news side's layer-0 tables (and the node table behind them) are read IN PLACE through the candidate ids when the
        # encoder can (small news graphs: digat_encoder_fwd_grouped_cached's news_index): no gathered copies of 65 MB per batch
        self.in_place = in_place
        self.sets = [bufs() for _ in range(nsets)]
        uniq_parts, rg_parts, self.uo, self.ro = [], [], [0], [0]
        for s, e in self.batches:
            imp_b = row_impression_host[s:e]
            first = np.r_[True, imp_b[1:] != imp_b[:-1]]
            uniq_parts.append(imp_b[first].astype(np.int64))
            rg_parts.append((np.cumsum(first) - 1).astype(np.int32))
            self.uo.append(self.uo[-1] + int(first.sum()))
            self.ro.append(self.ro[-1] + (e - s))
        self.uniq_all = torch.from_numpy(np.concatenate(uniq_parts)).to(dev)
        self.row_group_all = torch.from_numpy(np.concatenate(rg_parts)).to(dev)
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))       # the corpus tables and the index arrays above
        self.ready = [torch.cuda.Event() for _ in range(nsets)]
        self.done = [None] * nsets
        self.meta = [None] * nsets
        self._gather(0)

    def _gather(self, k):
        if k >= len(self.batches):
            return
        s, e = self.batches[k]
        par = k % self.nsets
        G, n = self.uo[k + 1] - self.uo[k], e - s
        if 4 * G > n:                             # too few rows per group for the grouped entry: per-row path
            self.meta[par] = (k, None)
            return
        dc, b = self.dc, self.sets[par]
        uniq = self.uniq_all[self.uo[k]:self.uo[k + 1]]
        if self.done[par] is not None:
            self.stream.wait_event(self.done[par])                    # this set's previous batch has been scored
        with torch.cuda.stream(self.stream):
            # every gather of the batch in one launch (digat_gather_tables): 15 index_select kernels of ~9 us each before —
            # 7 % of the kernel time of a scoring step, on a stream that shares its hardware queue with the encoder's
            from . import _lib
            cand_ptr = dc.row_candidate.data_ptr() + 8 * s
            uniq_ptr = uniq.data_ptr()
            H, d = dc.history.shape[1], dc.news_embedding.shape[1]
            N = dc.news_graph.shape[1]
            hist_tab = dc.history.data_ptr()
            jobs = []

            def job(src, dst, row_bytes, rows, idx, idx2=0, inner=1):
                jobs.append((src, dst, row_bytes, rows, idx, idx2, inner))

            def rowb(t):
                return t[0].numel() * t.element_size()
            job(hist_tab, b["hist"].data_ptr(), rowb(dc.history), G, uniq_ptr)
            job(dc.news_embedding.data_ptr(), b["user_rep"].data_ptr(), d * 4, G * H, uniq_ptr, hist_tab, H)
            if dc.user_graph is not None:
                job(dc.user_graph.data_ptr(), b["user_graph"].data_ptr(), rowb(dc.user_graph), G, uniq_ptr)
                job(dc.user_category_mask.data_ptr(), b["cat_mask"].data_ptr(), rowb(dc.user_category_mask), G, uniq_ptr)
            job(dc.user_category_indices.data_ptr(), b["cat_idx"].data_ptr(), rowb(dc.user_category_indices), G, uniq_ptr)
            if b["sa"] is not None:
                job(dc.SA_news_representations.data_ptr(), b["sa"].data_ptr(), rowb(dc.SA_news_representations), n, cand_ptr)
            if b["news_graph"] is not None:
                job(dc.news_graph.data_ptr(), b["news_graph"].data_ptr(), rowb(dc.news_graph), n, cand_ptr)
                job(dc.news_graph_mask.data_ptr(), b["news_mask"].data_ptr(), rowb(dc.news_graph_mask), n, cand_ptr)
            if b["c_n0"] is not None:
                job(dc.c_n0.data_ptr(), b["c_n0"].data_ptr(), d * 4, n, cand_ptr)
            if b["ctx_layers"] is not None:
                for t in range(self.ctx_layers.shape[0]):      # [K, n, d] <- news_ctx_layers[t][candidate]
                    job(self.ctx_layers[t].data_ptr(), b["ctx_layers"].data_ptr() + 4 * t * n * d, d * 4, n, cand_ptr)
            if b["hist_hpq"] is not None:
                for t in range(3):             # [3, G*H, d] <- user_hpq0[t][history of the impression]
                    job(dc.user_hpq0[t].data_ptr(), b["hist_hpq"].data_ptr() + 4 * t * G * H * d, d * 4, G * H, uniq_ptr, hist_tab, H)
            if b["ctxq"] is not None:
                for t in range(3):             # [3, n, d] <- ctxq0[t][candidate]
                    job(dc.ctxq0[t].data_ptr(), b["ctxq"].data_ptr() + 4 * t * n * d, d * 4, n, cand_ptr)
            if b["hpq"] is not None:
                for t in range(3):             # contiguous [3, n, N, d] for this batch's n rows
                    job(dc.news_hpq0[t].data_ptr(), b["hpq"].data_ptr() + 4 * t * n * N * d, N * d * 4, n, cand_ptr)
            arr = (_lib.GatherJob * len(jobs))(*[_lib.GatherJob(*j) for j in jobs])
            _lib.check(_lib.lib().digat_gather_tables(arr, len(jobs), _lib.stream_ptr()), "digat_gather_tables")
            if dc.user_graph is None:          # no table to gather from: the groups' graphs and masks are built in the set's buffers
                user_graphs_from_indices(dc.user_category_indices, dc.category_num, rows=uniq, out=(b["user_graph"][:G], b["cat_mask"][:G]))
            self.ready[par].record(self.stream)
        self.meta[par] = (k, (G, n, self.row_group_all[self.ro[k]:self.ro[k + 1]]))

    def take(self, k):
        """The 9 inputs of ``Model.inference_grouped`` for batch k, or None (use ``gather_batch`` + ``inference``)."""
        par = k % self.nsets
        assert self.meta[par] is not None and self.meta[par][0] == k, "batches must be taken in order"
        info = self.meta[par][1]
        if info is None:
            return None
        G, n, row_group = info
        b = self.sets[par]
        torch.cuda.current_stream(self.dev).wait_event(self.ready[par])
        s0, e0 = self.batches[k]

        def rows(t):
            return t[:n] if t is not None else None
        sa = b["sa"][:n] if b["sa"] is not None else (self.dc.SA_news_representations if self.in_place else None)
        out = (b["user_rep"][:G], b["user_graph"][:G], b["cat_mask"][:G], b["cat_idx"][:G], row_group,
               sa, rows(b["news_graph"]), rows(b["news_mask"]), rows(b["c_n0"]))
        if b["ctx_layers"] is not None:          # an ablation encoder: no layer-0 tables, the candidates' context rows instead
            K_ = self.ctx_layers.shape[0]
            return out + (None, None, None, None, None, b["ctx_layers"][:K_ * n * self.dc.news_embedding.shape[1]].view(K_, n, -1))
        N_, d_ = self.dc.news_graph.shape[1], self.dc.news_embedding.shape[1]
        H_ = b["hist"].shape[1]
        news_hpq = b["hpq"][:3 * n * N_ * d_].view(3, n, N_, d_) if b["hpq"] is not None else (self.dc.news_hpq0 if self.in_place else None)
        news_index = self.dc.row_candidate[s0:e0] if self.in_place else None
        hist_hpq = b["hist_hpq"][:3 * G * H_ * d_].view(3, G, H_, d_) if b["hist_hpq"] is not None else None
        ctxq = b["ctxq"][:3 * n * d_].view(3, n, d_) if b["ctxq"] is not None else None
        if news_hpq is not None or hist_hpq is not None or ctxq is not None:
            out = out + (news_hpq, hist_hpq, self.dc.topic_hpq0 if hist_hpq is not None else None, ctxq, news_index)
        return out

    def scored(self, k):
        """Call once batch k's kernels are enqueued: the other buffer set may then be refilled for batch k+1."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.done[k % self.nsets] = ev
        self._gather(k + 1)

    def drain(self):
        """Make the current stream wait for every batch scored so far and for the gather stream: after this the pipeline (and
        its buffers, which the caching allocator may hand to someone else) can be dropped."""
        cur = torch.cuda.current_stream(self.dev)
        for ev in self.done:
            if ev is not None:
                cur.wait_event(ev)
        cur.wait_stream(self.stream)


_batch_streams = {}


def batch_streams(device, count: int = 3):
    """[current stream, extra streams ...] for scoring consecutive batches on alternating streams: a batch begins with
    small input-only kernels (user-node build, liveness, layer-0 projections of the groups) and ends with the last
    user context on the library's side stream — on one stream the GPU idles through both; with more, batch k+1's opening
    runs under batch k's last layer.  Every stream has its own scratch (``_lib.workspace`` is keyed by stream).
    Measured per 1024-row step (MIND-small shapes): 1 stream 1.48 ms, 2: 1.43, **3: 1.36**, 4: 1.48 — three batches in
    flight fill the phases where a batch has a single latency-bound kernel running (a kernel trace of the 2-stream run:
    no kernel 11 % of the time, one kernel 36 %).  The optimum depends on how the runtime maps the 2 x count + 1 streams to
    its 4 hardware queues: with 5 or more queues (GPU_MAX_HW_QUEUES) every count is slower (2.0-2.2 ms) — more kernels truly
    concurrent contend for the chip; without the library's side streams (DIGAT_PARAMS_SIDE_STREAM_OFF) two streams do as well as
    three with them (1.37 ms), one is worse (1.63 vs 1.48)."""
    cur = torch.cuda.current_stream(device)
    extra = _batch_streams.setdefault((device, cur.cuda_stream), [])
    while len(extra) < count - 1:
        extra.append(torch.cuda.Stream(device=device))
    return [cur] + extra[:count - 1]


# Rows one launch set scores.  The reference's dev batch (batch_size * 16 = 1024 rows, main.py:42) is what a 24 GB card's
# [B, n, n, d] activations allow; here rows are independent and nothing of that size exists, so consecutive dev batches are
# scored together: 4 096 rows per launch set fill the chip's 256 CUs better (the [B,d] linears, poolings and the news graph
# are 1-4 waves of workgroups at 1 024 rows).  Measured per 1 024 rows, three launch sets in flight: 1 024: 0.93 ms, 2 048:
# 0.92, 4 096: 0.80, 8 192: 0.80 — scores equal to the last fp32 bits or so (the [B,d] linears run on the tiled kernel from 2 048
# rows per pass up: DIGAT.pass_rows).
LAUNCH_ROWS = 4096


def launch_batches(start: int, end: int, batch_size: int, launch_rows: Optional[int] = None) -> List[Tuple[int, int]]:
    """Row ranges of the launch sets over [start, end): whole multiples of the caller's batch (``launch_rows`` rounded down
    to one, at least one batch)."""
    rows = LAUNCH_ROWS if launch_rows is None else launch_rows
    step = batch_size * max(1, rows // max(1, batch_size))
    return [(s, min(s + step, end)) for s in range(start, end, step)]


def _pass_rows(batch_size: int, launch_rows: Optional[int] = None) -> int:
    """Rows of a full launch set (what ``launch_batches`` steps by)."""
    rows = LAUNCH_ROWS if launch_rows is None else launch_rows
    return batch_size * max(1, rows // max(1, batch_size))


def range_overflow_any_rank(enc, world_size: int = 1, group=None, also: bool = False) -> bool:
    """Has an fp16x3 GEMM of ``enc`` met an activation beyond the format's range since the flag was last cleared — on ANY rank of
    ``group``?  Every rank gets the same answer (MAX all-reduce), so that all of them fall back to bf16x6 together: a per-rank
    decision would all-gather scores of two formats and leave the ranks' caches and weights_key diverged."""
    if not hasattr(enc, "range_overflowed"):
        return False
    hit = bool(enc.range_overflowed()) or bool(also)         # `also`: this rank's latch from prepare_news_side (DeviceCorpus.range_overflow_at_prepare)
    if world_size > 1:
        import torch.distributed as dist
        backend = dist.get_backend(group)
        dev = enc.topic_node_embedding.device if backend == "nccl" else torch.device("cpu")
        t = torch.tensor([1 if hit else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        hit = bool(int(t.item()))
    return hit


def score_rows(model, dc: DeviceCorpus, start: int, end: int, batch_size: int, grouped: bool = True,
               streams: int = 3, in_place_tables: bool = True, launch_rows: Optional[int] = None,
               check_range: bool = True) -> torch.Tensor:
    """Scores of rows [start, end): the hot loop of util.py:51-69.  ``grouped`` passes each impression's user
    tensors once (DIGAT: bit-identical scores, less work in layer 0; the ablation encoders: what does not depend on the
    candidate once per impression or per news); it needs the graph encoder's ``inference_grouped``.  ``grouped=False`` is the
    per-row entry, for every encoder.  ``streams``:
    consecutive launch sets alternate over this many HIP streams (same kernels, same bits: see ``batch_streams``).
    ``batch_size`` is the reference's dev batch; ``launch_rows`` (default ``LAUNCH_ROWS``) how many rows — whole batches — one
    pass through the encoder takes (``launch_rows=batch_size``: the reference's own chunking).

    ``check_range`` (default): when the projections ran in the range-limited fp16x3 format (what "auto" resolves to once
    ``prepare_news_side`` has seen the corpus), the encoder's range flag is read after the run — one host synchronisation — and a
    run that met an activation at or beyond |x| = 4094 is redone in bf16x6 ("auto"; the encoder stays there) or refused
    (explicit "fp16x3").  ``compute_scores`` passes False and makes the same decision for all ranks together.  Callers that drive
    ``model.inference`` / ``inference_grouped`` themselves after ``prepare_news_side`` (bench.py's timed loop) must read
    ``graph_encoder.range_overflowed()`` themselves."""
    enc0 = getattr(model, "graph_encoder", None)
    if enc0 is not None:
        apply_corpus_hint(enc0, dc)
    watch = check_range and hasattr(enc0, "range_overflowed") and enc0.gemm_format() == 1
    if watch:
        enc0.range_overflowed()            # clear what earlier calls may have left in the flag
    scores = _score_rows_once(model, dc, start, end, batch_size, grouped, streams, in_place_tables, launch_rows)
    # ... or the tables this run read were built from out-of-range activations (the layer-0 GEMMs run in prepare_news_side)
    if watch and (enc0.range_overflowed() or (dc.range_overflow_at_prepare and enc0.gemm_format() == 1)):
        _range_fallback(enc0, dc, batch_size)
        scores = _score_rows_once(model, dc, start, end, batch_size, grouped, streams, in_place_tables, launch_rows)
    return scores


def _range_fallback(enc, dc, batch_size):
    """An fp16x3 GEMM met an activation at or beyond the format's range (|x| >= 4094: node features of a deep layer, say): its
    results are degraded or inf.  Under "auto" the encoder moves to the range-free bf16x6 format (and stays there) and the
    per-news tables are rebuilt; an explicit "fp16x3" is the caller's word against the data's — refuse to return such scores."""
    if enc.projection_mode in ("fp16x3", "fp16-fp8c"):       # both explicit, both with fp16x3's range
        from ._lib import DigatHipError
        raise DigatHipError(f"projection_mode='{enc.projection_mode}': an activation left the format's range (|x| >= 4094); "
                            "use 'bf16x6' or 'auto'")
    import warnings
    warnings.warn("digat_amd: fp16x3 projections met activations beyond the format's range; re-scoring in bf16x6")
    enc.range_fallback = True
    prepare_news_side(enc, dc, batch_size)


def _score_rows_once(model, dc, start, end, batch_size, grouped, streams, in_place_tables, launch_rows):
    dev = dc.news_embedding.device
    scores = torch.empty(end - start, dtype=torch.float32, device=dev)
    batches = launch_batches(start, end, batch_size, launch_rows)
    enc = getattr(model, "graph_encoder", None)
    # the grouped route needs the GRAPH ENCODER's grouped entry (Model.inference_grouped only forwards to it); a model without a
    # graph encoder is taken at its word
    grouped = grouped and hasattr(model, "inference_grouped") and (enc is None or hasattr(enc, "inference_grouped"))
    if enc is not None:
        apply_corpus_hint(enc, dc)
    if hasattr(enc, "pass_rows") and batches:
        # the launch-set size names the kernel of the [B,d] linears for the whole run (tail set included); per-news tables made
        # under the other name are rebuilt (they hold the same linears' results)
        enc.pass_rows = _pass_rows(batch_size, launch_rows)
        if dc.weights_key is not None and dc.weights_key != weights_key(enc, dc):
            prepare_news_side(enc, dc, batch_size)
    lanes = batch_streams(dev, max(1, streams))
    # a single lane has nothing else to put under the user graph's kernels: there the library's side stream (news chain) stays on
    # for big passes too (4096 rows, one lane: 3.50 vs 3.64 ms; three lanes: 3.17 without it vs 3.29 with it — the default)
    # (a per-call, per-thread launch option — digat_params.flags — not a process-wide switch)
    if len(lanes) == 1 and hasattr(enc, "launch_options") and enc._launch_option("side_stream") == "auto":
        with enc.launch_options(side_stream="on"):
            return _score_sets(model, dc, start, batches, scores, lanes, grouped, in_place_tables)
    return _score_sets(model, dc, start, batches, scores, lanes, grouped, in_place_tables)


def _score_sets(model, dc, start, batches, scores, lanes, grouped, in_place_tables):
    enc = getattr(model, "graph_encoder", None)
    if not grouped and hasattr(enc, "launch_options") and enc._launch_option("detect_shared_users"):
        # grouped=False means the per-row entry as the reference's driver would call it WITHOUT the encoder's own search for
        # shared users (tests compare the two paths; drivers that want the search call model.inference themselves)
        with enc.launch_options(shared_users=False):
            return _score_sets(model, dc, start, batches, scores, lanes, grouped, in_place_tables)
    with torch.no_grad():
        news_sparse = (enc.resolved_xattn_mode("news") == "sparse") if hasattr(enc, "resolved_xattn_mode") else None
        pipe = (GroupedBatchPipeline(dc, batches, dc.row_impression.cpu().numpy(), nsets=len(lanes), in_place_tables=in_place_tables,
                                     news_sparse=news_sparse, reads=getattr(enc, "PIPELINE_READS", None))
                if grouped and batches else None)
        # the parameter block (split weights, folded queries) is (re)built on the first lane BEFORE the other lanes are
        # ordered after it: a rebuild inside the loop would run on one lane while the next batch reads it on the other
        if enc is not None and hasattr(enc, "_params") and batches:
            with torch.cuda.stream(lanes[0]):
                enc._params()
        for extra in lanes[1:]:
            extra.wait_stream(lanes[0])                       # the corpus tables, `scores`, the pipeline's index arrays
        for k, (s, e) in enumerate(batches):
            with torch.cuda.stream(lanes[k % len(lanes)]):
                inputs = pipe.take(k) if pipe is not None else None
                if inputs is not None:
                    scores[s - start:e - start] = model.inference_grouped(*inputs)
                else:
                    scores[s - start:e - start] = model.inference(*gather_batch(dc, s, e))
                if pipe is not None:
                    pipe.scored(k)
    for extra in lanes[1:]:
        lanes[0].wait_stream(extra)
    if pipe is not None:
        with torch.cuda.stream(lanes[0]):
            pipe.drain()                  # its buffers go back to the allocator when this function returns
    return scores


# ---- top-k recommendation ---------------------------------------------------------------------------------------------------------
# Pairs (user, candidate) that exist at once in ``recommend``: each costs 20 bytes outside the scoring pass (its two int64 row ids
# and its fp32 score), so 4 Mi pairs bound those arrays at 80 MiB; the pass's own buffers are sized by LAUNCH_ROWS, not by this.
RECOMMEND_MAX_ROWS = 4 << 20


def _ndim(x) -> int:
    return x.dim() if torch.is_tensor(x) else np.ndim(x)


def recommend_user_arrays(users, I: int, H: int, news_num: int, dev, names=("history", "user_category_indices")):
    """``users`` of a ``recommend`` in either form, checked and moved to ``dev``: ``(idx [G] int64, None, None)`` for a 1-D integer
    array of impression indices in [0, I), or ``(None, a [G,H] int64, b [G,H])`` for a pair of arrays called ``names`` that
    describes people who are no rows of the corpus (``a``: history ids in [0, news_num))."""
    as_t = lambda x: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if isinstance(users, (tuple, list)) and len(users) == 2 and _ndim(users[0]) == 2:
        a, b = as_t(users[0]).to(torch.int64), as_t(users[1])
        if tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"users must be ({names[0]} [G,H], {names[1]} [G,H]), got {tuple(a.shape)} and {tuple(b.shape)}")
        if int(a.shape[1]) != H:
            raise ValueError(f"users' history length {int(a.shape[1])} is not the corpus's max_history_num {H}")
        if a.numel() and (int(a.min()) < 0 or int(a.max()) >= news_num):
            raise ValueError(f"history ids must lie in [0, {news_num})")
        return None, a.to(dev).contiguous(), b.to(dev).contiguous()
    idx = as_t(users)
    if idx.dim() != 1 or idx.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise ValueError(f"users must be a 1-D integer array of impression indices or a ({names[0]}, {names[1]}) pair")
    idx = idx.to(torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= I):
        raise ValueError(f"impression indices must lie in [0, {I})")
    return idx.to(dev), None, None


def recommend_users(dc: DeviceCorpus, users):
    """The user side of ``recommend``: ``(history [G,H], user_category_indices [G,H], user_graph, user_category_mask)`` on the
    corpus's device.  ``users``: a 1-D integer array of impression indices of ``dc`` (the corpus's graph and mask tables are
    gathered when it has them), or a pair ``(history [G,H], user_category_indices [G,H])`` of users that are no rows of the
    corpus — padded as the corpus is (history id 0, category index C) — whose graphs are then derived on the device."""
    idx, hist, cat = recommend_user_arrays(users, int(dc.history.shape[0]), int(dc.history.shape[1]), int(dc.news_embedding.shape[0]),
                                           dc.history.device)
    if idx is None:
        return hist, cat.to(torch.int64), None, None
    graph = dc.user_graph.index_select(0, idx) if dc.user_graph is not None else None
    mask = dc.user_category_mask.index_select(0, idx) if dc.user_graph is not None else None
    return dc.history.index_select(0, idx), dc.user_category_indices.index_select(0, idx), graph, mask


def recommend_candidates(candidates, users: int, news_num: int):
    """``candidates`` of ``recommend`` as ``(ids int64 tensor, start int64 numpy [users + 1] or None)``: a 1-D pool shared by all
    users (``start`` None) or a pair ``(ids [R], start [users + 1])`` of per-user lists (CSR).  The ids stay where they are."""
    if isinstance(candidates, (tuple, list)) and len(candidates) == 2 and _ndim(candidates[0]) == 1 and _ndim(candidates[1]) == 1:
        ids, start = candidates
        start = np.asarray(start.cpu() if torch.is_tensor(start) else start).astype(np.int64)
        ids = torch.as_tensor(np.asarray(ids) if not torch.is_tensor(ids) else ids).to(torch.int64)
        if start.shape != (users + 1,):
            raise ValueError(f"candidate starts must have users + 1 = {users + 1} entries, got {start.shape}")
        if start[0] != 0 or np.any(np.diff(start) < 0):
            raise ValueError("candidate starts must begin at 0 and never decrease")
        if int(start[-1]) != int(ids.shape[0]):
            raise ValueError(f"the last candidate start ({int(start[-1])}) is not the number of candidate ids ({int(ids.shape[0])})")
    else:
        ids = torch.as_tensor(np.asarray(candidates) if not torch.is_tensor(candidates) else candidates)
        if ids.dim() != 1:
            raise ValueError("candidates must be a 1-D pool of news ids or a pair (ids [R], start [users + 1])")
        ids, start = ids.to(torch.int64), None
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= news_num):
        raise ValueError(f"candidate ids must lie in [0, {news_num})")
    return ids.contiguous(), start


def recommend_rows(g0: int, g1: int, ids: torch.Tensor, start: Optional[np.ndarray]):
    """The user-major (user, candidate) pairs of users [g0, g1): ``(row_impression [r], row_candidate [r], seg_start [g1-g0+1])``,
    int64 tensors on the device of ``ids``.  ``start`` None: every user meets the whole pool ``ids``; else user g meets
    ``ids[start[g]:start[g+1]]``."""
    dev, g = ids.device, g1 - g0
    users = torch.arange(g0, g1, dtype=torch.int64, device=dev)
    if start is None:
        P = int(ids.shape[0])
        return users.repeat_interleave(P), ids.repeat(g), torch.arange(g + 1, dtype=torch.int64, device=dev) * P
    seg = torch.from_numpy(start[g0:g1 + 1] - start[g0]).to(dev)
    rows = int(start[g1] - start[g0])
    return users.repeat_interleave(seg[1:] - seg[:-1], output_size=rows), ids[int(start[g0]):int(start[g1])], seg


def recommend_user_chunks(users: int, ids_len: int, start: Optional[np.ndarray], max_rows: int) -> List[Tuple[int, int]]:
    """Ranges [g0, g1) of consecutive users whose pairs number at most ``max_rows`` (a single user's own list may exceed it)."""
    if max_rows < 1:
        raise ValueError("max_rows must be positive")
    if start is None:
        step = max(1, max_rows // max(1, ids_len))
        return [(g, min(g + step, users)) for g in range(0, users, step)]
    out, g0 = [], 0
    while g0 < users:
        g1 = int(np.searchsorted(start, start[g0] + max_rows, side="right")) - 1
        g1 = min(users, max(g1, g0 + 1))
        out.append((g0, g1))
        g0 = g1
    return out


def recommend_limits(k, skip_len: int, long_lists: bool = False) -> int:
    """``k`` as an int, once it and the length of the skip rows (histories) are what ``evaluate.topk_segments`` takes — or, with
    ``long_lists``, what ``evaluate.shortlist_segments`` takes."""
    evaluate._check_limit(k, evaluate._SHORTLIST_LIMIT if long_lists else evaluate._TOPK_LIMIT)
    if skip_len > evaluate.TOPK_MAX_SKIP:
        raise ValueError(f"exclude_history takes histories of at most {evaluate.TOPK_MAX_SKIP} news, this corpus has {skip_len}")
    return int(k)


def recommend_select(G: int, k: int, ids: torch.Tensor, start: Optional[np.ndarray], skip: Optional[torch.Tensor], max_rows: int,
                     score: Callable, prepare: Optional[Callable] = None, long_lists: bool = False):
    """Select k per user over chunked (user, candidate) pairs: ``(news_ids [G,k] int64, scores [G,k] float32, count [G] int32)`` on
    the device of ``ids``, rows without pairs and slots at or beyond ``count`` holding id -1 and score -inf.  ``ids`` / ``start``
    as ``recommend_candidates`` returns them; ``skip`` [G, L] holds ids user g must not get, or None.  Users are taken in chunks
    of at most ``max_rows`` pairs (``recommend_user_chunks``); ``score(g0, g1, row_user, row_cand)`` returns the scores [r] of a
    chunk's pairs (``recommend_rows``), which ``evaluate.topk_segments`` selects from — ``topk_segments_host`` for host scores.
    ``prepare()`` runs once, behind the argument checks and before the first ``score``.  ``long_lists``: k up to
    ``evaluate.SHORTLIST_MAX_K``, selected by ``evaluate.shortlist_segments`` / ``shortlist_segments_host``."""
    k = recommend_limits(k, 0 if skip is None else int(skip.shape[1]), long_lists)
    on_device, on_host = ((evaluate.shortlist_segments, evaluate.shortlist_segments_host) if long_lists else
                          (evaluate.topk_segments, evaluate.topk_segments_host))
    chunks = recommend_user_chunks(G, int(ids.shape[0]), start, int(max_rows))
    if prepare is not None:
        prepare()
    out_ids = torch.full((G, k), -1, dtype=torch.int64, device=ids.device)
    out_scores = torch.full((G, k), float("-inf"), dtype=torch.float32, device=ids.device)
    out_count = torch.zeros((G,), dtype=torch.int32, device=ids.device)
    for g0, g1 in chunks:
        row_user, row_cand, seg = recommend_rows(g0, g1, ids, start)
        if int(row_user.shape[0]) == 0:
            continue
        scores, sk = score(g0, g1, row_user, row_cand), None if skip is None else skip[g0:g1]
        if scores.is_cuda:
            s, i, c = on_device(scores, seg, k, ids=row_cand, skip=sk)
        else:
            s, i, c = map(torch.from_numpy, on_host(scores.numpy(), seg.numpy(), k, ids=row_cand.numpy(),
                                                    skip=None if sk is None else sk.numpy()))
        out_scores[g0:g1], out_ids[g0:g1], out_count[g0:g1] = s, i, c
    return out_ids, out_scores, out_count


def refresh_news_side(model, dc: DeviceCorpus, batch_size: int) -> None:
    """What a run over ``dc`` needs of its news side, brought up to the model's weights: the news tables of the corpus it shares
    them with (``adopt_news_side``), the text news table, this corpus's sparse / dense hint, the per-news caches."""
    enc, ne = model.graph_encoder, getattr(model, "news_encoder", None)
    if hasattr(enc, "pass_rows"):
        enc.pass_rows = _pass_rows(batch_size)      # what score_rows will pass per call; weights_key names it: set before the keys are compared
    adopt_news_side(model, dc)
    if dc.title_text is not None and ne is not None and not hasattr(ne, "table"):
        # a text news encoder (MSA): util.py:24-33 re-encodes every news at the start of each dev / test run — here whenever the
        # encoder's weights have moved on since news_embedding was computed (training epochs), not otherwise
        nk = tuple((p.data_ptr(), p._version) for p in ne.parameters())
        if dc.news_key != nk:
            dc.news_embedding = cache_news_representations(ne, dc.title_text, dc.title_mask, max(batch_size, 4096))
            dc.news_key = nk               # a new tensor: weights_key below changes and the per-news caches follow
    apply_corpus_hint(enc, dc)
    if dc.c_n0 is None or dc.weights_key != weights_key(enc, dc):
        prepare_news_side(enc, dc, batch_size)      # first use, or the weights moved on since (an optimizer step, load_state_dict)


def unit_rows(table: torch.Tensor) -> torch.Tensor:
    """The rows of ``table`` [N, d] scaled to L2 norm 1 (float32, contiguous); a zero row stays zero.  What ``diversify`` measures
    DIGAT's news by: the inner product of two unit rows is their cosine."""
    t = table.detach().to(torch.float32)
    norm = t.norm(dim=1, keepdim=True)
    return (t / torch.where(norm > 0, norm, torch.ones_like(norm))).contiguous()


# ---- the greedy re-rank behind recommend(diversity= / calibration= / rerank=): one contract (evaluate.rerank_select_host), of which
# maximal marginal relevance and calibration are the two named reductions; one limits check, one stage and one driver serve all three
def _rerank_limits(k, shortlist, default_width, max_list) -> Tuple[int, int]:
    """``(k, k')`` of a re-ranked ``recommend``: the plain selection runs at ``k' = shortlist or min(max_list, default_width k)``."""
    if not 1 <= int(k) <= evaluate.TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {evaluate.TOPK_MAX_K}], got {k}")
    k = int(k)
    wide = min(max_list, default_width * k) if not shortlist else int(shortlist)
    if not k <= wide <= max_list:
        raise ValueError(f"shortlist must lie in [k, {max_list}] = [{k}, {max_list}], got {shortlist}")
    return k, wide


def _check_cap(max_per_category) -> None:
    if int(max_per_category) < 0:
        raise ValueError(f"max_per_category must be >= 0 (0: no cap), got {max_per_category}")


def diversify_limits(k, diversity, shortlist, max_per_category) -> Tuple[int, int, float]:
    """``(k, k', lam)`` of a diversified ``recommend``: the plain selection runs at ``k' = shortlist or min(128, 4 k)``, and
    ``evaluate.mmr_select`` cuts its lists to k with ``lam = 1 - diversity``."""
    k, wide = _rerank_limits(k, shortlist, 4, evaluate.MMR_MAX_LIST)
    if not 0.0 <= float(diversity) <= 1.0:
        raise ValueError(f"diversity must lie in [0, 1], got {diversity}")
    _check_cap(max_per_category)
    return k, wide, 1.0 - float(diversity)


def calibrate_limits(k, calibration, shortlist) -> Tuple[int, int, float]:
    """``(k, k', lam)`` of a calibrated ``recommend``: the plain selection runs at ``k' = shortlist or min(1024, 8 k)``, and
    ``calibrate`` cuts its lists to k with ``lam = 1 - calibration``."""
    k, wide = _rerank_limits(k, shortlist, 8, evaluate.CAL_MAX_LIST)
    if not 0.0 <= float(calibration) <= 1.0:
        raise ValueError(f"calibration must lie in [0, 1], got {calibration}")
    return k, wide, 1.0 - float(calibration)


def rerank_limits(k, rerank, shortlist, max_per_category) -> Tuple[int, int, Tuple[float, float]]:
    """``(k, k', (diversity, calibration))`` of a jointly re-ranked ``recommend``: the plain selection runs at ``k' = shortlist or
    min(1024, 8 k)`` and ``rerank`` cuts its lists to k with ``evaluate.rerank_weights(diversity, calibration)``."""
    k, wide = _rerank_limits(k, shortlist, 8, evaluate.RERANK_MAX_LIST)
    try:
        diversity, calibration = rerank
    except (TypeError, ValueError):
        raise ValueError(f"rerank must be a pair (diversity, calibration), got {rerank!r}") from None
    evaluate.rerank_weights(diversity, calibration)
    _check_cap(max_per_category)
    return k, wide, (float(diversity), float(calibration))


def _tensor_on(x, dev) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t if dev is None else t.to(dev)


def _rerank_stage(ids, scores, count, vectors, need_sim, category, target, on_device: Callable, on_host: Callable):
    """The fork ``diversify``, ``calibrate`` and ``rerank`` share.  ``category`` and ``target`` go onto the lists' device; with
    ``vectors`` a category array has one entry per row of them.  Device lists: ``on_device(category, target)``, an ``evaluate``
    wrapper.  CPU lists: ``on_host(ids, scores, count, sim, category, target)`` on numpy arrays, a host contract, ``sim`` the Gram
    of stock PyTorch (``evaluate.mmr_gram_stock``) where ``need_sim``.  Both return ``(scores, ids, count[, kl])``; the stage
    returns ``recommend``'s order ``(news_ids, scores, count[, kl])`` as tensors."""
    cat = None if category is None else _tensor_on(category, ids.device)
    tgt = None if target is None else _tensor_on(target, ids.device).to(torch.float32)
    if cat is not None and vectors is not None and (cat.dim() != 1 or int(cat.shape[0]) != int(vectors.shape[0])):
        raise ValueError(f"category must be [{int(vectors.shape[0])}], one entry per news, got shape {tuple(cat.shape)}")
    if ids.is_cuda:
        s, i, *rest = on_device(cat, tgt)
        return (i, s, *rest)
    host = lambda t: None if t is None else t.numpy()
    sim = evaluate.mmr_gram_stock(ids, vectors.detach().to(torch.float32)).numpy() if need_sim else None
    s, i, *rest = on_host(host(ids), host(scores), host(count), sim, host(cat), host(tgt))
    return tuple(torch.from_numpy(x) for x in (i, s, *rest))


def diversify(ids: torch.Tensor, scores: torch.Tensor, count: torch.Tensor, vectors: torch.Tensor, k: int, lam: float, category=None,
              max_per_category: int = 0):
    """The last stage of a diversified ``recommend``: the lists ``(ids [G,M], scores [G,M], count [G])`` of the plain selection cut
    to k by greedy maximal-marginal relevance over ``vectors`` [N, d] — ``evaluate.mmr_select`` on the device; on CPU tensors the
    Gram of stock PyTorch (``evaluate.mmr_gram_stock``) and ``evaluate.mmr_select_host``.  Returns ``recommend``'s triple
    ``(news_ids [G,k], scores [G,k], count [G])``."""
    q = int(max_per_category)
    if q > 0 and category is None:
        raise ValueError("max_per_category needs category, one entry per news")
    return _rerank_stage(
        ids, scores, count, vectors, True, category if q > 0 else None, None,
        lambda cat, _: evaluate.mmr_select(ids, scores, count, vectors, k, lam, category=cat, max_per_category=max_per_category),
        lambda i, s, c, sim, cat, _: evaluate.mmr_select_host(i, s, c, sim, k, lam, category=cat, max_per_category=max_per_category,
                                                              news_num=int(vectors.shape[0])))


def calibrate(ids: torch.Tensor, scores: torch.Tensor, count: torch.Tensor, category, target, k: int, lam: float, alpha: float = 0.01):
    """The last stage of a calibrated ``recommend``: the lists ``(ids [G,M <= 1024], scores [G,M], count [G])`` of the plain selection
    cut to k by the greedy calibrated re-rank towards ``target`` [G, C <= 64] under ``category`` [N] —
    ``evaluate.calibrated_select`` on device tensors, ``evaluate.calibrated_select_host`` on CPU tensors, as ``diversify`` does.
    Returns ``recommend``'s triple and the divergence of every finished list: ``(news_ids [G,k], scores [G,k], count [G], kl [G])``."""
    if category is None:
        raise ValueError("calibrate needs category, one entry per news")
    return _rerank_stage(ids, scores, count, None, False, category, target,
                         lambda cat, tgt: evaluate.calibrated_select(ids, scores, count, cat, tgt, k, lam, alpha),
                         lambda i, s, c, _, cat, tgt: evaluate.calibrated_select_host(i, s, c, cat, tgt, k, lam, alpha))


def rerank(ids: torch.Tensor, scores: torch.Tensor, count: torch.Tensor, vectors: torch.Tensor, k: int, diversity: float, calibration: float,
           category=None, target=None, alpha: float = 0.01, max_per_category: int = 0):
    """The last stage of a jointly re-ranked ``recommend``: the lists ``(ids [G,M <= 1024], scores [G,M], count [G])`` of the plain
    selection cut to k by ONE greedy pass that weighs an entry's score (``1 - diversity - calibration``) against its largest
    similarity over ``vectors`` [N, d <= 512] to what is already picked (``diversity``) and against what it does for the KL
    divergence between ``target`` [G, C <= 64] and the list's mix under ``category`` [N] (``calibration``), with at most
    ``max_per_category`` picks of one category — ``evaluate.rerank_select`` on device tensors; on CPU tensors the Gram of stock
    PyTorch (``evaluate.mmr_gram_stock``) and ``evaluate.rerank_select_host``, as ``diversify`` / ``calibrate`` do.  ``category``
    is needed by a calibration weight, a target or a cap; ``target`` by a calibration weight.  Returns ``recommend``'s triple and
    the divergence of every finished list (0 without a target): ``(news_ids [G,k], scores [G,k], count [G], kl [G])``."""
    w = evaluate.rerank_weights(diversity, calibration)
    rest = dict(alpha=alpha, max_per_category=max_per_category)
    return _rerank_stage(
        ids, scores, count, vectors, w[1] != 0, category, target,
        lambda cat, tgt: evaluate.rerank_select(ids, scores, count, vectors, k, *w, category=cat, target=tgt, **rest),
        lambda i, s, c, sim, cat, tgt: evaluate.rerank_select_host(i, s, c, sim, k, *w, category=cat, target=tgt, news_num=int(vectors.shape[0]),
                                                                   **rest))


def calibration_kl(ids: torch.Tensor, count, category, target, alpha: float = 0.01) -> torch.Tensor:
    """``kl`` [G] float32 of given lists ``ids`` [G, M <= 128] (``count`` [G] or None: M) against ``target`` [G, C]: the smoothed KL
    divergence ``calibrate`` reports, for any list — a plain top-k, a diversified one.  It is ``calibrate`` at ``lam = 1`` and
    ``k = M``, which picks every element."""
    M = int(ids.shape[1]) if ids.dim() == 2 else 0
    if not 1 <= M <= evaluate.TOPK_MAX_K:
        raise ValueError(f"ids must be [G, M] with 1 <= M <= {evaluate.TOPK_MAX_K}, got {tuple(ids.shape)}")
    return calibrate(ids, torch.zeros(tuple(ids.shape), dtype=torch.float32, device=ids.device), count, category, target, M, 1.0, alpha)[3]


def cap_category(category, max_per_category, corpus_category):
    """The category array a cap of ``max_per_category`` goes by: ``category``, else the corpus's own; a cap without either is
    refused.  Without a cap: ``category`` as given."""
    if int(max_per_category) > 0 and category is None:
        category = corpus_category
    if int(max_per_category) > 0 and category is None:
        raise ValueError("max_per_category needs category: this corpus carries no news_category")
    return category


def calibration_category(category, corpus_category) -> Tuple[torch.Tensor, int]:
    """``(category [N] int32, C)`` of a calibrated ``recommend``: ``category``, else the corpus's own, where it is; ``C = max + 1``."""
    if category is None:
        category = corpus_category
    if category is None:
        raise ValueError("calibration needs category: this corpus carries no news_category")
    cat = _tensor_on(category, None).to(torch.int32)
    if cat.dim() != 1:
        raise ValueError(f"category must be [N], one entry per news, got shape {tuple(cat.shape)}")
    C = max(1, int(cat.max()) + 1) if cat.numel() else 1
    if C > evaluate.CAL_MAX_CATEGORIES:
        raise ValueError(f"calibration takes at most {evaluate.CAL_MAX_CATEGORIES} categories, category names {C}")
    return cat, C


def _shortlist_then(select: Callable, wide, cut: Callable, category, max_per_category, corpus_category, wants_target: bool = False,
                    history: Optional[Callable] = None, calibration_target=None):
    """The driver behind the three ``shortlist_then_*``, the limits checked by its caller.  The category array: with
    ``wants_target`` ``calibration_category``'s, else with a cap ``cap_category``'s, else none — a refusal happens before anything is
    scored.  Then ``select(wide, long_lists)``, ``long_lists`` when ``wide > 128`` (never for the diversity path: its lists stop at
    128).  Then the target where one is wanted: ``calibration_target`` [G, C], or ``evaluate.category_share`` of ``history()``.
    Returns ``(shortlist triple, cut(shortlist triple, category, target))``."""
    cat, C = None, 0
    if wants_target:
        cat, C = calibration_category(category, corpus_category)
    elif int(max_per_category) > 0:
        cat = _tensor_on(cap_category(category, max_per_category, corpus_category), None).to(torch.int32)
    short = select(wide, wide > evaluate.TOPK_MAX_K)
    dev = short[0].device
    cat = None if cat is None else cat.to(dev)
    target = None
    if wants_target and calibration_target is None:
        target = evaluate.category_share(history().to(dev), cat, C)
    elif wants_target:
        target = _tensor_on(calibration_target, dev).to(torch.float32)
        if target.dim() != 2 or int(target.shape[0]) != int(short[0].shape[0]):
            raise ValueError(f"calibration_target must be [users = {int(short[0].shape[0])}, C], got {tuple(target.shape)}")
    return short, cut(short, cat, target)


def shortlist_then_diversify(select: Callable, vectors: Callable, k, diversities, shortlist=None, category=None, max_per_category: int = 0,
                             corpus_category=None):
    """The step behind ``recommend(diversity=)`` of either model, and behind ``recommend_report``: ``select(k', False)`` — the plain
    selection, once, at ``diversify_limits``' width — then ``diversify`` over ``vectors()`` for every value of ``diversities`` on
    that one shortlist, a cap going by ``cap_category(category, max_per_category, corpus_category)``.  Returns ``(shortlist triple,
    [recommend's triple per diversity])``."""
    limits = [diversify_limits(k, f, shortlist, max_per_category) for f in diversities]
    if not limits:
        raise ValueError("diversities must name at least one value")

    def cut(short, cat, _):
        vec = vectors()
        return [diversify(*short, vec, kk, lam, cat, max_per_category) for kk, _, lam in limits]
    return _shortlist_then(select, limits[0][1], cut, category, max_per_category, corpus_category)


def shortlist_then_calibrate(select: Callable, history: Callable, k, calibration, shortlist=None, category=None, corpus_category=None,
                             calibration_target=None, alpha: float = 0.01):
    """The step behind ``recommend(calibration=)`` of either model: ``select(k', long_lists)`` — the plain selection at
    ``calibrate_limits``' width, ``long_lists`` when ``k' > 128`` — then ``calibrate`` towards ``calibration_target`` or, without
    one, ``evaluate.category_share`` of ``history()`` [G, H] (news ids, padded with 0) under ``calibration_category``.  Returns
    ``(shortlist triple, (news_ids, scores, count, kl))``."""
    k, wide, lam = calibrate_limits(k, calibration, shortlist)
    evaluate._check_alpha(alpha)
    return _shortlist_then(select, wide, lambda short, cat, target: calibrate(*short, cat, target, k, lam, alpha), category, 0,
                           corpus_category, True, history, calibration_target)


def rerank_refusals(rerank, **others) -> None:
    """What ``recommend(rerank=)`` of either model refuses before anything is scored: ``rerank`` beside a re-rank of one kind or an
    index (``others``: the names and values of the arguments it does not combine with)."""
    if rerank is None:
        return
    named = [name for name, value in others.items() if value is not None]
    if named:
        raise ValueError(f"rerank does not combine with {', '.join(named)}: it names the diversity and the calibration weight itself")


def shortlist_then_rerank(select: Callable, vectors: Callable, history: Callable, k, rerank_knob, shortlist=None, category=None,
                          max_per_category: int = 0, corpus_category=None, calibration_target=None, alpha: float = 0.01):
    """The step behind ``recommend(rerank=(diversity, calibration))`` of either model: ``select(k', long_lists)`` — the plain
    selection at ``rerank_limits``' width, ``long_lists`` when ``k' > 128`` — then ``rerank`` over ``vectors()`` towards
    ``calibration_target`` or, without one, ``evaluate.category_share`` of ``history()`` under ``calibration_category``; a cap goes
    by the same category array.  With a calibration weight of 0 and no ``calibration_target`` there is no target and categories are
    needed by a cap alone (``cap_category``).  Returns ``(shortlist triple, (news_ids, scores, count, kl))``."""
    k, wide, (diversity, calibration) = rerank_limits(k, rerank_knob, shortlist, max_per_category)
    evaluate._check_alpha(alpha)
    cut = lambda short, cat, target: rerank(*short, vectors(), k, diversity, calibration, cat, target, alpha, max_per_category)
    return _shortlist_then(select, wide, cut, category, max_per_category, corpus_category,
                           calibration != 0.0 or calibration_target is not None, history, calibration_target)


# ---- the stage behind recommend(exposure_cap=): the one that works on the batch of lists (evaluate.capped_select_host) --------------
def exposure_limits(k, exposure_cap, shortlist, pool) -> Tuple[int, int]:
    """``(k, k')`` of an exposure-capped ``recommend``: the plain selection runs at ``k' = shortlist or min(1024, 8 k)`` and
    ``cap_exposure`` cuts its lists to k.  ``exposure_cap``: an int >= 0 or an integer array / tensor [pool]."""
    k, wide = _rerank_limits(k, shortlist, 8, evaluate.CAP_MAX_LIST)
    if torch.is_tensor(exposure_cap):
        if tuple(exposure_cap.shape) != (int(pool),) or exposure_cap.is_floating_point() or exposure_cap.dtype == torch.bool:
            raise ValueError(f"exposure_cap must be an int >= 0 or an integer tensor [news = {int(pool)}], got {tuple(exposure_cap.shape)} "
                             f"{exposure_cap.dtype}")
    else:
        evaluate.capped_caps_host(exposure_cap, pool)
    return k, wide


def exposure_refusals(exposure_cap, **others) -> None:
    """What ``recommend(exposure_cap=)`` of either model refuses before anything is scored: ``exposure_cap`` beside a re-rank, a
    draw, a cap per category or an index (``others``: the names and values of the arguments it does not combine with)."""
    if exposure_cap is None:
        return
    named = [name for name, value in others.items() if value is not None and not (isinstance(value, int) and value == 0)]
    if named:
        raise ValueError(f"exposure_cap does not combine with {', '.join(named)}: it cuts the plain shortlists of the whole call")


def cap_exposure(ids: torch.Tensor, scores: torch.Tensor, count, k: int, cap, pool: int, priority=None):
    """The last stage of an exposure-capped ``recommend``: the lists ``(ids [G,M <= 1024], scores [G,M], count [G])`` of the plain
    selection cut to k so that news ``id`` stays in at most ``cap[id]`` lists OF THIS CALL (``cap``: an int >= 0 for every news, or
    an integer array [pool]; 0 blocks a news) — the list-optimal stable assignment of ``evaluate.capped_select_host``: a stable
    assignment, not the one of largest total score.  ``priority`` [G,M] orders the lists that contend for a news (None: by score).
    ``evaluate.capped_select`` on device tensors, ``evaluate.capped_select_host`` on CPU tensors, as ``diversify`` and ``calibrate``
    do.  Returns ``(news_ids [G,k], scores [G,k], count [G], slots [G,k], rounds)``; a list whose shortlist runs out comes back with
    fewer than k entries — the remedy is a deeper shortlist."""
    if ids.dim() != 2 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError(f"ids and scores must both be [G, M], got {tuple(ids.shape)} and {tuple(scores.shape)}")
    pr = None if priority is None else _tensor_on(priority, ids.device).to(torch.float32)
    if ids.is_cuda:
        capv = cap.to(ids.device) if torch.is_tensor(cap) else cap
        return evaluate.capped_select(ids, scores, count, k, capv, pool, pr)
    host = lambda t: None if t is None else t.numpy()
    capv = cap.numpy() if torch.is_tensor(cap) else cap
    *arrays, rounds = evaluate.capped_select_host(host(ids), host(scores), host(count), k, capv, pool, host(pr))
    return tuple(torch.from_numpy(x) for x in arrays) + (rounds,)


def shortlist_then_cap(select: Callable, k, exposure_cap, pool, shortlist=None):
    """The step behind ``recommend(exposure_cap=)`` of either model: ``select(k', long_lists)`` — the plain selection of ALL users
    of the call at ``exposure_limits``' width, ``long_lists`` when ``k' > 128`` — then ``cap_exposure`` over those lists together.
    Returns ``(shortlist triple, (news_ids, scores, count, slots, rounds))``."""
    k, wide = exposure_limits(k, exposure_cap, shortlist, pool)
    short = select(wide, wide > evaluate.TOPK_MAX_K)
    return short, cap_exposure(*short, k, exposure_cap, pool)



def sample_limits(k, sample, shortlist) -> Tuple[int, int, float]:
    """``(k, k', temperature)`` of a sampled ``recommend``: the plain selection runs at ``k' = shortlist or min(1024, 8 k)``, and
    ``sample_lists`` draws one slate of k from it at temperature ``sample`` > 0."""
    if not 1 <= int(k) <= evaluate.PL_MAX_K:
        raise ValueError(f"k must be in [1, {evaluate.PL_MAX_K}], got {k}")
    if not 0.0 < float(sample) < float("inf"):                      # a NaN fails both comparisons
        raise ValueError(f"sample is a temperature: positive and finite, got {sample}")
    k = int(k)
    wide = min(evaluate.PL_MAX_LIST, 8 * k) if not shortlist else int(shortlist)
    if not k <= wide <= evaluate.PL_MAX_LIST:
        raise ValueError(f"shortlist must lie in [k, {evaluate.PL_MAX_LIST}] = [{k}, {evaluate.PL_MAX_LIST}], got {shortlist}")
    return k, wide, float(sample)


def sample_refusals(sample, seed, streams, **others) -> None:
    """What ``recommend(sample=)`` of either model refuses before anything is scored: ``sample`` beside a re-rank or an index
    (``others``: the names and values of the arguments it does not combine with), ``seed`` / ``streams`` without ``sample``."""
    if sample is None:
        if seed or streams is not None:
            raise ValueError("seed and streams belong to a sampled call: name sample (a temperature)")
        return
    named = [name for name, value in others.items() if value is not None and not (isinstance(value, int) and value == 0)]
    if named:
        raise ValueError(f"sample does not combine with {', '.join(named)}: the policy is Plackett-Luce over the plain shortlist")


def sample_lists(ids: torch.Tensor, scores: torch.Tensor, count, k: int, temperature: float, seed: int = 0, samples: int = 1, streams=None,
                 first_sample: int = 0):
    """Plackett-Luce slates from given lists ``(ids [G,M <= 1024], scores [G,M], count [G])`` — what ``recommend``,
    ``recommend_lists``, ``nrms.shortlist`` and ``score_lists`` return —: ``samples`` draws of k without replacement from
    ``softmax(scores / temperature)`` over every list's own entries, each with its probability.  Returns ``(news_ids [G,S,k] int64,
    scores [G,S,k] float32 — the input score bits —, n_out [G] int32, logp [G,S] float64, step_logp [G,S,k] float32)``: slots at or
    beyond ``n_out`` hold -1 / -inf.  ``evaluate.pl_sample`` on device tensors, ``evaluate.pl_sample_host`` on CPU tensors, as
    ``calibrate`` does; ``streams`` [G] (None: the list's index) and ``seed`` name the draws (``evaluate.pl_draws_host``)."""
    if ids.dim() != 2 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError(f"ids and scores must both be [G, M], got {tuple(ids.shape)} and {tuple(scores.shape)}")
    st = None if streams is None else _tensor_on(streams, ids.device)
    if ids.is_cuda:
        picks, n_out, logp, step = evaluate.pl_sample(scores, count, k, temperature, seed, samples, first_sample, st)
    else:
        picks, n_out, logp, step = map(torch.from_numpy, evaluate.pl_sample_host(
            scores.numpy(), None if count is None else count.numpy(), k, temperature, seed, samples, first_sample, None if st is None else st.numpy()))
    G, S, k = (int(x) for x in picks.shape)
    at = picks.to(torch.int64).clamp(min=0).view(G, S * k)
    hit = picks >= 0
    out_ids = torch.where(hit, ids.to(torch.int64).gather(1, at).view(G, S, k), torch.full_like(picks, -1, dtype=torch.int64))
    out_scores = torch.where(hit, scores.gather(1, at).view(G, S, k), torch.full_like(step, float("-inf")))
    return out_ids, out_scores, n_out, logp, step


def slate_positions(ids: torch.Tensor, count, slates: torch.Tensor) -> torch.Tensor:
    """``picks`` [G,S,k] int32: the position of every news of ``slates`` [G,S,k] in its user's list ``ids`` [G,M] (the first one
    below ``count``), -1 for a news that is absent and for a negative id."""
    G, M = int(ids.shape[0]), int(ids.shape[1])
    live = torch.arange(M, device=ids.device)[None, :] < (count.to(torch.int64)[:, None] if count is not None else M)
    picks = torch.empty(tuple(slates.shape), dtype=torch.int32, device=ids.device)
    rows = max(1, (1 << 24) // max(1, M * int(slates.shape[1]) * int(slates.shape[2])))
    for g0 in range(0, G, rows):                                    # [rows, S k, M] comparisons at a time
        sl = slates[g0:g0 + rows].to(torch.int64)
        eq = (sl.reshape(sl.shape[0], -1, 1) == ids[g0:g0 + rows, None, :].to(torch.int64)) & live[g0:g0 + rows, None, :]
        first = torch.where(eq, torch.arange(M, device=ids.device), torch.full((), M, device=ids.device, dtype=torch.int64)).amin(dim=2)
        found = (first < M) & (sl.reshape(sl.shape[0], -1) >= 0)
        picks[g0:g0 + rows] = torch.where(found, first, torch.full_like(first, -1)).view(sl.shape).to(torch.int32)
    return picks


def slate_log_prob(ids: torch.Tensor, scores: torch.Tensor, count, slates, temperature: float, differentiable: bool = False):
    """The probability of GIVEN slates under other scores — a logged slate under another model: ``slates`` [G,S,k] news ids are
    matched to positions of ``ids`` [G,M] (``slate_positions``) and ``evaluate.pl_log_prob`` (CPU tensors:
    ``evaluate.pl_log_prob_host``) gives ``logp`` [G,S] float64 and ``step_logp`` [G,S,k] float32 under ``softmax(scores /
    temperature)``.  A news that is absent from the list — or whose score there is not finite — ends the slate at that slot.
    Returns ``(logp, step_logp, covered [G,S] bool)``: ``covered`` says that every news of the slate (every slot with an id >= 0)
    was found and counted.  ``differentiable=True`` routes through ``evaluate.pl_scores``: the same ``logp`` bits on the device,
    with a gradient in ``scores`` — a DIGAT or ablation model whose list scores carry a graph can be trained on a log
    (``-(weight * logp).sum()``); on CPU tensors the stock composition in the dtype of ``scores``."""
    sl = _tensor_on(slates, ids.device)
    if sl.dim() != 3 or int(sl.shape[0]) != int(ids.shape[0]) or sl.is_floating_point():
        raise ValueError(f"slates must be integer news ids [G = {int(ids.shape[0])}, S, k], got {tuple(sl.shape)} {sl.dtype}")
    if ids.dim() != 2 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError(f"ids and scores must both be [G, M], got {tuple(ids.shape)} and {tuple(scores.shape)}")
    picks = slate_positions(ids, count, sl)
    if differentiable:
        logp, step = evaluate.pl_scores(scores, count, picks, temperature)
    elif ids.is_cuda:
        logp, step = evaluate.pl_log_prob(scores, count, picks, temperature)
    else:
        logp, step = map(torch.from_numpy, evaluate.pl_log_prob_host(scores.numpy(), None if count is None else count.numpy(), picks.numpy(),
                                                                     temperature))
    finite = torch.isfinite(scores.gather(1, picks.to(torch.int64).clamp(min=0).view(picks.shape[0], -1))).view(picks.shape)
    covered = ((sl < 0) | ((picks >= 0) & finite)).all(dim=2)
    return logp, step, covered


def slate_step_values(ids: torch.Tensor, scores: torch.Tensor, count, slates, temperature: float, values: torch.Tensor):
    """``slate_log_prob`` with the control variate of a doubly robust value: ``slates`` [G,S,k] news ids are matched to positions of
    ``ids`` [G,M] (``slate_positions``) and ``evaluate.pl_expect`` (CPU tensors: ``evaluate.pl_expect_host``) gives, under
    ``softmax(scores / temperature)``, ``logp`` [G,S] float64, ``step_logp`` [G,S,k] float32, ``step_mean`` [G,S,k] float64 — the
    expectation of ``values`` [G,M] (a value per item of every list) over what is left of the list at every step —, ``step_value``
    [G,S,k] float32 — the value of the item shown — and ``length`` [G,S] int32, the slot at which the slate ended.  Returns those
    five and ``covered`` [G,S] bool, ``slate_log_prob``'s."""
    sl = _tensor_on(slates, ids.device)
    if sl.dim() != 3 or int(sl.shape[0]) != int(ids.shape[0]) or sl.is_floating_point():
        raise ValueError(f"slates must be integer news ids [G = {int(ids.shape[0])}, S, k], got {tuple(sl.shape)} {sl.dtype}")
    if ids.dim() != 2 or tuple(scores.shape) != tuple(ids.shape) or tuple(values.shape) != tuple(ids.shape):
        raise ValueError(f"ids, scores and values must all be [G, M], got {tuple(ids.shape)}, {tuple(scores.shape)} and {tuple(values.shape)}")
    picks = slate_positions(ids, count, sl)
    if ids.is_cuda:
        out = evaluate.pl_expect(scores, count, picks, _tensor_on(values, ids.device), temperature)
    else:
        out = tuple(map(torch.from_numpy, evaluate.pl_expect_host(scores.numpy(), None if count is None else count.numpy(), picks.numpy(),
                                                                  values.numpy(), temperature)))
    finite = torch.isfinite(scores.gather(1, picks.to(torch.int64).clamp(min=0).view(picks.shape[0], -1))).view(picks.shape)
    covered = ((sl < 0) | ((picks >= 0) & finite)).all(dim=2)
    return out + (covered,)


def off_policy_report(log: dict, target_scores: torch.Tensor, reward, values=None, position_weight=None, temperature=None, clip=None,
                      units=None, replicates: int = 2000, level: float = 0.95, seed: int = 0):
    """What a target policy would have earned on a ``recommend_slates`` log, by four estimators side by side.  ``log``: that dict;
    ``target_scores`` [G,k']: the target's scores of the log's shortlist ``ids`` (``score_lists``); ``reward`` [G,S,k]: the reward at
    every position of every logged slate; ``values`` [G,k'] (optional): a model of an item's reward, scaled per position by
    ``position_weight`` [k] (None: ones); ``temperature`` None: the log's own.  The target's step probabilities and the model's
    per-step expectation come from one ``slate_step_values`` call.  Returns ``ips`` / ``snips`` (``evaluate.off_policy_value`` on the
    slate's summed reward and the slate-level weight, with its ``ess`` and ``max_weight``), ``pdis`` and — with ``values`` — ``dr``
    (``evaluate.off_policy_steps``, with ``step_ess`` / ``step_max_weight`` [k]), every one with ``metric_intervals``' fields, and
    ``n`` / ``dropped``: a slate that the target cannot draw in full (it ends earlier under the target than in the log) is left out
    and counted — with ``units`` given such a slate is a ``ValueError``, because the rows of a unit must stay contiguous."""
    ids, slates = log["ids"], log["slates"]
    T = float(log["temperature"] if temperature is None else temperature)
    tgt = _tensor_on(target_scores, ids.device)
    vals = torch.zeros_like(tgt, dtype=torch.float32) if values is None else _tensor_on(values, ids.device)
    logp, step, mean, used, length, _ = slate_step_values(ids, tgt, log["count"], slates, T, vals)
    G, S, k = (int(x) for x in slates.shape)
    r = np.asarray(evaluate._host(reward), dtype=np.float64)
    if r.shape != (G, S, k):
        raise ValueError(f"reward must be [G, S, k] = {(G, S, k)}, got {r.shape}")
    ln = evaluate._host(length).reshape(-1).astype(np.int64)
    ln_log = np.repeat(evaluate._host(log["n_out"]).astype(np.int64), S)
    keep = ln == ln_log
    dropped = int((~keep).sum())
    if dropped and units is not None:
        raise ValueError(f"{dropped} logged slates end earlier under the target than in the log: leave them out of the log and of units first")
    if not keep.any():
        raise ValueError("the target can draw none of the logged slates in full")
    rows = lambda x: np.asarray(evaluate._host(x), dtype=np.float64).reshape(G * S, -1)[keep]
    r2 = rows(r)
    shown = np.arange(k)[None, :] < ln[keep][:, None]
    slate = evaluate.off_policy_value(np.where(shown, r2, 0.0).sum(axis=1), rows(logp)[:, 0], rows(log["logp"])[:, 0], clip, units, replicates,
                                      level, seed)
    steps = evaluate.off_policy_steps(r2, rows(step), rows(log["step_logp"]), ln[keep], None if values is None else rows(mean),
                                      None if values is None else rows(used), position_weight, clip, units, replicates, level, seed,
                                      length_logging=ln_log[keep])
    out = {"ips": slate["ips"], "snips": slate["snips"], "pdis": steps["pdis"], "ess": slate["ess"], "max_weight": slate["max_weight"],
           "step_ess": steps["ess"], "step_max_weight": steps["max_weight"], "n": steps["n"], "dropped": dropped}
    if values is not None:
        out["dr"] = steps["dr"]
    return out


def shortlist_then_sample(select: Callable, k, sample, shortlist=None, seed: int = 0, streams=None, samples: int = 1):
    """The step behind ``recommend(sample=)`` of either model and ``recommend_slates``: ``select(k', long_lists)`` — the plain
    selection at ``sample_limits``' width, ``long_lists`` when ``k' > 128`` — then ``sample_lists``.  Returns ``(shortlist triple,
    (news_ids [G,S,k], scores [G,S,k], n_out [G], logp [G,S], step_logp [G,S,k]))``."""
    k, wide, temperature = sample_limits(k, sample, shortlist)
    evaluate._check_pl_args((1, wide), None, k, temperature, samples)               # refused before anything is scored
    short = select(wide, wide > evaluate.TOPK_MAX_K)
    return short, sample_lists(*short, k, temperature, seed, samples, streams)


def user_streams(users):
    """The default ``streams`` of a sampled ``recommend``: the impression indices where ``users`` are given as indices (a user's
    draws do not depend on who else is in the call), None — the list's index — for users given as arrays."""
    if isinstance(users, (tuple, list)) and len(users) == 2 and _ndim(users[0]) == 2:
        return None
    return users


def recommend_slates(model, dc: DeviceCorpus, users, candidates, k: int, temperature: float, samples: int = 1, seed: int = 0,
                     shortlist: Optional[int] = None, streams=None, exclude_history: bool = True, batch_size: int = 1024,
                     max_rows: int = RECOMMEND_MAX_ROWS):
    """The logging side of off-policy evaluation: the plain selection at ``k' = shortlist or min(1024, 8 k)`` and ``samples``
    Plackett-Luce slates of k per user from it at ``temperature``, each with its propensity.  Returns a dict: ``ids`` / ``scores``
    [G,k'] / ``count`` [G] — the shortlist, the support of the policy —, ``slates`` [G,S,k] int64, ``slate_scores`` [G,S,k],
    ``n_out`` [G], ``logp`` [G,S] float64, ``step_logp`` [G,S,k] float32, and ``temperature`` / ``seed``.  Another model's
    probability of the same slates: ``score_lists`` on ``ids`` / ``count``, then ``slate_log_prob``; ``evaluate.off_policy_value``
    takes both ``logp``.  ``streams`` None: ``user_streams``."""
    plain = lambda wide, long_lists: recommend_lists(model, dc, users, candidates, wide, exclude_history, batch_size, max_rows, long_lists)
    short, (slates, slate_scores, n_out, logp, step) = shortlist_then_sample(
        plain, k, temperature, shortlist, seed, user_streams(users) if streams is None else streams, samples)
    return {"ids": short[0], "scores": short[1], "count": short[2], "slates": slates, "slate_scores": slate_scores, "n_out": n_out,
            "logp": logp, "step_logp": step, "temperature": float(temperature), "seed": int(seed)}


def measure_lists(ids, count, vectors, category=None, base_ids=None, base_count=None, exposure=None):
    """``evaluate.list_quality`` on device lists; on CPU tensors the Gram of stock PyTorch (``evaluate.mmr_gram_stock``) and
    ``evaluate.list_quality_host``, as ``diversify`` does.  ``exposure`` [N] int32 is updated in place either way.  Returns the
    dict with the exposure in it."""
    if ids.is_cuda:
        return evaluate.list_quality(ids, count, vectors, category, base_ids, base_count, exposure)
    host = lambda t: None if t is None else t.numpy()
    q = evaluate.list_quality_host(ids.numpy(), host(count), evaluate.mmr_gram_stock(ids, vectors).numpy(), host(category), host(base_ids),
                                   host(base_count), int(vectors.shape[0]), host(exposure))
    if exposure is not None:
        exposure.copy_(torch.from_numpy(q["exposure"]).to(torch.int32))
    return q


def candidate_pool(candidates):
    """The ids of ``recommend``'s ``candidates`` in either form (``recommend_candidates``): the shared pool, or all ids of the
    per-user lists."""
    if isinstance(candidates, (tuple, list)) and len(candidates) == 2 and _ndim(candidates[0]) == 1 and _ndim(candidates[1]) == 1:
        return candidates[0]
    return candidates


def quality_report(select: Callable, mmr_vectors: Callable, quality_vectors: Callable, k, diversities, shortlist, category,
                   max_per_category, corpus_category, pool, targets=None, return_lists: bool = False):
    """The sweep behind ``recommend_report`` of either model: ``shortlist_then_diversify`` — one ``select``, every diversity's
    lists from that shortlist, the lists ``recommend(diversity=f)`` returns bit for bit — and after each ``diversify`` one
    ``measure_lists`` over ``quality_vectors()`` (unit rows: the similarities are cosines) with ``category``, else
    ``corpus_category``, else no category figures, the first k slots of the shortlist (the plain top-k) as the base list and an
    exposure histogram that starts from zero for every diversity.  Returns one dict per diversity: ``{"diversity": f,
    **evaluate.quality_summary(...)}`` with the coverage over ``pool`` (ids), and with ``targets = (target_ids [T], target_start
    [G+1])`` also ``recall@k``, ``user_recall@k`` and ``mrr`` of the lists (``evaluate.list_ranks``, ``evaluate.rank_metrics``).
    ``return_lists``: ``(rows, [triple per diversity])``."""
    if targets is not None and not (isinstance(targets, (tuple, list)) and len(targets) == 2):
        raise ValueError("targets must be None or a pair (target_ids [T], target_start [G+1])")
    diversities = [float(f) for f in diversities]
    short, lists = shortlist_then_diversify(select, mmr_vectors, k, diversities, shortlist, category, max_per_category, corpus_category)
    k = int(k)
    unit = quality_vectors()
    dev = short[0].device
    cat = category if category is not None else corpus_category
    if cat is not None:
        cat = torch.as_tensor(np.asarray(cat) if not torch.is_tensor(cat) else cat).to(dev, torch.int32)
    base_ids, base_count = short[0][:, :k].contiguous(), torch.clamp(short[2], max=k)
    rows = []
    for f, (ids, _, count) in zip(diversities, lists):
        exposure = torch.zeros((int(unit.shape[0]),), dtype=torch.int32, device=dev)
        q = measure_lists(ids, count, unit, cat, base_ids, base_count, exposure)
        row = {"diversity": f, **evaluate.quality_summary(q, exposure, pool)}
        if targets is not None:
            m = evaluate.rank_metrics(evaluate.list_ranks(ids, count, targets[0], targets[1]), targets[1], ks=(k,))
            row.update({name: m[name] for name in (f"recall@{k}", f"user_recall@{k}", "mrr")})
        rows.append(row)
    return (rows, lists) if return_lists else rows


def recommend_report(model, dc: DeviceCorpus, users, candidates, k: int, diversities=(0.0, 0.1, 0.3, 0.5), shortlist: Optional[int] = None,
                     category=None, max_per_category: int = 0, targets=None, exclude_history: bool = True, batch_size: int = 1024,
                     max_rows: int = RECOMMEND_MAX_ROWS, return_lists: bool = False):
    """What the ``diversity`` knob of ``recommend`` buys and costs, for every value of ``diversities``, at the price of ONE scoring
    pass: the plain selection runs once at ``k' = shortlist or min(128, 4 k)``, then every diversity's lists are cut from that
    shortlist (``diversify``) and measured (``evaluate.list_quality``).  The lists are the ones ``recommend(..., diversity=f,
    shortlist=, category=, max_per_category=)`` returns, bit for bit.  Returns one dict per diversity (``quality_report``):
    ``diversity``, then ``evaluate.quality_summary``'s ``ild`` / ``max_sim`` (cosines: ``unit_rows(dc.news_embedding)``),
    ``categories`` / ``category_max_share`` (``category``, else ``dc.news_category`` where the corpus has one; NaN without),
    ``overlap`` with the plain top-k, ``coverage`` / ``gini`` of the exposure over the candidate pool (the shared pool, or the
    distinct ids of per-user lists) and ``lists``; with ``targets = (target_ids, target_start)`` also ``recall@k``,
    ``user_recall@k`` and ``mrr``.  ``return_lists``: ``(rows, [(news_ids, scores, count) per diversity])``."""
    select = lambda wide, long_lists: recommend_lists(model, dc, users, candidates, wide, exclude_history, batch_size, max_rows, long_lists)
    unit = functools.lru_cache(maxsize=None)(lambda: unit_rows(dc.news_embedding))     # behind select: a text encoder's table is fresh then
    return quality_report(select, unit, unit, k, diversities, shortlist, category, max_per_category, dc.news_category,
                          candidate_pool(candidates), targets, return_lists)


def recommend(model, dc: DeviceCorpus, users, candidates, k: int, exclude_history: bool = True, batch_size: int = 1024,
              max_rows: int = RECOMMEND_MAX_ROWS, diversity: Optional[float] = None, shortlist: Optional[int] = None, category=None,
              max_per_category: int = 0, calibration: Optional[float] = None, calibration_target=None, alpha: float = 0.01,
              sample: Optional[float] = None, seed: int = 0, streams=None, rerank=None, exposure_cap=None):
    """For every user, which k news of its candidates, in order: ``(news_ids [G,k] int64, scores [G,k] float32, count [G] int32)``
    on the device.  Order: score descending, equal scores in candidate order (the rank file's order); ``count[g]`` is the number of
    valid slots of row g, the slots behind it hold id -1 and score -inf.

    ``users``: impression indices of ``dc``, or ``(history, user_category_indices)`` arrays of users that are no rows of the corpus
    (``recommend_users``).  ``candidates``: one pool of news ids for all users, or ``(ids, start)`` per user
    (``recommend_candidates``).  ``exclude_history``: a news of the user's history is never returned — histories are padded with
    id 0, so the PAD news is then never returned either; False takes the candidates at their word.

    Scoring is ``score_rows`` on a view of ``dc`` (same per-news tables and caches; the users' tensors and the user-major pairs in
    place of the corpus's impressions and rows), so the grouped route and the fp16x3 range check apply; selection and the chunks of
    at most ``max_rows`` pairs (``RECOMMEND_MAX_ROWS``: 20 bytes per pair, 80 MiB) are ``recommend_select``'s.  Like
    ``compute_scores`` this puts the model in eval mode and refreshes the per-news tables when the weights have moved on
    (``refresh_news_side``).  The chunking may move fp32 bits of a score (pass composition), as the launch-set size does.

    ``diversity`` in [0, 1] (None: off, the call above and nothing else): the selection above runs at ``k' = shortlist or
    min(128, 4 k)`` and ``diversify`` cuts every list to k by greedy maximal-marginal relevance with ``lam = 1 - diversity`` over
    ``unit_rows(dc.news_embedding)``: a pick's score is weighed against its largest cosine to what the user already got.
    ``max_per_category`` q >= 1 lets at most q news of one ``category`` [news_num] (None: ``dc.news_category``) into a list.  The
    scores returned are still the model's.

    ``calibration`` in [0, 1] (None: off) makes the list keep the reader's own category mix: the selection above runs at ``k' =
    shortlist or min(1024, 8 k)`` — calibration needs a deep pool, a user's rarer categories sit far down the list — and
    ``calibrate`` cuts every list to k with ``lam = 1 - calibration``, each pick weighing its score against what it does for the KL
    divergence between the target mix and the list's.  The target is ``evaluate.category_share`` of the users' histories under
    ``category`` (None: ``dc.news_category``; at most 64 categories), or ``calibration_target`` [G, C] as given; ``alpha`` smooths
    the list's mix.  A user with an empty history gets the plain top-k.  As for ``diversity``, ``lam`` weighs raw model scores
    against a gain of order 1: the useful range of the knob depends on the scale of the scores.  ``calibration`` and ``diversity``
    do not combine.

    ``sample`` — a temperature > 0 (None: off, the call as it was, bit for bit) — makes the list a DRAW: the selection above runs at
    ``k' = shortlist or min(1024, 8 k)`` and ``sample_lists`` draws one Plackett-Luce slate of k from ``softmax(score / sample)``
    over that shortlist; the triple returned is the slate in the order drawn, its scores the model's, ``count`` the slate's length.
    ``seed`` and ``streams`` [G] name the draws (``streams`` None: the impression indices where ``users`` are indices, so a user's
    slate does not depend on who else is in the call).  As ``sample`` goes to 0 the slate becomes the plain list.  ``sample`` does
    not combine with ``diversity``, ``calibration`` or ``max_per_category``; ``recommend_slates`` also returns the propensities.

    ``rerank=(diversity, calibration)`` (None: off, the call as it was, bit for bit) is both at once, in ONE objective: the
    selection above runs at ``k' = shortlist or min(1024, 8 k)`` and ``rerank`` cuts every list to k, each pick weighing its score
    (``1 - diversity - calibration``) against its largest cosine over ``unit_rows(dc.news_embedding)`` to what the user already got
    and against what it does for the KL divergence towards the target mix — so the penalty sees every pick calibration makes, and
    calibration picks from the deep pool.  Both weights lie in [0, 1], their sum at most 1.  ``shortlist``, ``category``,
    ``max_per_category``, ``calibration_target`` and ``alpha`` mean what they mean above; ``rerank=(d, 0)`` is maximal marginal
    relevance over up to 1024 entries.  ``rerank`` does not combine with ``diversity``, ``calibration`` or ``sample``.

    ``exposure_cap`` (None: off, the call as it was, bit for bit) bounds how often a news is shown ACROSS the lists of this call: an
    int c >= 0 — no news in more than c lists — or an integer array [news_num] of capacities (0 blocks a news).  The selection above
    runs ONCE over all users of the call at ``k' = shortlist or min(1024, 8 k)`` and ``cap_exposure`` sees every chunk's lists
    together: each list keeps its best k entries among those whose news still has room for it, a contested news going to the lists
    that score it highest, equal scores to the earlier user (``evaluate.capped_select_host``: the list-optimal stable assignment —
    stable, not the assignment of largest total score).  The cap holds PER CALL: two calls know nothing of each other, so users
    that should share one budget belong in one call.  A list whose shortlist runs out comes back with ``count < k``; the remedy is a
    deeper ``shortlist``.  ``exposure_cap`` does not combine with ``diversity``, ``calibration``, ``rerank``, ``sample`` or
    ``max_per_category``."""
    select = lambda wide, long_lists: recommend_lists(model, dc, users, candidates, wide, exclude_history, batch_size, max_rows, long_lists)
    return recommend_dispatch(select, lambda: unit_rows(dc.news_embedding), lambda: recommend_users(dc, users)[0], k,
                              getattr(dc, "news_category", None), user_streams(users), diversity, shortlist, category, max_per_category, calibration, calibration_target, alpha,
                              sample, seed, streams, rerank, exposure_cap=exposure_cap, news_num=lambda: int(dc.news_embedding.shape[0]))


def recommend_dispatch(select: Callable, vectors: Callable, history: Callable, k, corpus_category, streams_default, diversity=None,
                       shortlist=None, category=None, max_per_category=0, calibration=None, calibration_target=None, alpha=0.01, sample=None,
                       seed=0, streams=None, rerank=None, own_knobs=None, own_refusals: Optional[Callable] = None, exposure_cap=None,
                       news_num: Optional[Callable] = None):
    """The ladder behind ``recommend`` of either model — which knob runs which step, and every refusal, before anything is scored.
    ``select(k', long_lists)`` is the model's plain selection (the call without a knob is ``select(k, False)``), ``vectors()`` the
    rows a diversity term measures, ``history()`` the users' histories [G, H] padded with 0; the knobs are ``recommend``'s.
    ``own_knobs`` names the caller's further knobs that neither ``sample`` nor ``rerank`` combines with (``nrms``: index, refine),
    ``own_refusals()`` raises what else the caller refuses, behind those two.  ``exposure_cap`` (with ``news_num()``, the number of
    news its capacities are counted over) combines with ``shortlist`` alone.  Returns ``recommend``'s triple."""
    own_knobs = own_knobs or {}
    exposure_refusals(exposure_cap, diversity=diversity, calibration=calibration, calibration_target=calibration_target, rerank=rerank,
                      sample=sample, category=category, max_per_category=max_per_category, **own_knobs)
    sample_refusals(sample, seed, streams, diversity=diversity, calibration=calibration, calibration_target=calibration_target,
                    category=category, max_per_category=max_per_category, **own_knobs, rerank=rerank)
    rerank_refusals(rerank, diversity=diversity, calibration=calibration, **own_knobs)
    if own_refusals is not None:
        own_refusals()
    if exposure_cap is not None:
        return shortlist_then_cap(select, k, exposure_cap, news_num(), shortlist)[1][:3]
    if rerank is not None:
        return shortlist_then_rerank(select, vectors, history, k, rerank, shortlist, category, max_per_category, corpus_category,
                                     calibration_target, alpha)[1][:3]
    if sample is not None:
        ids, scores, n_out = shortlist_then_sample(select, k, sample, shortlist, seed, streams_default if streams is None else streams)[1][:3]
        return ids[:, 0].contiguous(), scores[:, 0].contiguous(), n_out
    if calibration is not None:
        if diversity is not None or max_per_category:
            raise ValueError("calibration does not combine with diversity or max_per_category: name one of them")
        return shortlist_then_calibrate(select, history, k, calibration, shortlist, category, corpus_category, calibration_target, alpha)[1][:3]
    if calibration_target is not None:
        raise ValueError("calibration_target belongs to a calibrated call: name calibration")
    if diversity is not None:
        return shortlist_then_diversify(select, vectors, k, (diversity,), shortlist, category, max_per_category, corpus_category)[1][0]
    if shortlist is not None or category is not None or max_per_category:
        raise ValueError("shortlist, category and max_per_category belong to a diversified call: name diversity (0.0: the cap alone)")
    return select(k, False)


def recommend_lists(model, dc: DeviceCorpus, users, candidates, k: int, exclude_history: bool = True, batch_size: int = 1024,
                    max_rows: int = RECOMMEND_MAX_ROWS, long_lists: bool = True):
    """``recommend`` without a re-rank — the same triple, order and fill; with ``long_lists`` for k up to
    ``evaluate.SHORTLIST_MAX_K`` = 1024 (``recommend_select``: ``evaluate.shortlist_segments``), the deep shortlist a calibrated
    re-rank picks from; for ``k <= 128`` the lists are ``recommend``'s, bit for bit."""
    hist, cat, graph, mask = recommend_users(dc, users)
    ids, start = recommend_candidates(candidates, int(hist.shape[0]), int(dc.news_embedding.shape[0]))
    prepare, score = recommend_scoring(model, dc, hist, cat, graph, mask, batch_size)
    return recommend_select(int(hist.shape[0]), k, ids.to(dc.news_embedding.device), start, hist if exclude_history else None,
                            max_rows, score, prepare, long_lists=long_lists)


def score_lists(model, dc: DeviceCorpus, users, ids, count=None, batch_size: int = 1024, max_rows: int = RECOMMEND_MAX_ROWS):
    """The model's scores of given per-user lists IN PLACE: ``scores`` [G, M] float32 on the device, slot ``j`` of row g belonging to
    ``ids[g, j]`` — ``-inf`` at or beyond ``count[g]`` (None: M) and for an id outside the corpus.  ``users`` as ``recommend`` takes
    them; ``ids`` [G, M] and ``count`` [G] are what ``recommend`` / ``nrms.shortlist`` return.  Nothing is selected, so M goes up to
    ``evaluate.SHORTLIST_MAX_K`` = 1024 where ``recommend`` stops at 128: a DIGAT (or ablation) teacher for an NRMS shortlist
    (``nrms.distil_retriever``).  The scoring closure and the chunks of at most ``max_rows`` pairs are ``recommend``'s: a slot holds the
    bits ``recommend`` returns for that id on the same per-user lists and ``max_rows``."""
    hist, cat, graph, mask = recommend_users(dc, users)
    G, N, dev = int(hist.shape[0]), int(dc.news_embedding.shape[0]), dc.news_embedding.device
    ids = torch.as_tensor(np.asarray(ids) if not torch.is_tensor(ids) else ids)
    if ids.dim() != 2 or int(ids.shape[0]) != G or ids.dtype in (torch.float16, torch.float32, torch.float64, torch.bool):
        raise ValueError(f"ids must be an integer array [users = {G}, M], got {tuple(ids.shape)} {ids.dtype}")
    M = int(ids.shape[1])
    if not 1 <= M <= evaluate.SHORTLIST_MAX_K:
        raise ValueError(f"a list holds between 1 and SHORTLIST_MAX_K = {evaluate.SHORTLIST_MAX_K} slots, got M = {M}")
    ids = ids.to(dev, torch.int64)
    if count is not None:
        count = torch.as_tensor(np.asarray(count) if not torch.is_tensor(count) else count).to(dev)
        if tuple(count.shape) != (G,):
            raise ValueError(f"count must have one entry per list ({G}), got shape {tuple(count.shape)}")
    elem = evaluate.list_elements(ids, count, N)
    start = np.concatenate([[0], np.cumsum(elem.sum(dim=1).cpu().numpy())]).astype(np.int64)
    flat = torch.nonzero(elem.view(-1)).view(-1)                     # row-major: user-major, slots ascending
    pairs = ids.view(-1).index_select(0, flat)
    out = torch.full((G * M,), float("-inf"), dtype=torch.float32, device=dev)
    prepare, score = recommend_scoring(model, dc, hist, cat, graph, mask, batch_size)
    chunks = recommend_user_chunks(G, int(pairs.shape[0]), start, int(max_rows))
    prepare()
    for g0, g1 in chunks:
        row_user, row_cand, _ = recommend_rows(g0, g1, pairs, start)
        if int(row_user.shape[0]) == 0:
            continue
        out[flat[int(start[g0]):int(start[g1])]] = score(g0, g1, row_user, row_cand).to(dev, torch.float32)
    return out.view(G, M)


def recommend_scoring(model, dc: DeviceCorpus, hist, cat, graph, mask, batch_size: int):
    """``(prepare, score)`` of ``recommend_select`` for the model's own scores of the users ``recommend_users`` returned: ``prepare()``
    puts the model in eval mode and refreshes the per-news tables; ``score(g0, g1, row_user, row_cand)`` is ``score_rows`` on a view
    of ``dc`` with the users' tensors and the user-major pairs in place of the corpus's impressions and rows.  ``recommend`` and
    ``score_lists`` both run on it."""
    def prepare():
        if hasattr(model, "eval"):
            model.eval()
        refresh_news_side(model, dc, batch_size)

    def score(g0, g1, row_user, row_cand):
        view = dataclasses.replace(dc, history=hist, user_category_indices=cat, user_graph=graph, user_category_mask=mask,
                                   row_impression=row_user, row_candidate=row_cand)
        scores = score_rows(model, view, 0, view.rows, batch_size)
        if view.weights_key != dc.weights_key:        # the range fallback rebuilt the per-news tables: on the view — keep them
            for f in ("SA_news_representations", "c_n0", "news_hpq0", "user_hpq0", "topic_hpq0", "ctxq0", "news_ctx_layers",
                      "weights_key", "xattn_hint", "range_overflow_at_prepare"):
                setattr(dc, f, getattr(view, f))
        return scores
    return prepare, score


def all_gather_scores(local: torch.Tensor, counts: List[int], group=None) -> torch.Tensor:
    """Concatenate every rank's block of scores in rank order (blocks are ragged: pad to the max)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    width = max(counts)
    padded = torch.zeros(width, dtype=local.dtype, device=local.device)
    padded[:local.numel()] = local
    out = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(out, padded, group=group)
    return torch.cat([o[:c] for o, c in zip(out, counts)])


_HEAP_FROZEN = False


def freeze_host_heap(force: bool = False) -> bool:
    """Take the objects alive NOW out of the reach of Python's cyclic garbage collector (``gc.collect(); gc.freeze()``).

    A driver loop of this package enqueues hundreds of launches per pass from Python and allocates a few thousand short-lived
    container objects per step; every few dozen steps that triggers a generation-2 collection, which walks EVERY tracked object of
    the process — with a corpus's Python-side structures resident that is 75-110 ms on the GPU boxes' hosts (round 5: one such pause
    inside a 60-step training region, 7.06 instead of 6.28 ms per step; the device sat idle at its end).  The reference's MIND_Corpus
    keeps dictionaries of millions of entries: the same pauses, longer.  Frozen objects are still freed by reference counting;
    they are just never walked again — which also means cyclic garbage that forms later AMONG them is never reclaimed: a
    process-global side effect the embedding application may not want.  So (round 6): at most ONCE per process however often the
    library's entry points are called (``compute_scores`` runs every dev epoch; ``force=True`` freezes again, for a driver that has
    just built another corpus), and not at all under ``DIGAT_FREEZE_HEAP=0``.  Returns whether this call froze anything."""
    global _HEAP_FROZEN
    if os.environ.get("DIGAT_FREEZE_HEAP", "1") == "0" or (_HEAP_FROZEN and not force):
        return False
    import gc
    gc.collect()
    gc.freeze()
    _HEAP_FROZEN = True
    return True


def compute_scores(model, dc: DeviceCorpus, batch_size: int, labels: Optional[np.ndarray] = None,
                   result_file: Optional[str] = None, rank: int = 0, world_size: int = 1, group=None,
                   score_fn: Optional[Callable] = None):
    """Score every row, rank candidates per impression, write the rank file, return
    ``(scores [R] cpu, (auc, mrr, ndcg5, ndcg10) or None)``.

    ``model`` needs ``.graph_encoder`` (for ``compute_news_graph_context``) and ``.inference``.
    With ``world_size > 1`` each rank scores its impression-aligned block and the blocks are
    all-gathered; metrics and the rank file are produced on rank 0 (the others return ``None`` metrics).
    ``score_fn(model, dc, start, end, batch_size)`` replaces the scorer (tests)."""
    if hasattr(model, "eval"):
        model.eval()
    freeze_host_heap()
    if score_fn is None:
        if hasattr(model.graph_encoder, "range_overflowed"):
            model.graph_encoder.range_overflowed()                  # clear what earlier calls may have left in the flag
        refresh_news_side(model, dc, batch_size)
    row_imp = dc.row_impression.cpu().numpy()
    start, end = shard_rows(row_imp, world_size, rank)
    enc = getattr(model, "graph_encoder", None)
    watch_range = score_fn is None and hasattr(enc, "range_overflowed")
    local = score_fn(model, dc, start, end, batch_size) if score_fn else score_rows(model, dc, start, end, batch_size, check_range=False)
    # the fp16x3 range check of score_rows, decided for ALL ranks together (a rank whose shard overflowed must not fall back alone)
    if watch_range and range_overflow_any_rank(enc, world_size, group, also=dc.range_overflow_at_prepare and enc.gemm_format() == 1):
        _range_fallback(enc, dc, batch_size)
        local = score_rows(model, dc, start, end, batch_size, check_range=False)
    if world_size > 1:
        counts = [shard_rows(row_imp, world_size, r) for r in range(world_size)]
        scores = all_gather_scores(local, [e - s for s, e in counts], group)
    else:
        scores = local
    scores_np = scores.detach().cpu().numpy()
    if rank != 0:
        return scores_np, None
    # ranking + metrics on the device (digat_rank_metrics); host tensors only occur in the CPU harness tests (score_fn)
    return scores_np, evaluate.ranks_metrics_file(scores, row_imp, labels, result_file)[1]


def compare_models(model_a, model_b, dc: DeviceCorpus, labels: np.ndarray, replicates: int = 2000, level: float = 0.95, seed: int = 0,
                   batch_size: int = 1024, score_fn: Optional[Callable] = None):
    """Is model_a better than model_b on this corpus?  Two ``compute_scores`` passes over ``dc``, the per-impression AUC / MRR /
    nDCG@5 / nDCG@10 of each (``evaluate.impression_metrics``: on the device for a CUDA corpus) and their PAIRED bootstrap over
    impressions (``evaluate.compare_metrics``: every replicate resamples the same impressions for both models).  Returns
    ``{"auc", "mrr", "ndcg5", "ndcg10"} -> {a, b, diff, lo, hi, se, p, wins}``; ``a`` and ``b`` are the metrics ``compute_scores``
    reports, to float64 rounding.  Any two models that score the same corpus will do — ``DIGAT`` against an ablation encoder, two
    checkpoints of one architecture.  The resampling unit is the impression; ``score_fn`` is ``compute_scores``'.  A model whose news encoder is a table scores
    with its own table (``dc.news_embedding`` is set to it, as the dev driver does)."""
    if labels is None:
        raise ValueError("labels are needed: a comparison of metrics has nothing to compare on an unlabelled split")
    row_imp = dc.row_impression.cpu().numpy()
    dev = dc.row_impression.device
    per = []
    for model in (model_a, model_b):
        if hasattr(getattr(model, "news_encoder", None), "table"):
            dc.news_embedding = model.news_encoder.table.detach()
        scores, _ = compute_scores(model, dc, batch_size, labels=None, score_fn=score_fn)
        per.append(evaluate.impression_metrics(torch.from_numpy(np.ascontiguousarray(scores)).to(dev), row_imp, labels))
    return evaluate.compare_metrics(per[0], per[1], names=evaluate.METRIC_NAMES, replicates=replicates, level=level, seed=seed)
