"""Drop-in ``--graph_encoder=DIGAT`` plugin backed by the gfx950 HIP kernels.

Mirrors the reference's class contract (graphEncoders.py:10-198): constructor
``DIGAT(config, news_embedding_dim)`` reading ``config.{news_graph_size, max_history_num,
category_num, graph_depth, dropout_rate}``; methods ``initialize``, ``forward`` (7 tensors),
``inference`` (8 tensors), ``compute_news_graph_context``, ``compute_user_graph_context``,
``compute_news_graph_embeddings``, ``compute_user_graph_embeddings``; attribute
``max_history_num``; and the same parameter names, so reference checkpoints load and the
trainer's ``'graph_encoder.'`` no-decay match still works.

All arithmetic happens in ``libdigat_hip.so`` through the C ABI (include/digat_hip.h).  There is
no eager / CPU fallback: tensors must be on the GPU and the extension must be built.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading

import torch
import torch.nn as nn

from . import _lib
from .layers import ScaledDotProductAttention

_TLS = threading.local()          # per-thread launch-option overrides, keyed by encoder (DIGAT.launch_options)


def derive_user_graph(user_graph, user_category_mask, user_category_indices, category_num: int):
    """``user_graph=None`` (and then ``user_category_mask=None``) means "derive both from ``user_category_indices``": they are a
    pure function of the indices (``util.user_graphs_from_indices``, one launch into Python-allocated buffers).  A given graph
    passes through untouched.  ``category_num``: C, without the padding bucket."""
    if user_graph is not None:
        return user_graph, user_category_mask
    if user_category_mask is not None:
        raise ValueError("user_graph=None derives the category mask too: pass user_category_mask=None")
    from .util import user_graphs_from_indices
    return user_graphs_from_indices(user_category_indices, category_num)


class GraphEncoder(nn.Module):
    def __init__(self, config, news_embedding_dim: int):
        super().__init__()
        self.news_graph_size = config.news_graph_size
        self.user_graph_size = config.max_history_num + config.category_num
        self.max_history_num = config.max_history_num
        self.category_num = config.category_num + 1          # +1: the padding bucket (E3)
        self.news_embedding_dim = news_embedding_dim
        self.graph_depth = config.graph_depth
        self.dropout_rate = float(config.dropout_rate)
        self.attention_scalar = math.sqrt(float(self.news_embedding_dim))
        self.topic_node_embedding = nn.Parameter(torch.zeros([config.category_num, self.news_embedding_dim]))

    def initialize(self):
        nn.init.zeros_(self.topic_node_embedding)

    def forward(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                user_category_mask, user_category_indices):
        raise Exception('Function forward must be implemented at sub-class')

    def inference(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                  user_category_mask, user_category_indices, news_graph_context):
        raise Exception('Function inference must be implemented at sub-class')


class DIGAT(GraphEncoder):
    def __init__(self, config, news_embedding_dim: int):
        super().__init__(config, news_embedding_dim)
        d, L = self.news_embedding_dim, self.graph_depth
        if d % 4 != 0:
            raise ValueError("digat_amd needs news_embedding_dim % 4 == 0 (float4 rows)")
        if L > _lib.DIGAT_MAX_DEPTH or max(self.news_graph_size, self.user_graph_size) > _lib.DIGAT_MAX_NODES:
            raise ValueError("graph_depth <= %d and graph sizes <= %d are supported"
                             % (_lib.DIGAT_MAX_DEPTH, _lib.DIGAT_MAX_NODES))
        # compute_news_graph_context
        self.candidate_attention = ScaledDotProductAttention(d, d, d)
        self.news_graph_W = nn.Linear(d * 2, d, bias=True)
        # compute_user_graph_context
        self.user_news_K = nn.Linear(d, d, bias=False)
        self.user_news_Q = nn.Linear(d, d, bias=True)
        self.featureAffine = nn.Linear(d, d, bias=True)
        self.userAttention = ScaledDotProductAttention(d, d, d)
        # Eq. 8 layers
        for g in ("news", "user"):
            setattr(self, f"{g}_graph_attention_W", nn.ModuleList([nn.Linear(d, d, bias=True) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn1", nn.ModuleList([nn.Linear(d, d, bias=False) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn2", nn.ModuleList([nn.Linear(d, d, bias=False) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn3", nn.ModuleList([nn.Linear(d, d, bias=True) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_a", nn.ModuleList([nn.Linear(d, 1, bias=False) for _ in range(L)]))
        self._param_block = None
        # node projections: "bf16x6" = fp32-equivalent product on the bf16 matrix cores (default), "bf16x6-pq3" = the same
        # for h, three of the six products for P and Q (they only feed the score: DIGAT_PROJ_PQ_X3), "fp32" = v_mfma_f32_16x16x4_f32;
        # BASELINE configs[4]: "pq-bf16" = pq3 + P', Q of the user graph's layers >= 1 STORED in bf16 (DIGAT_PQ_BF16; the
        # reference's quantised K3 + K1 + K2, README.md:62-66), "pq-bf16-x1" = the same with one bf16 product for P and Q;
        # "pq-fp8" = the same launches with P', Q stored as block-scaled OCP e4m3 (DIGAT_PQ_FP8: one fp32 scale per row and
        # 80-channel strip; the fp8 half of configs[4]);
        # "fp16x3" = every operand as two fp16 pieces, three products (digat_set_gemm_format(1): 0.7x the GEMM time, error at or
        # below an fp32 fma chain's against fp64 for |w| < 63, |x| < 4094 — fp16's range after the format's scaling);
        # "fp16-fp8c" (opt-in) = fp16x3 everywhere except the Eq. 8 node projections [W | ffn1 | ffn2] of every layer, whose two
        # correction products run on the block-scaled fp8 matrix cores (DIGAT_GEMM_F16F8C / DIGAT_PARAMS_PROJ_F16F8C: e4m3 with
        # one power-of-two scale per 32 K values; ~2^-15 of the result); fp16x3's range limits and range flag apply;
        # "auto" (default) = "fp16x3" when every projected weight is below 32 in magnitude, else "bf16x6" (no range limit)
        self.projection_mode = "auto"
        self._resolved_pm = None
        self._range_flag = None            # device word raised by the fp16x3 GEMMs on out-of-range activations (range_flag())
        self.range_fallback = False        # set by util.compute_scores after such a run: "auto" then resolves to bf16x6
        self.corpus_activation_max = None  # max |news representation| of the corpus, set by util.prepare_news_side
        # rows the driver passes through inference() per call (util.score_rows sets it to its launch-set size, util.LAUNCH_ROWS):
        # it NAMES the kernel of the [B,d] linears (>= 2048: tiled split-operand, below: split-image; DIGAT_PARAMS_BD_TILED) —
        # the row count of a call does not, so a row's bits do not depend on the batch it sits in
        self.pass_rows = 4096
        # Eq. 8 of the user graph: "auto" (the device counts the adjacency entries of the batch and runs the sparse
        # edge-list kernel or the dense tile + MFMA pair), "dense", "sparse" (digat_params.flags, include/digat_hip.h)
        self.user_xattn_mode = "auto"
        # ... and of news graphs of more than 16 nodes: "dense", "sparse" (DIGAT_NEWS_XATTN_SPARSE) or "auto" = dense until
        # util.prepare_news_side has looked at the corpus (there is no device-side decision for this graph)
        self.news_xattn_mode = "auto"
        self.corpus_xattn_hint = {}        # {"user": "sparse" | "dense", "news": ...}: set by util.prepare_news_side
        # per-call launch options (digat_params.flags bits 9-11; results do not depend on them, bit for bit):
        # side_stream "auto" = the news chain of a layer on the library's side stream for passes below 2 048 rows, "on" / "off" =
        # always / never; live_rows False = project, score and write every user-graph node (default: dead nodes are skipped).
        # ``launch_options(...)`` overrides them for the calling THREAD only — nothing here is process-wide.
        self.side_stream = "auto"
        self.live_rows = True
        # A/B switch of featureAffine's GEMM launch (digat_params.flags bits 13-14; results do not depend on it, bit for bit):
        # "long-first" = ragged 240-column tiles (3 + 2 strips at d = 400), the full-width tiles dispatched first, "row-major" = the
        # same tiles in row-tile-major order, "off" = one-strip tiles.  The environment sets the default so that a benchmark run
        # can be A/B'd (2.80 against 2.85 ms per step).
        self.ragged_tiles = os.environ.get("DIGAT_RAGGED_TILES", "long-first")
        # compute_user_graph_context of the folded inference path as ONE launch (csrc/digat_ctxfused.inc: topic pooling, featureAffine
        # and the SDPA pooling without T / T' leaving the CU; fp16x3 format, H <= 52, 192 < d <= 448, C + 1 <= 20).  OFF by default:
        # measured at parity with the three launches it replaces (round 6: 0.73 against 0.78 ms of kernel time per 4 096-row pass alone,
        # the same step time with three passes in flight, 3 % slower at 1 024 rows per pass — DESIGN.md section 4).  Read when the
        # parameter block is built (a weight version): set it before the first call.
        self.fused_user_context = False

    # ------------------------------------------------------------------ init (graphEncoders.py:76-101)
    def initialize(self):
        super().initialize()
        relu_gain = nn.init.calculate_gain('relu')
        leaky_gain = nn.init.calculate_gain('leaky_relu', 0.2)
        for g in ("news", "user"):
            for i in range(self.graph_depth):
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_W")[i].weight)
                nn.init.zeros_(getattr(self, f"{g}_graph_attention_W")[i].bias)
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_a")[i].weight, gain=leaky_gain)
                for f in ("ffn1", "ffn2", "ffn3"):
                    nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_{f}")[i].weight, gain=relu_gain)
                nn.init.zeros_(getattr(self, f"{g}_graph_attention_ffn3")[i].bias)
        self.candidate_attention.initialize()
        nn.init.xavier_uniform_(self.news_graph_W.weight)
        nn.init.zeros_(self.news_graph_W.bias)
        nn.init.xavier_uniform_(self.user_news_K.weight)
        nn.init.xavier_uniform_(self.user_news_Q.weight)
        nn.init.zeros_(self.user_news_Q.bias)
        nn.init.xavier_uniform_(self.featureAffine.weight, gain=relu_gain)
        nn.init.zeros_(self.featureAffine.bias)
        self.userAttention.initialize()

    @contextlib.contextmanager
    def launch_options(self, side_stream=None, live_rows=None, shared_users=None):
        """Override ``side_stream`` / ``live_rows`` for the calls the CURRENT THREAD makes inside the block (util.score_rows turns
        the side stream on for single-lane runs this way): another thread driving the same encoder keeps its own settings."""
        table = _TLS.__dict__.setdefault("opts", {})
        prev = table.get(id(self))
        cur = dict(prev or {})
        if side_stream is not None:
            if side_stream not in ("auto", "on", "off"):
                raise ValueError("side_stream must be 'auto', 'on' or 'off'")
            cur["side_stream"] = side_stream
        if live_rows is not None:
            cur["live_rows"] = bool(live_rows)
        if shared_users is not None:          # inference(): look for runs of identical consecutive user rows (False: the per-row entry as is)
            cur["detect_shared_users"] = bool(shared_users)
        table[id(self)] = cur
        try:
            yield self
        finally:
            if prev is None:
                table.pop(id(self), None)
            else:
                table[id(self)] = prev

    def _launch_option(self, name):
        return _TLS.__dict__.get("opts", {}).get(id(self), {}).get(name, getattr(self, name))

    def resolved_xattn_mode(self, g: str) -> str:
        """The Eq. 8 variant in force for graph ``g``: the explicit setting, or what ``util.prepare_news_side`` found in the
        corpus it was last shown while the setting is "auto" (``corpus_xattn_hint``); "auto" otherwise."""
        mode = getattr(self, f"{g}_xattn_mode", "auto")
        return self.corpus_xattn_hint.get(g, "auto") if mode == "auto" else mode

    # ------------------------------------------------------------------ parameter block for the C ABI
    def _apply(self, fn, *args, **kwargs):
        self._param_block = None          # .cuda() / .to() move the storages
        return super()._apply(fn, *args, **kwargs)

    def _params(self) -> "_lib.Params":
        # the matrix-core operand format ("fp16x3": two fp16 pieces, three products; everything else: three bf16 pieces, six
        # products) is a property of the split images made below and travels in P.flags: nothing process-wide
        pm = self.resolved_projection_mode()
        fmt = self.gemm_format()
        ptrs = tuple(p.data_ptr() for p in self.parameters())
        if self._param_block is not None and self._param_block[0] == ptrs and self._param_block[2] == self._fold_key():
            # the Eq. 8 variant and the launch options only select kernels (flags): they never invalidate the split weights or
            # the folded queries, so changing them (util.prepare_news_side's corpus hint, launch_options) must not rebuild them
            return self._call_block(self._param_block[1])
        for p in self.parameters():
            if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.DigatHipError("DIGAT parameters must be contiguous float32 CUDA tensors "
                                         "(call model.cuda()); there is no CPU path")
        P = _lib.Params()
        P.d, P.depth, P.category_num = self.news_embedding_dim, self.graph_depth, self.category_num - 1
        P.flags = self._flags()
        P.topic_node_embedding = self.topic_node_embedding.data_ptr()
        P.cand_K = self.candidate_attention.K.weight.data_ptr()
        P.cand_Q = self.candidate_attention.Q.weight.data_ptr()
        P.cand_bQ = self.candidate_attention.Q.bias.data_ptr()
        P.news_graph_W = self.news_graph_W.weight.data_ptr()
        P.news_graph_b = self.news_graph_W.bias.data_ptr()
        P.user_news_K = self.user_news_K.weight.data_ptr()
        P.user_news_Q = self.user_news_Q.weight.data_ptr()
        P.user_news_bQ = self.user_news_Q.bias.data_ptr()
        P.featureAffine_W = self.featureAffine.weight.data_ptr()
        P.featureAffine_b = self.featureAffine.bias.data_ptr()
        P.userAtt_K = self.userAttention.K.weight.data_ptr()
        P.userAtt_Q = self.userAttention.Q.weight.data_ptr()
        P.userAtt_bQ = self.userAttention.Q.bias.data_ptr()
        for g, arr in (("news", P.news), ("user", P.user)):
            for i in range(self.graph_depth):
                lp = arr[i]
                W = getattr(self, f"{g}_graph_attention_W")[i]
                lp.W, lp.bW = W.weight.data_ptr(), W.bias.data_ptr()
                lp.F1 = getattr(self, f"{g}_graph_attention_ffn1")[i].weight.data_ptr()
                lp.F2 = getattr(self, f"{g}_graph_attention_ffn2")[i].weight.data_ptr()
                F3 = getattr(self, f"{g}_graph_attention_ffn3")[i]
                lp.F3, lp.b3 = F3.weight.data_ptr(), F3.bias.data_ptr()
                lp.a = getattr(self, f"{g}_graph_attention_a")[i].weight.data_ptr()
        # bf16x6 projections: split [W | ffn1 | ffn2] of every layer into three bf16 planes (once per weight version)
        P._splits = []
        if pm in ("bf16x6", "bf16x6-pq3", "pq-bf16", "pq-bf16-x1", "pq-fp8", "fp16x3", "fp16-fp8c") and self.news_embedding_dim % 80 == 0:
            L_ = _lib.lib()
            d = self.news_embedding_dim
            # the layers' images: "fp16-fp8c" splits them in their own format (every other image of the block stays fp16x3)
            lfmt = _lib.GEMM_F16F8C if pm == "fp16-fp8c" else fmt
            nbytes = L_.digat_split_weights_bytes_format(3 * d, d, lfmt)
            for g, arr in (("news", P.news), ("user", P.user)):
                for i in range(self.graph_depth):
                    buf = _lib.split_buffer(nbytes, self.topic_node_embedding.device)
                    _lib.check(L_.digat_split_proj_weights(
                        getattr(self, f"{g}_graph_attention_W")[i].weight.data_ptr(),
                        getattr(self, f"{g}_graph_attention_ffn1")[i].weight.data_ptr(),
                        getattr(self, f"{g}_graph_attention_ffn2")[i].weight.data_ptr(), d, buf.data_ptr(), lfmt,
                        _lib.stream_ptr()), "digat_split_proj_weights")
                    arr[i].wsplit = buf.data_ptr()
                    P._splits.append(buf)
            buf = _lib.split_buffer(L_.digat_split_weights_bytes(d, d), self.topic_node_embedding.device)
            _lib.check(L_.digat_split_weights(self.featureAffine.weight.data_ptr(), d, d, buf.data_ptr(), fmt, _lib.stream_ptr()),
                       "digat_split_weights")
            P.featureAffine_wsplit = buf.data_ptr()
            P._splits.append(buf)
            if fmt == _lib.GEMM_F16X3:           # one device word the fp16x3 GEMMs raise when an activation leaves the format's range
                P.range_flag = self.range_flag().data_ptr()
        # inference: fold the key projections into the query weights once per weight version
        P._folds = None
        if not self.training:
            P._folds = self._fold_attention()
            (P.cand_fold_W, P.cand_fold_b, P.user_news_fold_W, P.user_news_fold_b,
             P.userAtt_fold_W, P.userAtt_fold_b) = (t.data_ptr() for t in P._folds)
            if P._splits:
                # the [B,d] linears of the folded path on split images too (gemm_skinny_split_kernel): K3 of the news graph,
                # the candidate query, the gate, and per layer the three matrices applied to the news context
                L_, d, dev = _lib.lib(), self.news_embedding_dim, self.topic_node_embedding.device

                def image(rows, K, fn, *args):
                    buf = _lib.split_buffer(L_.digat_split_weights_bytes(rows, K), dev)
                    _lib.check(fn(*args, buf.data_ptr(), fmt, _lib.stream_ptr()), "split")
                    P._splits.append(buf)
                    return buf.data_ptr()
                for i in range(self.graph_depth):
                    P.news[i].f3_wsplit = image(d, d, L_.digat_split_weights, self.news_graph_attention_ffn3[i].weight.data_ptr(), d, d)
                P.cand_fold_wsplit = image(d, d, L_.digat_split_weights, P.cand_fold_W, d, d)
                P.gate_wsplit = image(d, 2 * d, L_.digat_split_weights, self.news_graph_W.weight.data_ptr(), d, 2 * d)
                for l in range(self.graph_depth + 1):
                    third = self.user_graph_attention_ffn3[l].weight.data_ptr() if l < self.graph_depth else P.userAtt_fold_W
                    P.ctx_wsplit[l] = image(3 * d, d, L_.digat_split_proj_weights, P.user_news_fold_W, P.userAtt_fold_W, third, d)
                if fmt == _lib.GEMM_F16X3 and self.fused_user_context:
                    # compute_user_graph_context as one launch (csrc/digat_ctxfused.inc): featureAffine in the fused kernel's lane order
                    buf = _lib.split_buffer(L_.digat_split_ctx_fused_bytes(d), dev)
                    _lib.check(L_.digat_split_ctx_fused_weights(self.featureAffine.weight.data_ptr(), d, buf.data_ptr(), _lib.stream_ptr()),
                               "digat_split_ctx_fused_weights")
                    P._splits.append(buf)
                    P.featureAffine_fsplit = buf.data_ptr()
        self._param_block = (ptrs, P, self._fold_key())
        return self._call_block(P)

    def _call_block(self, P):
        """The parameter block one call hands to the library: a COPY of the cached block (2.6 KB of pointers) with this call's
        flags — two threads with different launch options never write the same struct."""
        Q = _lib.Params.from_buffer_copy(P)
        Q.flags = self._flags()
        return Q

    def resolved_projection_mode(self) -> str:
        """``projection_mode`` with "auto" resolved from the weights' range (once per weight version; one host sync)."""
        return self._auto_base() if self.projection_mode == "auto" else self.projection_mode

    def gemm_format(self) -> int:
        """The operand format of this encoder's split weight images: fp16x3 when asked for, and under "auto" / "pq-bf16" whenever
        the range conditions of ``_auto_base`` hold; bf16x6 otherwise."""
        pm = self.projection_mode
        if pm in ("fp16x3", "fp16-fp8c") or (pm in ("auto", "pq-bf16", "pq-fp8") and self._auto_base() == "fp16x3"):
            return _lib.GEMM_F16X3
        return _lib.GEMM_BF16X6

    def _auto_base(self) -> str:
        if self.news_embedding_dim % 80 != 0:
            return "bf16x6"
        ws = [m.weight for g in ("news", "user") for f in ("W", "ffn1", "ffn2") for m in getattr(self, f"{g}_graph_attention_{f}")]
        ws.append(self.featureAffine.weight)
        key = tuple((w.data_ptr(), w._version) for w in ws + [self.topic_node_embedding])
        key += (self.corpus_activation_max, self.range_fallback)
        if self._resolved_pm is None or self._resolved_pm[0] != key:
            amax = self.corpus_activation_max
            # fp16x3 needs a driver that looks at the range flag after the run: util.score_rows and util.compute_scores do (and
            # redo the run in bf16x6); "auto" therefore picks it only once util.prepare_news_side has seen the corpus — plain
            # forward / inference calls get the range-free bf16x6.  A caller that runs prepare_news_side and then drives
            # inference / inference_grouped itself (bench.py's timed loop) must read range_overflowed() after its run.  Then: weights below 32 (the format holds 63), the topic nodes and the
            # corpus's news representations below 256 (the format holds 4094; what the features of layers >= 1 grow to is
            # checked on the device, by the GEMM itself); nan compares false
            ok = amax is not None and not self.range_fallback
            if ok:
                wmax = float(torch.stack([w.detach().abs().max() for w in ws]).max())
                tmax = float(self.topic_node_embedding.detach().abs().max())
                ok = wmax < 32.0 and amax < 256.0 and tmax < 256.0
            self._resolved_pm = (key, "fp16x3" if ok else "bf16x6")
        return self._resolved_pm[1]

    def range_flag(self) -> torch.Tensor:
        """The device word the fp16x3 GEMMs OR 1 into when an activation reaches the format's range (digat_params.range_flag)."""
        dev = self.topic_node_embedding.device
        if self._range_flag is None or self._range_flag.device != dev:
            self._range_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._range_flag

    def range_overflowed(self, reset: bool = True) -> bool:
        """True when an fp16x3 GEMM of this encoder has seen an activation at or beyond the format's range since the last
        reset (one host synchronisation: call it once per scoring run, as util.compute_scores does)."""
        if self._range_flag is None:
            return False
        hit = bool(int(self._range_flag.item()))
        if reset and hit:
            self._range_flag.zero_()
        return hit

    def _flags(self) -> int:
        """digat_params.flags (include/digat_hip.h): Eq. 8 variant of the user graph (bits 0-1), DIGAT_PROJ_PQ_X3 (bit 2),
        DIGAT_NEWS_XATTN_SPARSE (bit 3), ..., DIGAT_PARAMS_BD_TILED (bit 7: ``pass_rows``)."""
        pm = self.projection_mode
        return ({"auto": 0, "dense": 1, "sparse": 2}[self.resolved_xattn_mode("user")]
                | (4 if pm in ("bf16x6-pq3", "pq-bf16", "pq-fp8") else 0)
                | (8 if self.resolved_xattn_mode("news") == "sparse" else 0)
                | (16 if pm in ("pq-bf16", "pq-bf16-x1") else 0)         # DIGAT_PQ_BF16: P', Q of Eq. 8 stored in bf16
                | (32 if pm == "pq-bf16-x1" else 0)                      # DIGAT_PQ_X1: ... and computed with one bf16 product
                | (256 if pm == "pq-fp8" else 0)                         # DIGAT_PQ_FP8: P', Q of Eq. 8 stored as block-scaled e4m3
                | (_lib.PARAMS_GEMM_F16X3 if self.gemm_format() == _lib.GEMM_F16X3 else 0)
                | (_lib.PARAMS_PROJ_F16F8C if pm == "fp16-fp8c" else 0)  # ... except the layers' images: fp16 + MX-e4m3 corrections
                | (_lib.PARAMS_BD_TILED if self.pass_rows >= 2048 else 0)
                | {"auto": 0, "off": _lib.PARAMS_SIDE_STREAM_OFF, "on": _lib.PARAMS_SIDE_STREAM_ON}[self._launch_option("side_stream")]
                | (0 if self._launch_option("live_rows") else _lib.PARAMS_NO_LIVE_ROWS)
                | {"long-first": 0, "row-major": _lib.PARAMS_RAGGED_ROWMAJOR, "off": _lib.PARAMS_RAGGED_OFF}[self.ragged_tiles])

    def _fold_sources(self):
        ca, ua = self.candidate_attention, self.userAttention
        return ((ca.K.weight, ca.Q.weight, ca.Q.bias), (self.user_news_K.weight, self.user_news_Q.weight,
                                                        self.user_news_Q.bias), (ua.K.weight, ua.Q.weight, ua.Q.bias))

    def _fold_key(self):
        key = (self.training, self.resolved_projection_mode(), self.gemm_format()) + tuple(t._version for trio in self._fold_sources() for t in trio)
        for g in ("news", "user"):
            for f in ("W", "ffn1", "ffn2"):
                key += tuple(m.weight._version for m in getattr(self, f"{g}_graph_attention_{f}"))
        return key + (self.featureAffine.weight._version, bool(self.fused_user_context))

    def _fold_attention(self):
        """(K x).(Q c + b) = x.(Wf c + bf) with Wf = K^T Q, bf = K^T b, computed by the library itself."""
        L = _lib.lib()
        d = self.news_embedding_dim
        dev = self.topic_node_embedding.device
        nbytes = L.digat_fold_workspace_bytes(d)
        ws = _lib.workspace(nbytes, dev, "fold")
        out = []
        for K, Q, b in self._fold_sources():
            Wf = torch.empty((d, d), dtype=torch.float32, device=dev)
            bf = torch.empty((d,), dtype=torch.float32, device=dev)
            _lib.check(L.digat_fold_attention(K.data_ptr(), Q.data_ptr(), b.data_ptr(), Wf.data_ptr(), bf.data_ptr(), d,
                                              ws.data_ptr(), nbytes, _lib.stream_ptr()), "digat_fold_attention")
            out += [Wf, bf]
        return out

    def _eval_only(self, what: str):
        if self.training and self.dropout_rate > 0 and torch.is_grad_enabled():
            raise NotImplementedError(
                f"{what}: the HIP path implements eval-mode semantics (dropout = identity); "
                "call model.eval() / torch.no_grad(), or train through digat_amd.training")

    # ------------------------------------------------------------------ a3 (graphEncoders.py:109-114)
    def compute_news_graph_context(self, news_graph_embeddings, news_graph_mask):
        X = _lib.f32(news_graph_embeddings)
        dev = _lib.require_device(X, news_graph_mask)
        B, N, d = X.shape
        mask = _lib.as_bytes(news_graph_mask)
        out = torch.empty((B, d), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        L = _lib.lib()
        nbytes = L.digat_news_ctx_workspace_bytes(B, N, d)
        ws = _lib.workspace(nbytes, dev, "ctx")
        ca, g = self.candidate_attention, self.news_graph_W
        _lib.check(L.digat_news_ctx_fwd(X.data_ptr(), mask.data_ptr(), ca.K.weight.data_ptr(), ca.Q.weight.data_ptr(),
                                        ca.Q.bias.data_ptr(), g.weight.data_ptr(), g.bias.data_ptr(), None,
                                        out.data_ptr(), B, N, d, ws.data_ptr(), nbytes, _lib.stream_ptr()),
                   "digat_news_ctx_fwd")
        return out

    # ------------------------------------------------------------------ a4 (graphEncoders.py:123-134)
    def compute_user_graph_context(self, user_graph_embeddings, user_category_mask, user_category_indices,
                                   news_graph_context):
        Xu = _lib.f32(user_graph_embeddings)
        c_n = _lib.f32(news_graph_context)
        dev = _lib.require_device(Xu, user_category_mask, user_category_indices, c_n)
        B, U, d = Xu.shape
        H, C1 = self.max_history_num, self.category_num
        mask = _lib.as_bytes(user_category_mask)
        idx = user_category_indices.to(torch.int64).contiguous()
        out = torch.empty((B, d), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        L = _lib.lib()
        nbytes = L.digat_user_ctx_workspace_bytes(B, U, H, C1, d)
        ws = _lib.workspace(nbytes, dev, "ctx")
        ua = self.userAttention
        _lib.check(L.digat_user_ctx_fwd(Xu.data_ptr(), mask.data_ptr(), idx.data_ptr(), c_n.data_ptr(),
                                        self.user_news_K.weight.data_ptr(), self.user_news_Q.weight.data_ptr(),
                                        self.user_news_Q.bias.data_ptr(), self.featureAffine.weight.data_ptr(),
                                        self.featureAffine.bias.data_ptr(), ua.K.weight.data_ptr(),
                                        ua.Q.weight.data_ptr(), ua.Q.bias.data_ptr(), None, out.data_ptr(),
                                        B, U, H, C1, d, ws.data_ptr(), nbytes, _lib.stream_ptr()),
                   "digat_user_ctx_fwd")
        return out

    # ------------------------------------------------------------------ a1 / a2 (graphEncoders.py:143-174)
    def _xattn(self, g: str, index: int, X, A, ctx, return_alpha: bool = False):
        X, ctx = _lib.f32(X), _lib.f32(ctx)
        dev = _lib.require_device(X, A, ctx)
        B, n, d = X.shape
        adj = _lib.as_bytes(A)
        out = torch.empty_like(X)
        alpha = torch.empty((B, n, n), dtype=torch.float32, device=dev) if return_alpha else None
        if B == 0:
            return (out, alpha) if return_alpha else out
        L = _lib.lib()
        nbytes = L.digat_xattn_workspace_bytes(B, n, d)
        ws = _lib.workspace(nbytes, dev, "xattn")
        W = getattr(self, f"{g}_graph_attention_W")[index]
        F3 = getattr(self, f"{g}_graph_attention_ffn3")[index]
        mode = self.resolved_xattn_mode(g)
        if mode == "sparse" and not return_alpha and n > 16 and d <= 1024:      # the caller knows the graphs are sparse
            _lib.check(L.digat_xattn_fwd_mode(X.data_ptr(), adj.data_ptr(), ctx.data_ptr(), W.weight.data_ptr(), W.bias.data_ptr(),
                                              getattr(self, f"{g}_graph_attention_ffn1")[index].weight.data_ptr(),
                                              getattr(self, f"{g}_graph_attention_ffn2")[index].weight.data_ptr(),
                                              F3.weight.data_ptr(), F3.bias.data_ptr(),
                                              getattr(self, f"{g}_graph_attention_a")[index].weight.data_ptr(),
                                              out.data_ptr(), B, n, d, 2, ws.data_ptr(), nbytes, _lib.stream_ptr()),
                       "digat_xattn_fwd_mode")
            return out
        _lib.check(L.digat_xattn_fwd(X.data_ptr(), adj.data_ptr(), ctx.data_ptr(), W.weight.data_ptr(),
                                     W.bias.data_ptr(),
                                     getattr(self, f"{g}_graph_attention_ffn1")[index].weight.data_ptr(),
                                     getattr(self, f"{g}_graph_attention_ffn2")[index].weight.data_ptr(),
                                     F3.weight.data_ptr(), F3.bias.data_ptr(),
                                     getattr(self, f"{g}_graph_attention_a")[index].weight.data_ptr(),
                                     out.data_ptr(), _lib.ptr(alpha), B, n, d, ws.data_ptr(), nbytes,
                                     _lib.stream_ptr()), "digat_xattn_fwd")
        return (out, alpha) if return_alpha else out

    def compute_news_graph_embeddings(self, index, news_graph_embeddings, news_graph, user_graph_context):
        self._eval_only("compute_news_graph_embeddings")
        return self._xattn("news", index, news_graph_embeddings, news_graph, user_graph_context)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph, news_graph_context):
        self._eval_only("compute_user_graph_embeddings")
        return self._xattn("user", index, user_graph_embeddings, user_graph, news_graph_context)

    # ------------------------------------------------------------------ a5 (graphEncoders.py:177-198)
    def _encode(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                user_category_mask, user_category_indices, news_graph_context, shared: bool = False):
        Xn, ue = _lib.f32(news_graph_embeddings), _lib.f32(user_news_embedding)
        dev = _lib.require_device(Xn, news_graph, news_graph_mask, ue, user_graph, user_category_mask,
                                  user_category_indices)
        B, N, d = Xn.shape
        H, C = self.max_history_num, self.category_num - 1
        if ue.shape != (B, H, d) or user_graph.shape[1] != H + C or N != self.news_graph_size:
            raise _lib.DigatHipError("input shapes do not match the encoder's configuration")
        An, Mn = _lib.as_bytes(news_graph), _lib.as_bytes(news_graph_mask)
        Au, cm = _lib.as_bytes(user_graph), _lib.as_bytes(user_category_mask)
        ci = user_category_indices.to(torch.int64).contiguous()
        c0 = None if news_graph_context is None else _lib.f32(news_graph_context)
        out_n = torch.empty((B, d), dtype=torch.float32, device=dev)
        out_u = torch.empty((B, d), dtype=torch.float32, device=dev)
        if B == 0:                       # empty tensors have no storage to point at
            return out_n, out_u
        L = _lib.lib()
        # shared: digat_encoder_fwd_shared — the same arguments, runs of identical consecutive user rows found on the device
        nbytes = (L.digat_encoder_shared_workspace_bytes if shared else L.digat_encoder_workspace_bytes)(B, N, H, C, d, self.graph_depth)
        ws = _lib.workspace(nbytes, dev, "encoder")
        P = self._params()
        _lib.binding().encoder_fwd(_lib.addressof(P), bool(shared), Xn, An, Mn, ue, Au, cm, ci, c0, out_n, out_u, ws)
        return out_n, out_u

    def project_news_layer0(self, news_graph_embeddings):
        """[h|P|Q] of layer 0 of the news graph for M news graphs ([M,N,d] -> [3,M,N,d]): they depend on the news alone, so a
        driver can keep them per news next to the news representations and c_n0 (``util.prepare_news_side``) and hand the
        batch's rows to ``inference_grouped(news_hpq0=...)``.  Same launch, same bits as inside the encoder."""
        X = _lib.f32(news_graph_embeddings)
        dev = _lib.require_device(X)
        M, N, d = X.shape
        out = torch.empty((3, M, N, d), dtype=torch.float32, device=dev)
        if M:
            _lib.check(_lib.lib().digat_news_project0(self._params(), X.data_ptr(), out.data_ptr(), M, N, _lib.stream_ptr()),
                       "digat_news_project0")
        return out

    def project_user_layer0(self, rows):
        """[h|P|Q] of layer 0 of the USER graph for M node embeddings ([M,d] -> [3,M,d]): row-wise, so they can be kept per
        news (history nodes) and per topic (``self.topic_node_embedding``) — see ``util.prepare_news_side``."""
        X = _lib.f32(rows)
        dev = _lib.require_device(X)
        M, d = X.shape
        out = torch.empty((3, M, d), dtype=torch.float32, device=dev)
        if M:
            _lib.check(_lib.lib().digat_user_project0(self._params(), X.data_ptr(), out.data_ptr(), M, _lib.stream_ptr()),
                       "digat_user_project0")
        return out

    def news_context_queries(self, news_graph_context):
        """[topic query | user-attention query | K3 of the user graph's layer 0] of M news contexts ([M,d] -> [3,M,d]): linear maps
        of the candidate's cached c_n0, so a driver keeps them per news next to c_n0 (``util.prepare_news_side``) and hands the
        batch's rows to ``inference_grouped(ctxq0=...)``.  Same launch, same bits as inside the encoder (eval mode)."""
        c = _lib.f32(news_graph_context)
        dev = _lib.require_device(c)
        M, d = c.shape
        out = torch.empty((3, M, d), dtype=torch.float32, device=dev)
        if self.graph_depth == 0:
            out[2].zero_()
        if M:
            _lib.check(_lib.lib().digat_news_context_queries(self._params(), c.data_ptr(), out.data_ptr(), M, _lib.stream_ptr()),
                       "digat_news_context_queries")
        return out

    def inference_grouped(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                          user_category_mask, user_category_indices, row_group, news_graph_context, news_hpq0=None,
                          hist_hpq0=None, topic_hpq0=None, ctxq0=None, news_index=None):
        """``inference`` for rows that share users (not in the reference: its driver expands the user tensors per
        row, util.py:57-67).  The four user tensors are given once per GROUP ([G,...]) and ``row_group`` [B] maps
        each row to its group; results are bit-identical to ``inference`` on the expanded tensors.
        ``news_index`` [B] int64: ``news_graph_embeddings`` and ``news_hpq0`` are then the per-news TABLES ([news_num, N, d],
        [3, news_num, N, d]) and row b reads their row ``news_index[b]`` in place (no gathered copies)."""
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        Xn, ue = _lib.f32(news_graph_embeddings), _lib.f32(user_news_embedding)
        dev = _lib.require_device(Xn, news_graph, news_graph_mask, ue, user_graph, user_category_mask,
                                  user_category_indices, row_group)
        _, N, d = Xn.shape
        B = news_graph.shape[0]
        if news_index is None and Xn.shape[0] != B:
            raise ValueError("news_graph_embeddings must have one graph per row (or pass news_index with the per-news tables)")
        G = ue.shape[0]
        H, C = self.max_history_num, self.category_num - 1
        if B == 0 or 4 * G > B or self.training:       # empty batch, or too few rows per group to pay off: expand, plain path
            rg = row_group.long()
            if news_index is not None:
                Xn = Xn.index_select(0, news_index.long())
            return self._encode(Xn, news_graph, news_graph_mask, ue.index_select(0, rg), user_graph.index_select(0, rg),
                                user_category_mask.index_select(0, rg), user_category_indices.index_select(0, rg),
                                news_graph_context)
        An, Mn = _lib.as_bytes(news_graph), _lib.as_bytes(news_graph_mask)
        Au, cm = _lib.as_bytes(user_graph), _lib.as_bytes(user_category_mask)
        ci = user_category_indices.to(torch.int64).contiguous()
        rg = row_group.to(torch.int32).contiguous()
        c0 = _lib.f32(news_graph_context)
        out_n = torch.empty((B, d), dtype=torch.float32, device=dev)
        out_u = torch.empty((B, d), dtype=torch.float32, device=dev)
        L = _lib.lib()
        nbytes = L.digat_encoder_grouped_workspace_bytes(B, N, H, C, d, self.graph_depth)
        ws = _lib.workspace(nbytes, dev, "encoder")
        hpq = hh = th = cq = ni = None
        if news_index is not None:
            if news_hpq0 is None or news_graph_context is None:
                raise ValueError("news_index needs news_hpq0 (the per-news table) and news_graph_context")
            ni = news_index.to(torch.int64).contiguous()
            M = Xn.shape[0]
            if ni.shape[0] != B or tuple(news_hpq0.shape) != (3, M, N, d):
                raise ValueError("with news_index: news_graph_embeddings [M, N, d], news_hpq0 [3, M, N, d], news_index [B]")
        if ctxq0 is not None:
            cq = _lib.f32(ctxq0)
            if tuple(cq.shape) != (3, B, d):
                raise ValueError("ctxq0 must be [3, B, d] (news_context_queries of the batch's news contexts)")
        if news_hpq0 is not None:
            hpq = _lib.f32(news_hpq0)
            if ni is None and tuple(hpq.shape) != (3, B, N, d):
                raise ValueError("news_hpq0 must be [3, B, N, d] (project_news_layer0 of the batch's candidates)")
        if hist_hpq0 is not None:
            hh, th = _lib.f32(hist_hpq0), _lib.f32(topic_hpq0)
            if tuple(hh.shape) != (3, G, H, d) or tuple(th.shape) != (3, C, d):
                raise ValueError("hist_hpq0 must be [3, G, H, d] and topic_hpq0 [3, C, d] (project_user_layer0)")
        # the per-news tables are optional, any subset: the binding takes the plain grouped entry when none is given
        P = self._params()
        _lib.binding().encoder_fwd_grouped(_lib.addressof(P), Xn, An, Mn, ue, Au, cm, ci, rg, c0, hpq, hh, th, cq, ni, out_n, out_u, ws)
        return out_n, out_u

    def forward(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                user_category_mask, user_category_indices):
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        if self.training and torch.is_grad_enabled():
            from .training import digat_forward_train
            return digat_forward_train(self, news_graph_embeddings, news_graph, news_graph_mask,
                                       user_news_embedding, user_graph, user_category_mask, user_category_indices)
        return self._encode(news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                            user_category_mask, user_category_indices, None)

    def inference(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                  user_category_mask, user_category_indices, news_graph_context):
        """graphEncoders.py:189-198.  The reference's driver expands an impression's user tensors once per candidate
        (util.py:57-67), so consecutive rows of a dev batch carry bit-identical users: with ``detect_shared_users`` (default) the
        call goes to ``digat_encoder_fwd_shared`` — the runs are found on the device (every byte of the four user tensors compared
        with the previous row's), nothing is read back by the host, and layer 0 of the user graph is computed once per run.
        Bit-identical to the per-row entry; rows that share nothing cost the comparison pass on top of it."""
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        want = bool(self._launch_option("detect_shared_users") and not self.training and self.graph_depth > 0
                    and news_graph_embeddings.shape[0] >= self.SHARED_USERS_MIN_ROWS)
        if (want and self.user_xattn_mode == "auto" and "user" not in self.corpus_xattn_hint and user_graph.is_cuda
                and not torch.cuda.is_current_stream_capturing()):
            # a driver that never showed the corpus to util.prepare_news_side (the reference's own loop): the sparse / dense choice
            # of the user graph's Eq. 8 is made here, ONCE, from the first batch (one host read; the library's per-batch device-side
            # choice launches both variants, and only the sparse one can share layer 0 between the rows of a run)
            from .util import SPARSE_ENTRIES_PER_NODE
            per_node = float(user_graph.sum(dtype=torch.float64) / max(1, user_graph.shape[0] * user_graph.shape[1]))
            self.corpus_xattn_hint = dict(self.corpus_xattn_hint, user="sparse" if per_node <= SPARSE_ENTRIES_PER_NODE else "dense")
        shared = want and self.resolved_xattn_mode("user") == "sparse"
        return self._encode(news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                            user_category_mask, user_category_indices, news_graph_context, shared=shared)

    detect_shared_users = True         # inference(): look for runs of identical consecutive user rows (see there)
    SHARED_USERS_MIN_ROWS = 128        # ... in batches of at least this many rows

    def _shared_user_runs(self, Xn, ue, Au, cm, ci):
        """(row_group [B] int32, leaders [G] int64) when the rows of this batch are runs of identical users worth grouping, else None:
        the search of ``digat_encoder_fwd_shared`` as a stand-alone call (``digat_user_row_runs``; one host read of the run count) for
        drivers that want to call ``inference_grouped`` themselves, and for the tests."""
        B = ue.shape[0]
        if (not self._launch_option("detect_shared_users") or self.training or B < self.SHARED_USERS_MIN_ROWS or self.graph_depth == 0
                or self.resolved_xattn_mode("user") == "dense" or ue.dtype != torch.float32 or not ue.is_cuda
                or torch.cuda.is_current_stream_capturing()):          # the run count is read on the host: not inside a graph capture
            return None
        H, d = self.max_history_num, self.news_embedding_dim
        U, C1 = self.user_graph_size, self.category_num
        if tuple(ue.shape) != (B, H, d) or tuple(Au.shape) != (B, U, U) or tuple(cm.shape) != (B, C1) or tuple(ci.shape) != (B, H):
            return None
        dev = _lib.require_device(ue, Au, cm, ci)
        ue_c, Au_b, cm_b = _lib.f32(ue), _lib.as_bytes(Au), _lib.as_bytes(cm)
        ci_c = ci.to(torch.int64).contiguous()
        row_group = torch.empty(B, dtype=torch.int32, device=dev)
        leaders = torch.empty(B, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _lib.workspace(B, dev, "runs")
        _lib.binding().user_row_runs(ue_c, Au_b, cm_b, ci_c, row_group, leaders, count, ws)
        G = int(count.item())              # the one host read of the drop-in path
        if 4 * G > B:
            return None
        return row_group, leaders[:G]


# ======================================================================================================
# the five ablation encoders of the reference (graphEncoders.py:201-842), on the same kernels
# ======================================================================================================
class _Ablation(GraphEncoder):
    """Shared machinery.  A subclass names which graph runs Eq. 8 (``EQ8``), which runs the vanilla-GAT layer (``GAT``)
    and whether the news context exists (``NEWS_CONTEXT``); parameter names are the reference's, so its checkpoints
    load.  Inference / eval-mode forward run on the HIP kernels (``digat_xattn_fwd``, ``digat_gat_fwd``,
    ``digat_news_ctx_fwd``, ``digat_user_ctx_fwd``); training-mode forward (with autograd) goes through
    ``training.ablation_forward_train`` on the ``digat_*_fwd_train`` / ``digat_*_bwd`` pairs.  ``inference_grouped`` is the
    scoring pass's entry (util.score_rows): user tensors once per impression, the candidate-independent halves computed once."""
    EQ8: tuple = ()
    GAT: tuple = ()
    NEWS_CONTEXT = True

    def __init__(self, config, news_embedding_dim: int):
        super().__init__(config, news_embedding_dim)
        d, L = self.news_embedding_dim, self.graph_depth
        if d % 4 != 0:
            raise ValueError("digat_amd needs news_embedding_dim % 4 == 0 (float4 rows)")
        if self.NEWS_CONTEXT:
            self.candidate_attention = ScaledDotProductAttention(d, d, d)
            self.news_graph_W = nn.Linear(d * 2, d, bias=True)
        self.user_news_K = nn.Linear(d, d, bias=False)
        self.user_news_Q = nn.Linear(d, d, bias=True)
        self.featureAffine = nn.Linear(d, d, bias=True)
        self.userAttention = ScaledDotProductAttention(d, d, d)
        for g in self.EQ8:
            setattr(self, f"{g}_graph_attention_W", nn.ModuleList([nn.Linear(d, d, bias=True) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn1", nn.ModuleList([nn.Linear(d, d, bias=False) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn2", nn.ModuleList([nn.Linear(d, d, bias=False) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_ffn3", nn.ModuleList([nn.Linear(d, d, bias=True) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_a", nn.ModuleList([nn.Linear(d, 1, bias=False) for _ in range(L)]))
        for g in self.GAT:
            setattr(self, f"{g}_graph_attention_W", nn.ModuleList([nn.Linear(d, d, bias=True) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_a1", nn.ModuleList([nn.Linear(d, 1, bias=False) for _ in range(L)]))
            setattr(self, f"{g}_graph_attention_a2", nn.ModuleList([nn.Linear(d, 1, bias=False) for _ in range(L)]))

    def initialize(self):
        super().initialize()
        relu_gain = nn.init.calculate_gain('relu')
        leaky_gain = nn.init.calculate_gain('leaky_relu', 0.2)
        for g in self.EQ8 + self.GAT:
            for i in range(self.graph_depth):
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_W")[i].weight)
                nn.init.zeros_(getattr(self, f"{g}_graph_attention_W")[i].bias)
        for g in self.EQ8:
            for i in range(self.graph_depth):
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_a")[i].weight, gain=leaky_gain)
                for f in ("ffn1", "ffn2", "ffn3"):
                    nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_{f}")[i].weight, gain=relu_gain)
                nn.init.zeros_(getattr(self, f"{g}_graph_attention_ffn3")[i].bias)
        for g in self.GAT:
            for i in range(self.graph_depth):
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_a1")[i].weight, gain=leaky_gain)
                nn.init.xavier_uniform_(getattr(self, f"{g}_graph_attention_a2")[i].weight, gain=leaky_gain)
        if self.NEWS_CONTEXT:
            self.candidate_attention.initialize()
            nn.init.xavier_uniform_(self.news_graph_W.weight)
            nn.init.zeros_(self.news_graph_W.bias)
        nn.init.xavier_uniform_(self.user_news_K.weight)
        nn.init.xavier_uniform_(self.user_news_Q.weight)
        nn.init.zeros_(self.user_news_Q.bias)
        nn.init.xavier_uniform_(self.featureAffine.weight, gain=relu_gain)
        nn.init.zeros_(self.featureAffine.bias)
        self.userAttention.initialize()

    # the context functions and the Eq. 8 layer are DIGAT's (same attribute names)
    _eval_only = DIGAT._eval_only
    compute_news_graph_context = DIGAT.compute_news_graph_context
    compute_user_graph_context = DIGAT.compute_user_graph_context
    _xattn = DIGAT._xattn
    resolved_xattn_mode = DIGAT.resolved_xattn_mode
    user_xattn_mode = "auto"      # Eq. 8 variant per graph for digat_xattn_fwd_mode ("auto" = dense until
    news_xattn_mode = "auto"      # util.prepare_news_side has looked at the corpus)
    corpus_xattn_hint: dict = {}  # replaced per instance by util.prepare_news_side

    def _gat(self, g: str, index: int, X, A):
        """Vanilla GAT update layer (graphEncoders.py:493-519)."""
        self._eval_only("vanilla GAT layer")
        X = _lib.f32(X)
        dev = _lib.require_device(X, A)
        B, n, d = X.shape
        out = torch.empty_like(X)
        if B == 0:
            return out
        adj = _lib.as_bytes(A)
        L = _lib.lib()
        nbytes = L.digat_gat_workspace_bytes(B, n, d)
        ws = _lib.workspace(nbytes, dev, "gat")
        W = getattr(self, f"{g}_graph_attention_W")[index]
        _lib.check(L.digat_gat_fwd(X.data_ptr(), adj.data_ptr(), W.weight.data_ptr(), W.bias.data_ptr(),
                                   getattr(self, f"{g}_graph_attention_a1")[index].weight.data_ptr(),
                                   getattr(self, f"{g}_graph_attention_a2")[index].weight.data_ptr(), out.data_ptr(), B, n, d,
                                   ws.data_ptr(), nbytes, _lib.stream_ptr()), "digat_gat_fwd")
        return out

    def _user_nodes(self, user_news_embedding):
        ue = _lib.f32(user_news_embedding)
        return torch.cat([ue, self.topic_node_embedding.unsqueeze(0).expand(ue.shape[0], -1, -1)], dim=1).contiguous()

    def _layer(self, g: str, i: int, X, A, ctx):
        if g in self.EQ8:
            self._eval_only("Eq. 8 layer")
            return self._xattn(g, i, X, A, ctx)
        return self._gat(g, i, X, A)

    def _encode(self, Xn, An, Mn, ue, Au, cm, ci, c_n):
        Xu = self._user_nodes(ue)
        c_u = self.compute_user_graph_context(Xu, cm, ci, c_n)
        for i in range(self.graph_depth):
            # both updates read the PREVIOUS contexts; tuple assignment keeps the reference's order of evaluation
            Xn, Xu = self._layer("news", i, Xn, An, c_u), self._layer("user", i, Xu, Au, c_n)
            c_n = c_n + self.compute_news_graph_context(Xn, Mn)
            c_u = c_u + self.compute_user_graph_context(Xu, cm, ci, c_n)
        return c_n, c_u

    def forward(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                user_category_mask, user_category_indices):
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        if self.training and torch.is_grad_enabled():
            from .training import ablation_forward_train
            return ablation_forward_train(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding,
                                          user_graph, user_category_mask, user_category_indices)
        c_n = self.compute_news_graph_context(news_graph_embeddings, news_graph_mask)
        return self._encode(_lib.f32(news_graph_embeddings), news_graph, news_graph_mask, user_news_embedding, user_graph,
                            user_category_mask, user_category_indices, c_n)

    def inference(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                  user_category_mask, user_category_indices, news_graph_context):
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        return self._encode(_lib.f32(news_graph_embeddings), news_graph, news_graph_mask, user_news_embedding, user_graph,
                            user_category_mask, user_category_indices, _lib.f32(news_graph_context))

    # ------------------------------------------------------------------ the scoring pass: what an impression's rows share
    # What util.GroupedBatchPipeline gathers per ROW for this class: "news_graphs" (neighbourhood embeddings, adjacency, mask),
    # "c_n0", "ctx_layers" (the candidates' rows of DeviceCorpus.news_ctx_layers).  The user side is always gathered per group.
    PIPELINE_READS: tuple = ("news_graphs", "c_n0")

    def _user_nodes_dev(self, user_news_embedding, row_group=None):
        """Xu^(0) in one launch (``digat_user_nodes_build``): [G,U,d] from ``user_news_embedding`` [G,H,d] and the topic
        embeddings, or — ``row_group`` [B] int32 — the expanded [B,U,d] written directly (no ``cat``, no ``index_select``)."""
        ue = _lib.f32(user_news_embedding)
        topic = _lib.f32(self.topic_node_embedding.detach())
        dev = _lib.require_device(ue, topic) if row_group is None else _lib.require_device(ue, topic, row_group)
        if ue.data_ptr() % 16:
            ue = ue.clone()
        G, H, d = ue.shape
        C = self.category_num - 1
        rows = G if row_group is None else int(row_group.shape[0])
        out = torch.empty((rows, H + C, d), dtype=torch.float32, device=dev)
        if rows:
            _lib.check(_lib.lib().digat_user_nodes_build(ue.data_ptr(), topic.data_ptr(), _lib.ptr(row_group), out.data_ptr(), rows, G,
                                                         H, C, d, _lib.stream_ptr()), "digat_user_nodes_build")
        return out

    def _user_ctx(self, Xu, user_category_mask, user_category_indices, c_n, acc=None, row_group=None):
        """``compute_user_graph_context`` added to ``acc`` in place (``addend == out``; ``acc=None``: a new tensor).  With ``row_group``
        [B] int32 the three user tensors are per GROUP and row b reads the nodes of group ``row_group[b]`` in place
        (``digat_user_ctx_fwd_grouped``: the bits of the per-row entry on the expanded tensors)."""
        Xu, c_n = _lib.f32(Xu), _lib.f32(c_n)
        dev = _lib.require_device(Xu, user_category_mask, user_category_indices, c_n)
        B, d = c_n.shape
        U, H, C1 = Xu.shape[1], self.max_history_num, self.category_num
        mask = _lib.as_bytes(user_category_mask)
        idx = user_category_indices.to(torch.int64).contiguous()
        out = acc if acc is not None else torch.empty((B, d), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        L = _lib.lib()
        ua = self.userAttention
        weights = (self.user_news_K.weight.data_ptr(), self.user_news_Q.weight.data_ptr(), self.user_news_Q.bias.data_ptr(),
                   self.featureAffine.weight.data_ptr(), self.featureAffine.bias.data_ptr(), ua.K.weight.data_ptr(),
                   ua.Q.weight.data_ptr(), ua.Q.bias.data_ptr())
        if row_group is None:
            nbytes = L.digat_user_ctx_workspace_bytes(B, U, H, C1, d)
            ws = _lib.workspace(nbytes, dev, "ctx")
            _lib.check(L.digat_user_ctx_fwd(Xu.data_ptr(), mask.data_ptr(), idx.data_ptr(), c_n.data_ptr(), *weights, _lib.ptr(acc),
                                            out.data_ptr(), B, U, H, C1, d, ws.data_ptr(), nbytes, _lib.stream_ptr()),
                       "digat_user_ctx_fwd")
            return out
        G = Xu.shape[0]
        nbytes = L.digat_user_ctx_grouped_workspace_bytes(B, G, U, H, C1, d)
        ws = _lib.workspace(nbytes, dev, "ctx")
        _lib.check(L.digat_user_ctx_fwd_grouped(Xu.data_ptr(), mask.data_ptr(), idx.data_ptr(), row_group.data_ptr(), c_n.data_ptr(),
                                                *weights, _lib.ptr(acc), out.data_ptr(), B, G, U, H, C1, d, ws.data_ptr(), nbytes,
                                                _lib.stream_ptr()), "digat_user_ctx_fwd_grouped")
        return out

    @staticmethod
    def _expand_rows(table, rows64):
        """``table.index_select(0, rows64)`` of a bool / byte table through ``digat_gather_tables`` (the groups' adjacency, per row)."""
        t = _lib.as_bytes(table)
        out = torch.empty((rows64.shape[0],) + tuple(t.shape[1:]), dtype=torch.uint8, device=t.device)
        if out.numel():
            job = (_lib.GatherJob * 1)(_lib.GatherJob(t.data_ptr(), out.data_ptr(), t[0].numel(), rows64.shape[0], rows64.data_ptr(), None, 1))
            _lib.check(_lib.lib().digat_gather_tables(job, 1, _lib.stream_ptr()), "digat_gather_tables")
        return out

    def news_context_layers(self, news_graph_embeddings, news_graph, news_graph_mask, news_graph_context=None):
        """c_n^(0..L) of M news as one [L+1, M, d] tensor, for the classes whose news graph runs the vanilla GAT layer: the chain
        depends on the news alone (``util.prepare_news_side`` keeps it per news).  Prefix sums in ``inference``'s order."""
        if "news" not in self.GAT:
            raise _lib.DigatHipError(type(self).__name__ + ": the news context depends on the user side")
        X = _lib.f32(news_graph_embeddings)
        c = (self.compute_news_graph_context(X, news_graph_mask) if news_graph_context is None else _lib.f32(news_graph_context))
        out = torch.empty((self.graph_depth + 1,) + tuple(c.shape), dtype=torch.float32, device=c.device)
        out[0] = c
        for i in range(self.graph_depth):
            X = self._gat("news", i, X, news_graph)
            c = c + self.compute_news_graph_context(X, news_graph_mask)
            out[i + 1] = c
        return out

    def news_side_tables(self, SA_news_representations, news_graph, news_graph_mask, batch_size: int):
        """``(c_n0 [news_num, d], news_ctx_layers [K, news_num, d] or None)`` for ``util.prepare_news_side``: whatever of this
        class's news side is a function of the news id alone, computed in chunks."""
        SA = SA_news_representations
        news_num, _, d = SA.shape
        c_n0 = torch.empty((news_num, d), dtype=torch.float32, device=SA.device)
        layers = None
        if "news" in self.GAT:
            layers = torch.empty((self.graph_depth + 1, news_num, d), dtype=torch.float32, device=SA.device)
        chunk = max(1, int(batch_size))
        for s in range(0, news_num, chunk):
            e = min(s + chunk, news_num)
            c_n0[s:e] = self.compute_news_graph_context(SA[s:e], news_graph_mask[s:e])
        if layers is not None:
            chunk = max(chunk, 4096)
            for s in range(0, news_num, chunk):
                e = min(s + chunk, news_num)
                layers[:, s:e] = self.news_context_layers(SA[s:e], news_graph[s:e], news_graph_mask[s:e], c_n0[s:e])
        return c_n0, layers

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        """The class's pass over B rows of G groups (``inference_grouped``): ``ue`` [G,H,d] and ``Xu0`` [G,U,d] built from it, the
        user tensors per group, ``rg`` / ``rg64`` the row -> group map as int32 / int64."""
        raise NotImplementedError

    def inference_grouped(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                          user_category_mask, user_category_indices, row_group, news_graph_context, *, news_ctx_layers=None,
                          news_index=None):
        """``inference`` for rows that share users: the four user tensors once per GROUP ([G,...]), ``row_group`` [B] mapping each
        row to its group (any mapping).  What does not depend on the candidate is computed once per group — the vanilla GAT layers
        of the user graph, Xu^(0) — and the user contexts on such features read them in place (``digat_user_ctx_fwd_grouped``).
        ``news_ctx_layers`` [K, B, d]: the rows' c_n^(0..L) (``news_context_layers``; wo_SA: K = 1, the candidate's own
        representation) — the news-side tensors may then be None for the classes that read nothing else of them.
        ``news_index`` [B] int64: ``news_graph_embeddings`` / ``news_ctx_layers`` are the per-news tables and row b is their row
        ``news_index[b]``.  Too few rows per group (4 G > B), an empty batch or training mode: expands and calls ``inference``."""
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        ue = _lib.f32(user_news_embedding)
        dev = _lib.require_device(ue, user_graph, user_category_mask, user_category_indices, row_group)
        B, G = int(row_group.shape[0]), int(ue.shape[0])
        Xn, layers = news_graph_embeddings, news_ctx_layers
        if news_index is not None:
            ni = news_index.long()
            Xn = None if Xn is None else Xn.index_select(0, ni)
            layers = None if layers is None else layers.index_select(1, ni)
        if B == 0 or 4 * G > B or self.training:
            if Xn is None or news_graph is None or news_graph_mask is None or news_graph_context is None:
                raise ValueError("inference_grouped: the per-row path needs the news-side tensors")
            rg = row_group.long()
            return self.inference(Xn, news_graph, news_graph_mask, ue.index_select(0, rg), user_graph.index_select(0, rg),
                                  user_category_mask.index_select(0, rg), user_category_indices.index_select(0, rg),
                                  news_graph_context)
        rg64 = row_group.to(torch.int64).clamp(0, G - 1)          # the gathers below index with it: no read leaves the groups' buffers
        rg = rg64.to(torch.int32)
        if layers is not None:
            layers = _lib.f32(layers)
            if layers.dim() != 3 or layers.shape[1] != B:
                raise ValueError("news_ctx_layers must be [K, B, d] (or the [K, news_num, d] table with news_index)")
        c_n = None if news_graph_context is None else _lib.f32(news_graph_context)
        reads = self.PIPELINE_READS
        if ("news_graphs" in reads or ("ctx_layers" in reads and layers is None)) and (
                Xn is None or news_graph is None or news_graph_mask is None):
            raise ValueError(type(self).__name__ + ".inference_grouped: the news-graph tensors may only be None with news_ctx_layers")
        if "c_n0" in reads and c_n is None:
            raise ValueError(type(self).__name__ + ".inference_grouped needs news_graph_context")
        return self._grouped(None if Xn is None else _lib.f32(Xn), news_graph, news_graph_mask, ue, self._user_nodes_dev(ue), user_graph,
                             user_category_mask, user_category_indices, rg, rg64, c_n, layers)

    def _eq8_user_rows(self, ue, rg, Au, cm, ci, rg64):
        """The per-row inputs of the user graph's Eq. 8 layers: expanded Xu^(0) (written directly), adjacency, mask, indices."""
        return (self._user_nodes_dev(ue, rg), self._expand_rows(Au, rg64), _lib.as_bytes(cm).index_select(0, rg64),
                ci.index_select(0, rg64))

    def _gat_user_layers(self, Xu0, Au):
        """Xu^(0..L) of the G groups: the vanilla GAT layers of the user graph see nothing of the candidate."""
        Xs = [Xu0]
        for i in range(self.graph_depth):
            Xs.append(self._gat("user", i, Xs[-1], Au))
        return Xs


class wo_SA(_Ablation):
    """graphEncoders.py:201-293 — no semantic-augmentation graph: the candidate's own representation is the context."""
    EQ8, GAT, NEWS_CONTEXT = ("user",), (), False
    PIPELINE_READS = ("ctx_layers",)

    def news_side_tables(self, SA_news_representations, news_graph, news_graph_mask, batch_size: int):
        """No news context exists: c_n0 is a zero table that is never read, and the one "layer" is the candidate's own
        representation (node 0 of its neighbourhood), so that a pass gathers d floats per row instead of N d."""
        SA = SA_news_representations
        return torch.zeros((SA.shape[0], SA.shape[2]), dtype=torch.float32, device=SA.device), SA[:, 0].contiguous().unsqueeze(0)

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        c = layers[0] if layers is not None else Xn[:, 0].contiguous()
        if self.graph_depth == 0:
            return c, self._user_ctx(Xu0, cm, ci, c, row_group=rg)
        Xu, Au_r, cm_r, ci_r = self._eq8_user_rows(ue, rg, Au, cm, ci, rg64)
        for i in range(self.graph_depth):
            Xu = self._layer("user", i, Xu, Au_r, c)
        return c, self._user_ctx(Xu, cm_r, ci_r, c)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph, news_graph_context):
        return self._layer("user", index, user_graph_embeddings, user_graph, news_graph_context)

    def _run(self, news_graph_embeddings, user_news_embedding, user_graph, user_category_mask, user_category_indices):
        c = _lib.f32(news_graph_embeddings)[:, 0].contiguous()
        Xu = self._user_nodes(user_news_embedding)
        for i in range(self.graph_depth):
            Xu = self._layer("user", i, Xu, user_graph, c)
        return c, self.compute_user_graph_context(Xu, user_category_mask, user_category_indices, c)

    def forward(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                user_category_mask, user_category_indices):
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        if self.training and torch.is_grad_enabled():
            from .training import ablation_forward_train
            return ablation_forward_train(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding,
                                          user_graph, user_category_mask, user_category_indices)
        return self._run(news_graph_embeddings, user_news_embedding, user_graph, user_category_mask, user_category_indices)

    def inference(self, news_graph_embeddings, news_graph, news_graph_mask, user_news_embedding, user_graph,
                  user_category_mask, user_category_indices, news_graph_context):
        user_graph, user_category_mask = derive_user_graph(user_graph, user_category_mask, user_category_indices, self.category_num - 1)
        return self._run(news_graph_embeddings, user_news_embedding, user_graph, user_category_mask, user_category_indices)


class Seq_SA(_Ablation):
    """graphEncoders.py:295-408 — the neighbourhood as a sequence: pooled once into the news context, never updated."""
    EQ8, GAT = ("user",), ()
    PIPELINE_READS = ("c_n0",)

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        c_u = self._user_ctx(Xu0, cm, ci, c_n, row_group=rg)
        if self.graph_depth:
            Xu, Au_r, cm_r, ci_r = self._eq8_user_rows(ue, rg, Au, cm, ci, rg64)
            for i in range(self.graph_depth):
                Xu = self._layer("user", i, Xu, Au_r, c_n)
                self._user_ctx(Xu, cm_r, ci_r, c_n, acc=c_u)
        return c_n, c_u

    def compute_news_sequence_context(self, news_graph_embeddings, news_graph_mask):
        return self.compute_news_graph_context(news_graph_embeddings, news_graph_mask)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph, news_graph_context):
        return self._layer("user", index, user_graph_embeddings, user_graph, news_graph_context)

    def _encode(self, Xn, An, Mn, ue, Au, cm, ci, c_n):
        Xu = self._user_nodes(ue)
        c_u = self.compute_user_graph_context(Xu, cm, ci, c_n)
        for i in range(self.graph_depth):
            Xu = self._layer("user", i, Xu, Au, c_n)
            c_u = c_u + self.compute_user_graph_context(Xu, cm, ci, c_n)
        return c_n, c_u


class wo_interaction(_Ablation):
    """graphEncoders.py:410-549 — vanilla GAT layers on both graphs."""
    EQ8, GAT = (), ("news", "user")
    PIPELINE_READS = ("ctx_layers",)

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        if layers is None:
            layers = self.news_context_layers(Xn, An, Mn, c_n)
        c_u = None
        for i, Xu in enumerate(self._gat_user_layers(Xu0, Au)):          # c_u = sum_i ctx(Xu^(i)[g], c_n^(i)[cand]), left to right
            c_u = self._user_ctx(Xu, cm, ci, layers[i], acc=c_u, row_group=rg)
        return layers[self.graph_depth], c_u

    def compute_news_graph_embeddings(self, index, news_graph_embeddings, news_graph):
        return self._gat("news", index, news_graph_embeddings, news_graph)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph):
        return self._gat("user", index, user_graph_embeddings, user_graph)


class News_graph_wo_inter(_Ablation):
    """graphEncoders.py:551-696 — vanilla GAT on the news graph, Eq. 8 on the user graph."""
    EQ8, GAT = ("user",), ("news",)
    PIPELINE_READS = ("ctx_layers",)

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        if layers is None:
            layers = self.news_context_layers(Xn, An, Mn, c_n)
        c_u = self._user_ctx(Xu0, cm, ci, layers[0], row_group=rg)
        if self.graph_depth:
            Xu, Au_r, cm_r, ci_r = self._eq8_user_rows(ue, rg, Au, cm, ci, rg64)
            for i in range(self.graph_depth):
                Xu = self._layer("user", i, Xu, Au_r, layers[i])
                self._user_ctx(Xu, cm_r, ci_r, layers[i + 1], acc=c_u)
        return layers[self.graph_depth], c_u

    def compute_news_graph_embeddings(self, index, news_graph_embeddings, news_graph):
        return self._gat("news", index, news_graph_embeddings, news_graph)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph, news_graph_context):
        return self._layer("user", index, user_graph_embeddings, user_graph, news_graph_context)


class User_graph_wo_inter(_Ablation):
    """graphEncoders.py:698-842 — Eq. 8 on the news graph, vanilla GAT on the user graph."""
    EQ8, GAT = ("news",), ("user",)
    PIPELINE_READS = ("news_graphs", "c_n0")

    def _grouped(self, Xn, An, Mn, ue, Xu0, Au, cm, ci, rg, rg64, c_n, layers):
        Xs = self._gat_user_layers(Xu0, Au)
        c_u = self._user_ctx(Xs[0], cm, ci, c_n, row_group=rg)
        for i in range(self.graph_depth):
            Xn = self._layer("news", i, Xn, An, c_u)
            c_n = c_n + self.compute_news_graph_context(Xn, Mn)
            self._user_ctx(Xs[i + 1], cm, ci, c_n, acc=c_u, row_group=rg)
        return c_n, c_u

    def compute_news_graph_embeddings(self, index, news_graph_embeddings, news_graph, user_graph_context):
        return self._layer("news", index, news_graph_embeddings, news_graph, user_graph_context)

    def compute_user_graph_embeddings(self, index, user_graph_embeddings, user_graph):
        return self._gat("user", index, user_graph_embeddings, user_graph)
