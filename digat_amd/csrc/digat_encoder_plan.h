// digat_encoder_plan.h — every decision of one encoder call: which path it takes, which kernels are eligible, what a refused call
// returns.  Plain C++, no HIP types: digat_encoder.inc issues what encoder_plan decides, and tests/test_encoder_plan_cpu.py builds
// this header with the host compiler to pin the whole plan per input.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/digat_hip.h"
#include "digat_xattn_plan.h"      // the Eq. 8 kernel eligibilities (eq8_*): the plan and the launch routes ask the same questions

enum { ENC_PLAIN, ENC_GROUPED, ENC_SHARED };      // the public entry: per-row users, users per group, per-row users with runs found

// ---- the operand formats of a weight version ------------------------------------------------------------------------------------
// fmt: the format every wsplit image of the parameters was split in; lfmt: the layers' [W|ffn1|ffn2] images (fp16-fp8c under
// DIGAT_PARAMS_PROJ_F16F8C); range_flag: fp16x3's overflow flag, not raised by bf16x6
struct GemmFormats { int fmt, lfmt; unsigned* range_flag; };
static inline GemmFormats gemm_formats(int flags, void* range_flag) {
    const int fmt = (flags & DIGAT_PARAMS_GEMM_F16X3) ? 1 : 0;
    return GemmFormats{fmt, (flags & DIGAT_PARAMS_PROJ_F16F8C) ? DIGAT_GEMM_F16F8C : fmt, fmt ? (unsigned*)range_flag : nullptr};
}
static inline GemmFormats gemm_formats(const digat_params* p) { return gemm_formats(p->flags, p->range_flag); }
// the kernel of the [B,d] linears is named by the caller, not chosen from B: a row's bits must not depend on the batch it sits in
// (nor on whether its context queries come from the per-news table)
static inline int bd_dispatch(int flags) { return (flags & DIGAT_PARAMS_BD_TILED) ? (1 << 30) : 1; }

// What the decisions depend on: the call's sizes and flags, and which optional inputs the caller passed.
struct EncoderPlanIn {
    int flags, B, N, H, C, d, L, G, variant;
    bool folded;                     // the weight version carries the folded attention queries
    bool c_n0, news_hpq0, hist_hpq0, topic_hpq0, ctxq0, news_index; int64_t news_rows;
    bool fsplit;                     // featureAffine_fsplit: the fused user context's weight image
    bool ctx_fused_fits;             // ... and whether (H, C + 1, d) fit that kernel (ctxfused_ok: the kernel's own limits)
};

struct EncoderPlan {
    int status;                      // != DIGAT_OK: the entry returns this before it looks at the workspace
    int status_after_carve;          // ... and this after the carve (DIGAT_ERR_WORKSPACE) and the B == 0 return: news_index not admissible
    bool folded;
    bool shared;                     // ENC_SHARED with the runs honoured (else the plain per-row path)
    bool by_group;                   // the user side of layer 0 is read through row_group (grouped rows, or shared runs)
    bool xu0_grouped;                // layer-0 user nodes exist once per group
    bool xu0_shared;                 // only the run-leading rows of Xu[0] were built
    bool c_n0_in_place;              // layer 0's news context update reads the caller's c_n0 directly
    bool ctxq0;                      // the caller's context queries are honoured (they belong to a given news context)
    int sparse_mode;                 // Eq. 8 of the user graph: DIGAT_XATTN_SPARSE, _DENSE, or _AUTO (both, the device choosing)
    bool want_live, want_scan;       // live-row lists; the adjacency pass (lists and / or the sparse / dense decision)
    bool l0_chunked, twins;          // layer 0 of grouped rows on the chunk kernel; twin centres served together in layers >= 1
    bool l0_sparse, l0_dense;        // layer 0 of grouped rows: the sparse launch, the expand + dense pair (both: the device chooses)
    bool group_tables;               // the group projection is assembled from the per-news / per-topic tables
    int pq_x3, pq_mode;              // DIGAT_PROJ_PQ_X3; bit 0 DIGAT_PQ_BF16, bit 1 _X1, bit 2 _FP8
    int fmt, lfmt, bd_disp;          // gemm_formats, bd_dispatch
    bool news_early;                 // small news graphs: a layer's node projections are issued a phase early
    bool news_lists;                 // live-node lists of the news graphs
    int news_sparse_mode;            // Eq. 8 of larger news graphs: DIGAT_XATTN_SPARSE when the caller says so, else _DENSE
    bool news_cached0, news_indexed0;   // layer 0's news projections are the caller's rows; ... read in place through news_index
    bool user_ctx_fused;             // the user context is the one fused launch
    int side_mode;                   // 0 = never, 1 = always, 2 = by pass size
    bool side_wanted;                // this pass wants a side stream (whether it gets one: side_stream())
};

// ---- the initial user context in one launch (user_ctx0_kernel, digat_ctx0.inc) ----------------------------------------------------
// The kernel's LDS image: M [ceil(C1 / 16) * 16, H | 1], per-wave score scratch [waves, 64], four 64-entry tables (+ 4), 16 per-wave
// floats, and the pooled topics [C1, d]
static inline size_t ctx0_lds_bytes(int H, int C1, int d) {
    const size_t ct = (size_t)(C1 + 15) / 16, waves = (size_t)(d + 63) / 64;
    return (ct * 16 * (size_t)(H | 1) + waves * 64 + 3 * 64 + 68 + 16 + (size_t)C1 * d) * 4;
}
// Does (H, C + 1, d) fit the kernel?  The history rows of a wave's 64 channels live in registers (H <= 64: 16 four-row steps; the
// 16-step instantiation is bounded to 512 threads like topic_pool_resident_kernel<16>, so H > 52 needs d <= 512), one wave per 64
// channels (d <= 1024), one lane per bucket (C1 <= 64), and at least two workgroups' LDS images per CU (64 KB each at most).
static inline bool ctx0_fits(int H, int C1, int d) {
    return H >= 1 && H <= 64 && d > 0 && d % 4 == 0 && d <= 1024 && C1 >= 1 && C1 <= 64 && (H <= 52 || d <= 512) &&
           ctx0_lds_bytes(H, C1, d) <= (size_t)64 * 1024;
}
// The plan bit: the folded pass's FIRST user context is the GEMM F x = ue W^T + user_ctx0_kernel, for every variant and operand
// format, with and without the fused user context (which keeps governing calls 1..L).  A function of the plan's input beside
// EncoderPlan rather than a member of it: it depends on the shape alone.
static inline bool encoder_plan_ctx0(const EncoderPlanIn& in) { return in.folded && ctx0_fits(in.H, in.C + 1, in.d); }

static inline EncoderPlan encoder_plan(const EncoderPlanIn& in) {
    EncoderPlan pl = {};
    const int flags = in.flags, B = in.B, N = in.N, H = in.H, C = in.C, d = in.d, L = in.L, U = H + C;
    const bool grouped = in.variant == ENC_GROUPED, folded = in.folded;
    pl.status = pl.status_after_carve = DIGAT_OK;
    pl.folded = folded;
    // ---- refusals, in the entries' order: arguments, then shapes
    if (in.hist_hpq0 != in.topic_hpq0) { pl.status = DIGAT_ERR_ARG; return pl; }
    if (in.ctxq0 && !in.c_n0) { pl.status = DIGAT_ERR_ARG; return pl; }          // the queries belong to a given news context
    if (grouped && in.G <= 0) { pl.status = DIGAT_ERR_ARG; return pl; }
    if (B < 0 || N <= 0 || H < 0) { pl.status = DIGAT_ERR_ARG; return pl; }
    if (grouped && !folded) { pl.status = DIGAT_ERR_ARG; return pl; }            // grouped = folded path
    if (d <= 0 || d % 4 || L < 0 || L > DIGAT_MAX_DEPTH || N > DIGAT_MAX_NODES || U > DIGAT_MAX_NODES || C < 0) { pl.status = DIGAT_ERR_SHAPE; return pl; }
    if (grouped && (size_t)4 * in.G > (size_t)B) { pl.status = DIGAT_ERR_SHAPE; return pl; }   // the group-level projections reuse one [B,U,d] buffer
    // per-news tables read in place: only where layer 0 of the news graph is the one reader of the node table (given c_n0,
    // cached projections, the small-graph kernel), or, for larger news graphs, the sparse Eq. 8 kernel through the candidate ids
    if (in.news_index && !(in.c_n0 && in.news_hpq0 && L > 0 && eq8_row_fits_wave(d) && in.news_rows > 0 && in.news_rows <= 0x7fffffffLL &&
                           (eq8_small_graph(N) || ((flags & DIGAT_NEWS_XATTN_SPARSE) && N <= DIGAT_MAX_NODES)) && folded))
        pl.status_after_carve = DIGAT_ERR_ARG;

    // ---- the path
    // Shared-user runs: taken when the group-indexed kernels of layer 0 apply (sparse Eq. 8 on the live lists); otherwise the
    // runs are ignored: the plain per-row path.
    pl.shared = in.variant == ENC_SHARED && folded && L > 0 && (flags & 3) == DIGAT_XATTN_SPARSE && !(flags & DIGAT_PARAMS_NO_LIVE_ROWS) &&
                eq8_multi_centre_fits(d, U) && eq8_sparse_graph(U);
    pl.by_group = grouped || pl.shared;
    // Rows of one impression share the user nodes.  When every reader of the layer-0 nodes can go through the group index (the
    // sparse Eq. 8 kernel and the topic pooling can; the dense tile / aggregation kernels cannot) they are built once per GROUP.
    pl.xu0_grouped = grouped && folded && L > 0 && (flags & 3) == DIGAT_XATTN_SPARSE && eq8_row_fits_wave(d) && eq8_sparse_graph(U) && 3 * (long)in.G <= B;
    pl.c_n0_in_place = in.c_n0 && folded && L > 0;
    pl.ctxq0 = folded && in.ctxq0 && in.c_n0;
    const GemmFormats f = gemm_formats(flags, nullptr);
    pl.fmt = f.fmt; pl.lfmt = f.lfmt; pl.bd_disp = bd_dispatch(flags);
    pl.pq_x3 = (flags & DIGAT_PROJ_PQ_X3) ? 1 : 0;
    pl.pq_mode = ((flags & DIGAT_PQ_BF16) ? 1 : 0) | ((flags & DIGAT_PQ_X1) ? 2 : 0) | ((flags & DIGAT_PQ_FP8) ? 4 : 0);
    // Eq. 8 of the user graph: the sparse kernel, the dense pair, or both with the device choosing (the choice comes out of the
    // adjacency pass)
    pl.sparse_mode = flags & 3;
    if (pl.sparse_mode == 3 || (pl.sparse_mode == DIGAT_XATTN_AUTO && L == 0)) pl.sparse_mode = DIGAT_XATTN_DENSE;
    pl.xu0_shared = pl.shared && pl.sparse_mode == DIGAT_XATTN_SPARSE;
    pl.want_live = L > 0 && !(flags & DIGAT_PARAMS_NO_LIVE_ROWS);
    pl.want_scan = pl.want_live || pl.sparse_mode == DIGAT_XATTN_AUTO;
    pl.l0_chunked = pl.by_group && (pl.xu0_grouped || pl.shared) && pl.want_live && pl.sparse_mode == DIGAT_XATTN_SPARSE && eq8_multi_centre_fits(d, U);
    pl.twins = pl.want_live && pl.sparse_mode == DIGAT_XATTN_SPARSE && eq8_multi_centre_fits(d, U) && L > 1;
    const bool group_l0 = folded && L > 0 && pl.by_group;       // layer 0 of the user graph goes through the group index
    pl.l0_sparse = group_l0 && pl.sparse_mode != DIGAT_XATTN_DENSE && eq8_row_fits_wave(d);
    pl.l0_dense = group_l0 && !(pl.sparse_mode == DIGAT_XATTN_SPARSE && eq8_row_fits_wave(d));
    pl.group_tables = group_l0 && !pl.shared && in.hist_hpq0 && in.topic_hpq0 && (long)B * U >= 2048;
    // Small news graphs (the small-graph score kernel adds K3 itself): the node projections of a layer depend only on the news
    // nodes, so they are issued a phase early — same arithmetic with and without the side stream.
    pl.news_early = L > 0 && eq8_small_graph(N) && eq8_row_fits_wave(d);
    // The padding slots of a news graph are dead nodes.  Larger graphs on the sparse kernel: projection and Eq. 8 run on the live
    // list.  Small graphs: the projections of layers >= 1 do, from 2 048 rows up (below, the three list launches sit on the news
    // chain's critical path and cost what two smaller projections save).
    const bool news_lists_on = L > 0 && eq8_row_fits_wave(d) && !(flags & DIGAT_PARAMS_NO_LIVE_ROWS);
    pl.news_lists = news_lists_on && ((!pl.news_early && (flags & DIGAT_NEWS_XATTN_SPARSE) && eq8_sparse_graph(N)) || (pl.news_early && L > 1 && B >= 2048));
    pl.news_sparse_mode = (flags & DIGAT_NEWS_XATTN_SPARSE) ? DIGAT_XATTN_SPARSE : DIGAT_XATTN_DENSE;
    pl.news_cached0 = folded && L > 0 && in.news_hpq0;
    pl.news_indexed0 = pl.news_cached0 && in.news_index;
    pl.user_ctx_fused = in.fsplit && pl.fmt == 1 && in.ctx_fused_fits;
    // side stream: never, always (the caller's flags), or by pass size (default): below 2 048 rows the news kernels are a few waves
    // of workgroups each; from 2 048 rows up every kernel fills the chip by itself and the second stream only makes launches share it
    pl.side_mode = (flags & DIGAT_PARAMS_SIDE_STREAM_OFF) ? 0 : ((flags & DIGAT_PARAMS_SIDE_STREAM_ON) ? 1 : 2);
    pl.side_wanted = folded && !(pl.side_mode == 0 || (pl.side_mode == 2 && B >= 2048));
    return pl;
}

// ---- how the strip-mined GEMM's launches are tiled (flags bits 13-14: A/B switches, no result depends on them) -------------------
// GemmArgs::ragged of the launches that ask for ragged 240-column tiles (featureAffine):
// DIGAT_GEMM_RAGGED (1), DIGAT_GEMM_RAGGED_ROWMAJOR (2), or 0 = nobody asks
static inline int encoder_ragged(int flags) { return (flags & DIGAT_PARAMS_RAGGED_OFF) ? 0 : ((flags & DIGAT_PARAMS_RAGGED_ROWMAJOR) ? 2 : 1); }
