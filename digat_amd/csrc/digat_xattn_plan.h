// digat_xattn_plan.h — every launch decision of Eq. 8: the limits of its kernels, the tile plan of the all-pairs score kernel, and one
// route per entry that chooses kernels (which kernel instantiation runs, on which grid, behind which device flag, and what a refused
// call returns).  Plain C++, no HIP types: digat_xattn.inc / digat_train.inc launch what the routes decide, digat_encoder_plan.h asks
// the same predicates, and tests/test_xattn_plan_cpu.py builds this header with the host compiler to pin every route per input.
//
// Training: eq8_train_fwd_route and eq8_train_bwd_route stand side by side and share their predicates.  They are NOT symmetric, and
// need not be — xattn_mode is a hint, both sides of every choice compute the same function, and the backward reads only what every
// forward saves (alpha, the scores before leaky_relu): for 512 < d <= 1024 the forward may run entry-wise (a row as four pieces per
// lane) while the backward is all-pairs whatever the mode (its entry-wise kernels hold two pieces per lane): eq8_train_entrywise_bwd.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/digat_hip.h"

// compile-time knobs the grids depend on (the kernels read the same names)
#ifndef DIGAT_TWIN_R
#define DIGAT_TWIN_R 2          // twin centres per wave (see xattn_sparse_twin_kernel)
#endif
#ifndef DIGAT_TWIN_WPG
#define DIGAT_TWIN_WPG 4        // waves per workgroup of the twin kernel
#endif
#ifndef DIGAT_L0_ROWS
#define DIGAT_L0_ROWS 4         // rows of one impression per wave of the layer-0 chunk kernel
#endif

// ---- the limits of the kernels: stated here and nowhere else --------------------------------------------------------------------
// float4 pieces of a row per lane of a wave-per-centre kernel (the template parameter U): 1, 2, 4, or 0 = the row does not fit a wave
static inline int eq8_width(int d4) { return d4 <= 64 ? 1 : (d4 <= 128 ? 2 : (d4 <= 256 ? 4 : 0)); }
// the wave-per-centre sparse kernel and the small-graph kernels hold a row as at most four float4 pieces per lane
static inline bool eq8_row_fits_wave(int d) { return eq8_width(d / 4) != 0; }
// kernels that keep several centres per wave, and the entry-wise backward, hold at most two
static inline bool eq8_row_fits_two_pieces(int d) { return eq8_row_fits_wave(d) && eq8_width(d / 4) <= 2; }
// a lane pair holds a centre's adjacency row: two words
static inline bool eq8_wave_graph(int n) { return n <= 128; }
// the layer-0 chunk kernel and the twin kernel keep several centres per wave: two float4 pieces per lane, one adjacency word pair
static inline bool eq8_multi_centre_fits(int d, int n) { return eq8_row_fits_two_pieces(d) && eq8_wave_graph(n); }
// graphs the sparse kernel serves: up to 16 nodes belong to the small-graph kernels (the graph in LDS, a workgroup per graph)
static inline bool eq8_sparse_graph(int n) { return n > 16; }
static inline bool eq8_small_graph(int n) { return n <= 16; }
// the small-graph kernels run a graph: a wave per centre, the neighbours across the lanes' registers
static inline bool eq8_small_kernel_fits(int n, int d) { return eq8_small_graph(n) && eq8_row_fits_wave(d); }
// training, the entry-wise kernels (a wave per centre / per node over the adjacency's entries): the forward is the sparse kernel
// on graphs the small-graph kernel does not take; the backward pair was written for two pieces per lane and sums K3's gradient
// into dr — so for 512 < d <= 1024 (or without dr) a forward that ran entry-wise is followed by the all-pairs backward
static inline bool eq8_train_entrywise_fwd(int n, int d) { return !eq8_small_kernel_fits(n, d) && eq8_row_fits_wave(d); }
static inline bool eq8_train_entrywise_bwd(int d, bool dr) { return eq8_row_fits_two_pieces(d) && dr; }

// ---- what a route hands to the launch side --------------------------------------------------------------------------------------
enum Eq8Kernel {
    EQ8_NONE,            // nothing is launched
    EQ8_SMALL_LDS,       // xattn_small_lds_kernel<U>: a graph in LDS, score + softmax + aggregation
    EQ8_SMALL,           // xattn_score_small_kernel<U>: a wave per centre of a small graph
    EQ8_TILE,            // xattn_score_kernel: all pairs, 4 x 4 tiles (XattnTile)
    EQ8_AGG,             // xattn_agg_kernel<maxt>
    EQ8_SPARSE,          // xattn_sparse_kernel<U, pq16, radd, train>
    EQ8_TWIN,            // xattn_sparse_twin_kernel<U, R>
    EQ8_L0,              // xattn_sparse_l0_kernel<U, R>
    EQ8_SPARSE_BWD,      // xattn_sparse_bwd_centre_kernel<U>, then xattn_sparse_bwd_node_kernel<U>
    EQ8_PAIR_BWD,        // xattn_pair_bwd_kernel<ch>
};
enum Eq8Guard { EQ8_UNGUARDED, EQ8_SKIP_IF, EQ8_RUN_IF };   // the device int of the launch: returns at once when it is != 0 / when it is 0

struct Eq8Launch {
    int kernel;                      // Eq8Kernel
    int U, pq16, R, maxt, ch;        // template parameters (those the kernel has; 0 otherwise)
    bool radd, train;
    unsigned grid, grid_y, block;
    size_t lds;                      // dynamic LDS bytes
    bool raise_lds;                  // more than 64 KiB: the kernel's 160 KiB attribute must have been raised
    int xcd_group;                   // SparseArgs::xcd_group of the launch
    int guard;                       // Eq8Guard
};

// ---- the tile plan of xattn_score_kernel ----------------------------------------------------------------------------------------
constexpr int XA_RING = 3;   // chunk images in the LDS ring
constexpr int XA_KMAX = 4;   // DMA wave-instructions one wave issues per chunk (upper bound)

// the geometry fields of ScoreArgs (see there), the workgroup, its dynamic LDS and the grid
struct XattnTile {
    int status;
    int B, n, d, d4;
    int NT, SN, CC4, nchunks, RB, img_slots, ring_slots, ninstr, am_off, a_off, tl_off, ld_off, pm_off;
    int threads; size_t lds; int blocks;
};

static inline size_t eq8_align16(size_t v) { return (v + 15) / 16 * 16; }

static inline XattnTile xattn_tile_plan(int B, int n, int d) {
    XattnTile g = {};
    if (B < 0 || n <= 0 || d <= 0) { g.status = DIGAT_ERR_ARG; return g; }
    if (d % 4 != 0 || n > DIGAT_MAX_NODES) { g.status = DIGAT_ERR_SHAPE; return g; }
    g.B = B; g.n = n; g.d = d; g.d4 = d / 4;
    g.NT = (n + 3) / 4;
    g.SN = (n + 3) / 4 * 4;
    const int tiles = g.NT * g.NT;
    int threads, rbmax;
    if (tiles >= 128) { threads = (tiles + 63) / 64 * 64; rbmax = 1; }
    else { threads = 256; rbmax = 256 / tiles; }
    if (rbmax > B && B > 0) rbmax = B;
    const int nwaves = threads / 64;
    int bestRB = 0, bestCC = 0;
    // <= 40 KiB keeps 4 workgroups per CU (1024 rows = one round on 256 CUs); graphs too large for
    // that may take up to 150 KiB.  The DMA ring must sit in the first 64 KiB of LDS (M0 addressing).
    // Phase 0 stages the adjacency bytes at the start of LDS, below the bit rows at am_off = max(ring, scores).  The three budgets
    // are first tried with the bytes inside the ring alone; wide graphs of few channels (n >= 111 at d = 4: a 12 KiB ring, 12 - 16 KiB
    // of bytes) find no plan that way, and a second round (`relaxed`) lets the bytes reach into the score area, which is idle until
    // the chunk loop has ended.  Plans of the first round are never replaced.
    for (int pass = 0; pass < 6 && !bestRB; ++pass) {
        const bool relaxed = pass >= 3;
        const int budget = pass % 3;
        const size_t lds_budget = budget == 0 ? 40 * 1024 : (budget == 1 ? 64 * 1024 : 150 * 1024);
        for (int rb = rbmax; rb >= 1 && !bestRB; --rb) {
            int cc_ok = 0;
            // odd chunk widths first (conflict-free LDS reads), widest first
            for (int odd = 1; odd >= 0 && !cc_ok; --odd) {
                for (int cc = g.d4; cc >= 1; --cc) {
                    if (g.d4 % cc || (cc & 1) != odd) continue;
                    const long img = (long)rb * 4 * g.NT * cc;
                    const long ring_slots = (2 * img + 63) / 64 * 64;
                    if (ring_slots / 64 > (long)XA_KMAX * nwaves) continue;
                    if ((size_t)XA_RING * ring_slots * 16 > 60 * 1024) continue;
                    const size_t sc = (size_t)rb * n * g.SN * 4;
                    const size_t ringb = (size_t)XA_RING * ring_slots * 16;
                    const size_t stage = (relaxed && sc > ringb) ? sc : ringb;     // where the byte image of phase 0 may lie
                    if ((size_t)rb * n * n + 32 > stage) continue;
                    const size_t tot = eq8_align16(ringb > sc ? ringb : sc) + (size_t)rb * n * ((n + 31) / 32) * 4
                                       + (size_t)d * 4 + ((size_t)rb * tiles + 16) * 4 + (size_t)rb * 8 * g.NT * 4
                                       + (size_t)2 * rb * n * 4;
                    if (2 * rb * 4 * g.NT > threads) continue;           // one thread per image row for the linear terms
                    if (tot > lds_budget) continue;
                    cc_ok = cc;
                    break;
                }
            }
            const int want = g.d4 < 5 ? 1 : 5;
            if (cc_ok >= want || (rb == 1 && cc_ok >= 1)) { bestRB = rb; bestCC = cc_ok; }
        }
    }
    if (!bestRB) { g.status = DIGAT_ERR_SHAPE; return g; }
    g.RB = bestRB; g.CC4 = bestCC; g.nchunks = g.d4 / g.CC4;
    g.img_slots = g.RB * 4 * g.NT * g.CC4;
    g.ring_slots = (2 * g.img_slots + 63) / 64 * 64;
    g.ninstr = g.ring_slots / 64;
    const size_t ringb = (size_t)XA_RING * g.ring_slots * 16;
    const size_t sc = (size_t)g.RB * n * g.SN * 4;
    g.am_off = (int)eq8_align16(ringb > sc ? ringb : sc);
    g.a_off = g.am_off + (int)eq8_align16((size_t)g.RB * n * ((n + 31) / 32) * 4);
    g.tl_off = g.a_off + d * 4;
    g.ld_off = g.tl_off + (g.RB * tiles + 16) * 4;
    g.pm_off = g.ld_off + g.RB * 8 * g.NT * 4;
    g.lds = g.pm_off + (size_t)2 * g.RB * n * 4;
    g.threads = threads;
    g.blocks = (B + g.RB - 1) / g.RB;
    return g;
}

// the score launch of a tile plan: the small-graph kernels where they fit (lds_form: the caller's fused form — aggregation here, no
// centre-side group index, no scores kept — which the graph-in-LDS kernel serves when P' and h of a graph fit 64 KB: LDS-DMA
// addresses go through M0), the tile kernel otherwise
static inline Eq8Launch eq8_score_launch(const XattnTile& t, bool lds_form, int guard) {
    Eq8Launch l = {};
    l.guard = guard; l.grid_y = 1;
    if (eq8_small_kernel_fits(t.n, t.d)) {
        const size_t lds = (size_t)2 * (((size_t)t.n * t.d4 + 63) / 64) * 1024;
        l.U = eq8_width(t.d4); l.block = 256;
        if (lds_form && lds <= 64 * 1024) { l.kernel = EQ8_SMALL_LDS; l.grid = (unsigned)t.B; l.lds = lds; }
        else { l.kernel = EQ8_SMALL; l.grid = (unsigned)(((long)t.B * t.n + 3) / 4); }
        return l;
    }
    l.kernel = EQ8_TILE; l.grid = (unsigned)t.blocks; l.block = (unsigned)t.threads; l.lds = t.lds; l.raise_lds = t.lds > 64 * 1024;
    return l;
}

// ---- aggregation: out = relu(alpha h) + X, a workgroup per row, a wave per 64 channels (up to 16 waves: from d = 1028 a wave takes
// several groups); alpha[b] and the live flags in LDS.  upto_1024: the GAT layer and the training forward keep the limit their other
// kernels were written and tested for (d <= 1024)
struct Eq8AggRoute { int status; int groups, sa; Eq8Launch launch; };     // groups, sa: AggArgs's fields of those names
static inline Eq8AggRoute eq8_agg_route(int B, int n, int d, bool upto_1024, int guard) {
    Eq8AggRoute r = {};
    r.groups = (d + 63) / 64; r.sa = n | 1;
    if (upto_1024 && r.groups > 16) { r.status = DIGAT_ERR_SHAPE; return r; }
    Eq8Launch& l = r.launch;
    l.kernel = EQ8_AGG; l.maxt = r.groups <= 8 ? 512 : 1024;
    l.grid = (unsigned)B; l.grid_y = 1; l.block = 64u * (unsigned)(r.groups < 16 ? r.groups : 16);
    l.lds = (size_t)n * r.sa * 4 + n;
    l.guard = guard;
    return r;
}

// ---- inference pairwise (launch_xattn_pairwise): score + aggregation, or both in one small-graph launch ----------------------------
struct Eq8PairIn { int B, n, d; bool alpha_wanted, live, group, radd, bindex, guarded; };     // the optional inputs: was it passed
struct Eq8PairRoute {
    int status;
    bool fused;                      // small graphs whose alpha nobody asked for: score, softmax and aggregation in one launch
    XattnTile tile;
    Eq8Launch score;                 // kernel == EQ8_NONE with status == DIGAT_OK: B == 0, nothing to do
    Eq8AggRoute agg;                 // !fused
};
static inline Eq8PairRoute eq8_pair_route(const Eq8PairIn& in) {
    Eq8PairRoute r = {};
    r.tile = xattn_tile_plan(in.B, in.n, in.d);
    r.status = r.tile.status;
    if (r.status || in.B == 0) return r;
    const bool small = eq8_small_kernel_fits(in.n, in.d);
    if (in.bindex && (in.alpha_wanted || in.live || in.group || !small)) { r.status = DIGAT_ERR_SHAPE; return r; }   // fused small-graph form only
    if (in.radd && !small) { r.status = DIGAT_ERR_SHAPE; return r; }        // only the small-graph kernels add K3 themselves
    const int guard = in.guarded ? EQ8_SKIP_IF : EQ8_UNGUARDED;
    r.fused = !in.alpha_wanted && small && !in.live && !in.group;
    r.score = eq8_score_launch(r.tile, r.fused, guard);
    if (!r.fused) r.agg = eq8_agg_route(in.B, in.n, in.d, false, guard);
    return r;
}

// ---- the wave-per-centre sparse kernels (launch_sparse, launch_sparse_l0, the training forward) -----------------------------------
struct Eq8SparseIn {
    int B, n, d4;
    bool train;                      // the training forward's instantiation (alpha and the scores leave the wave)
    bool radd, group, xgroup, live, run_if, fill_flags, rowidx, nrows_dev;      // SparseArgs's optional fields: was it passed
    bool twin;                       // twin, twlist and twcount, all three
    int pq16, centre_limit;
    long ld8;
};
struct Eq8SparseRoute { int status; Eq8Launch launch; };

// One wave per centre.  The grid covers every centre, or — guarded launches (run_if: the device decides between this kernel and the
// dense pair) — a fixed number of workgroups that stride over the centres, so that the launch that is NOT wanted costs a couple of
// microseconds of empty workgroups instead of one per four centres.
static inline Eq8SparseRoute eq8_sparse_route(const Eq8SparseIn& in) {
    Eq8SparseRoute r = {};
    if (!eq8_wave_graph(in.n) || !eq8_width(in.d4)) { r.status = DIGAT_ERR_SHAPE; return r; }
    Eq8Launch& l = r.launch;
    unsigned blocks = (unsigned)(((long)in.B * in.n + 3) / 4);
    const unsigned guarded_cap = in.train ? 8192u : 2048u;
    if (in.run_if && blocks > guarded_cap) blocks = guarded_cap;
    // 16: runs of 64 consecutive centres (about two user graphs) per XCD; measured 1.431 vs 1.442 ms per step against the
    // dispatcher's plain round-robin (0), 8: 1.434, 4: 1.436, 2: 1.443 (tools/exp/ab.sh, two alternating runs each)
    l.xcd_group = 16;
    blocks = (blocks + 8u * l.xcd_group - 1) / (8u * l.xcd_group) * (8u * l.xcd_group);       // whole windows of 8 x xcd_group workgroups
    l.U = eq8_width(in.d4); l.grid_y = 1;
    l.guard = in.run_if ? EQ8_RUN_IF : EQ8_UNGUARDED;
    if (in.train) { l.kernel = EQ8_SPARSE; l.train = true; l.grid = blocks; l.block = 256; return r; }
    if (in.twin && in.rowidx && !in.pq16 && !in.radd && !in.group && !in.run_if && !in.fill_flags && l.U <= 2) {
        // centres with equal adjacency rows together (xattn_sparse_twin_kernel); how many lead is known on the device only: a capped
        // grid whose waves stride over the list
        constexpr unsigned TWIN_GRID_CAP = 8192;
        if (blocks > TWIN_GRID_CAP) blocks = TWIN_GRID_CAP;
        l.kernel = EQ8_TWIN; l.R = DIGAT_TWIN_R;
        l.grid = (blocks * 4 + DIGAT_TWIN_WPG - 1) / DIGAT_TWIN_WPG; l.block = 64 * DIGAT_TWIN_WPG;
        return r;
    }
    if (in.pq16 == 2) {  // P' and Q as block-scaled e4m3 rows (projection GEMM with fp8 segments: 80-channel strips, d = 4 d4)
        if (in.radd || in.d4 % 20 || in.ld8 < 4 * in.d4 + 4 * (in.d4 / 20) || (in.ld8 & 7)) return Eq8SparseRoute{DIGAT_ERR_SHAPE, {}};
    } else if (in.pq16) {   // P' and Q in bf16 (projection GEMM with bf16 segments); K3 is in P' already: no radd here
        if (in.radd || (in.d4 & 1)) return Eq8SparseRoute{DIGAT_ERR_SHAPE, {}};
    }
    l.kernel = EQ8_SPARSE; l.pq16 = in.pq16 == 2 ? 2 : (in.pq16 ? 1 : 0); l.radd = in.radd;
    l.grid = blocks; l.block = 256;
    return r;
}

// layer 0 of grouped rows on the chunk kernel (xattn_sparse_l0_kernel): eligibility, and a grid of at most ceil(rows of a group / R)
// chunks per group — B / R + G chunks, n centres each
struct Eq8L0Route { bool eligible; Eq8Launch launch; };
static inline Eq8L0Route eq8_l0_route(const Eq8SparseIn& in, int G) {
    Eq8L0Route r = {};
    r.eligible = in.group && in.xgroup && in.radd && in.rowidx && in.nrows_dev && in.live && !in.run_if && !in.pq16 && !in.fill_flags &&
                 !in.centre_limit && eq8_multi_centre_fits(4 * in.d4, in.n);
    if (!r.eligible) return r;
    Eq8Launch& l = r.launch;
    l.kernel = EQ8_L0; l.U = eq8_width(in.d4); l.R = DIGAT_L0_ROWS;
    l.xcd_group = 16;       // runs of workgroups per XCD, as in eq8_sparse_route
    const unsigned blocks = (unsigned)((((long)in.B / DIGAT_L0_ROWS + G) * in.n + 3) / 4);
    l.grid = (blocks + 8u * l.xcd_group - 1) / (8u * l.xcd_group) * (8u * l.xcd_group);
    l.grid_y = 1; l.block = 256;
    l.guard = EQ8_UNGUARDED;
    return r;
}

// ---- training: forward and backward side by side ----------------------------------------------------------------------------------
// mode: DIGAT_TRAIN_XATTN_AUTO (the device's choice, where the caller passed a flag), _SPARSE (entry-wise), _DENSE (all pairs) — a
// hint: each direction follows it where its own kernels fit (see the head of this file)
struct Eq8TrainIn { int B, n, d, mode; bool flag, dr; };      // flag: the device int of the choice was passed; dr: K3's gradient is wanted
enum Eq8TrainPath {
    EQ8_TRAIN_NOTHING,       // B == 0, or refused
    EQ8_TRAIN_SMALL,         // the small-graph kernel scores, drops and aggregates from registers
    EQ8_TRAIN_ENTRYWISE,     // the sparse kernel alone
    EQ8_TRAIN_GUARDED,       // the decision, then the sparse kernel and the all-pairs pair: the device's flag lets one of them run
    EQ8_TRAIN_ALLPAIRS,      // tile score kernel + aggregation
};
struct Eq8TrainFwdRoute {
    int status; int path;
    XattnTile tile;
    Eq8Launch sparse;        // ENTRYWISE, GUARDED
    Eq8Launch score;         // SMALL, GUARDED, ALLPAIRS
    Eq8AggRoute agg;         // GUARDED, ALLPAIRS
};
static inline Eq8TrainFwdRoute eq8_train_fwd_route(const Eq8TrainIn& in) {
    Eq8TrainFwdRoute r = {};
    r.tile = xattn_tile_plan(in.B, in.n, in.d);
    r.status = r.tile.status;
    if (r.status || in.B == 0) return r;
    const bool small = eq8_small_kernel_fits(in.n, in.d);
    const bool eligible = eq8_train_entrywise_fwd(in.n, in.d);
    const bool guarded = eligible && in.flag && in.mode == DIGAT_TRAIN_XATTN_AUTO;
    Eq8SparseIn s = {};
    s.B = in.B; s.n = in.n; s.d4 = in.d / 4; s.train = true; s.run_if = guarded;
    if (eligible && (guarded || in.mode == DIGAT_TRAIN_XATTN_SPARSE)) {
        const Eq8SparseRoute sr = eq8_sparse_route(s);
        r.status = sr.status; r.sparse = sr.launch;
        if (r.status) return r;
        if (!guarded) { r.path = EQ8_TRAIN_ENTRYWISE; return r; }      // the caller knows the corpus is sparse
    }
    const int guard = guarded ? EQ8_SKIP_IF : EQ8_UNGUARDED;
    if (!small) {
        r.agg = eq8_agg_route(in.B, in.n, in.d, true, guard);
        r.status = r.agg.status;
        if (r.status) return r;
    }
    r.path = small ? EQ8_TRAIN_SMALL : (guarded ? EQ8_TRAIN_GUARDED : EQ8_TRAIN_ALLPAIRS);
    r.score = eq8_score_launch(r.tile, false, guard);        // the scores are kept: never the graph-in-LDS kernel
    return r;
}

struct Eq8TrainBwdRoute {
    bool only_sparse;        // the entry-wise pair alone, unguarded
    bool guard;              // both sides behind the forward's flag
    Eq8Launch sparse;        // only_sparse or guard: the centre and the node kernel, one launch each on this grid
    Eq8Launch pair;          // !only_sparse: the all-pairs dP', dQ, da kernel (behind launch_ds and launch_aggT)
};
static inline Eq8TrainBwdRoute eq8_train_bwd_route(const Eq8TrainIn& in) {
    Eq8TrainBwdRoute r = {};
    const bool eligible = eq8_train_entrywise_bwd(in.d, in.dr);
    // graphs of at most 16 nodes (the news graph): a centre has at most 16 entries whatever the adjacency — always the entry-wise pair
    // (the all-pairs launches walk 13 channel chunks per row for a 10 x 10 product: 65 us per layer against 20)
    r.only_sparse = eligible && (in.mode == DIGAT_TRAIN_XATTN_SPARSE || eq8_small_graph(in.n)) && in.mode != DIGAT_TRAIN_XATTN_DENSE;
    r.guard = eligible && !r.only_sparse && in.flag && in.mode == DIGAT_TRAIN_XATTN_AUTO;
    const int guard = r.guard ? EQ8_RUN_IF : EQ8_UNGUARDED;
    if (r.guard || r.only_sparse) {
        Eq8Launch& l = r.sparse;
        l.kernel = EQ8_SPARSE_BWD; l.U = eq8_width(in.d / 4);
        l.grid = (unsigned)(((long)in.B * in.n + 3) / 4); l.grid_y = 1; l.block = 256; l.guard = guard;
    }
    if (!r.only_sparse) {
        // P', Q and the gradient of `ch` channels of a graph, ds and the adjacency in LDS: 64 channels where that fits 160 KiB (n <= 112)
        const size_t n = (size_t)in.n;
        const auto lds_of = [&](int ch) { return ((size_t)3 * n * ch + n * n) * 4 + 2 * ((n * n + 3) & ~(size_t)3) + 2 * n * 4; };
        Eq8Launch& l = r.pair;
        l.kernel = EQ8_PAIR_BWD; l.ch = lds_of(64) <= 160 * 1024 ? 64 : 32;
        l.lds = lds_of(l.ch); l.raise_lds = l.lds > 64 * 1024;
        l.grid = (unsigned)in.B; l.grid_y = (unsigned)((in.d + l.ch - 1) / l.ch); l.block = 1024;
        l.guard = r.guard ? EQ8_SKIP_IF : EQ8_UNGUARDED;
    }
    return r;
}
