// digat_gemm_plan.h — the arguments of every GEMM launch and the launch plan: which kernel instantiation runs it, on which grid,
// and what the launch returns.  Plain C++, no HIP types: digat_gemm.inc launches what gemm_plan decides, and
// tests/test_gemm_plan_cpu.py builds this header with the host compiler to pin the decision per shape.
#pragma once
#include <stdint.h>
#include "../../include/digat_hip.h"

enum { EPI_NONE = 0, EPI_RELU_RES = 1, EPI_GATE = 2, EPI_ACCUM = 3,     // ACCUM: y += result (backward sums)
       EPI_ADD_E0 = 4 };   // y = result + e0 (strip-mined kernel only: a residual gradient joins without a copy + read-modify-write)

struct GemmArgs {
    const float* a0; long lda0; int k0;      // columns [0,k0) of A come from a0 ...
    const float* a1; long lda1;              // ... columns [k0,K) from a1 (gate: [local ; global])
    const float* w[3]; const float* bias[3]; float* y[3]; long ldy;
    int nseg, nsegs, M, K, transW;           // transW: w_s stored [K, nseg] (y = A @ w)
    int epi;
    const float* e0; long lde0; const float* e1; long lde1; const float* e2; long lde2;
    int mtiles, ntiles;
    const unsigned short* wsplit;            // bf16x6 path: [3 planes][nsegs*nseg][K] bf16 of the weights
    const float* radd; int radd_seg, rows_per_b;   // segment radd_seg: y += radd[row / rows_per_b][col]  (K3 + K1 of Eq. 8)
    unsigned long long* exec_rows;                 // profiling only: += rows processed by a row-list launch
    const int* rowidx; const int* nrows_dev;       // bf16x6 kernel only: process rows rowidx[0 .. *nrows_dev) of A / y (live rows)
    int gather_only;                               // with rowidx: only A is indexed (embedding lookup), y rows are 0 .. M-1
    int m_dispatch;                                // != 0: choose the kernel as if M were this (bit-identical results across batchings)
    int x3_segs;                                   // bf16x6 kernel: bit s set = segment s with the three leading products only
                                                   // (hi*hi, mid*hi, hi*mid: relative error ~2^-16 instead of ~2^-24)
    int x1_segs;                                   // ... bit s set = segment s with the leading product alone (hi*hi: ~2^-8)
    int bf16_segs;                                 // ... bit s set = y[s] is a bf16 array (round to nearest even), ldy in elements
    int fp8_segs; long ldy8;                       // ... bit s set = y[s] is an array of block-scaled e4m3 rows, ldy8 BYTES apart:
                                                   // [nseg bytes of OCP e4m3 | nseg / 80 fp32 scales, one per 80-column strip | pad]
                                                   // (value = e4m3 x scale; scale = the strip's absmax / 448: see the epilogue)
    int format;                                    // operand format of the strip-mined kernel AND of the wsplit image: 0 = three bf16
                                                   // pieces, six products ("bf16x6"); 1 = two scaled fp16 pieces, three products ("fp16x3")
    unsigned* range_flag;                          // fp16x3 only, optional: |= 1 when an activation leaves the format's range (|x| >= 4094)
    const uint8_t* dmask; long lddm; float dscale; // bf16x6 kernel, optional: y = (result [+ e0]) x (dmask[row][col] ? dscale : 0) — the backward
    int dmask_cols;                                // of the dropout in front of the layer (training: dX through the keep bytes [M, lddm]);
                                                   // dmask_cols > 0: the mask has that many columns, output columns beyond them are left as computed
    int ragged;                                    // != 0 ASKS for ragged 240-column tiles where N is no multiple of 240 (gemm_plan decides: see
                                                   // GemmPlan::ragged); DIGAT_GEMM_RAGGED: full-width tiles dispatched first, _ROWMAJOR: row-tile-major
    int strips;                                    // set by launch_gemm for a ragged launch: the 80-column strips of N (the last tile has strips % 3)
};
enum { DIGAT_GEMM_RAGGED = 1, DIGAT_GEMM_RAGGED_ROWMAJOR = 2 };

// Every GEMM kernel instantiation the library launches, X(id, kernel): the GemmKernel values, their names and launch_gemm's
// switch are all made from this one list.
#define DIGAT_GEMM_KERNELS(X)                                        \
    X(F16F8C_3, gemm_f16f8c_kernel<3>)                               \
    X(F16F8C_1, gemm_f16f8c_kernel<1>)                               \
    X(SKINNY_TW_2, gemm_skinny_kernel<2, false, true>)               \
    X(SKINNY_TW_1, gemm_skinny_kernel<1, false, true>)               \
    X(SKINNY_SPLIT_F16_2, gemm_skinny_split_kernel<2, true>)         \
    X(SKINNY_SPLIT_F16_1, gemm_skinny_split_kernel<1, true>)         \
    X(SKINNY_SPLIT_BF16_2, gemm_skinny_split_kernel<2, false>)       \
    X(SKINNY_SPLIT_BF16_1, gemm_skinny_split_kernel<1, false>)       \
    X(SKINNY_2_KTAIL, gemm_skinny_kernel<2, true, false>)            \
    X(SKINNY_2, gemm_skinny_kernel<2, false, false>)                 \
    X(SKINNY_1_KTAIL, gemm_skinny_kernel<1, true, false>)            \
    X(SKINNY_1, gemm_skinny_kernel<1, false, false>)                 \
    X(STRIP_3_F16_64, gemm_bf16x6s_kernel<3, true, 1, false>)        \
    X(STRIP_1_F16_64, gemm_bf16x6s_kernel<1, true, 1, false>)        \
    X(STRIP_3_BF16_64, gemm_bf16x6s_kernel<3, false, 1, false>)      \
    X(STRIP_1_BF16_64, gemm_bf16x6s_kernel<1, false, 1, false>)      \
    X(STRIP_3_F16_FULL, gemm_bf16x6s_kernel<3, true, 2, true>)       \
    X(STRIP_3_F16, gemm_bf16x6s_kernel<3, true, 2, false>)           \
    X(STRIP_3_BF16, gemm_bf16x6s_kernel<3, false, 2, false>)         \
    X(STRIP_1_F16, gemm_bf16x6s_kernel<1, true, 2, false>)           \
    X(STRIP_1_BF16, gemm_bf16x6s_kernel<1, false, 2, false>)         \
    X(F32_128_PROJ, gemm_f32_kernel<128, 80, 4, 1, 1, 1>)            \
    X(F32_128, gemm_f32_kernel<128, 80, 4, 1, 1, 0>)                 \
    X(F32_64, gemm_f32_kernel<64, 80, 4, 1, 2, 0>)                   \
    X(F32_32, gemm_f32_kernel<32, 64, 1, 4, 2, 0>)

enum GemmKernel {
    GEMM_NONE,             // no kernel implements the launch (refused: see GemmPlan::status)
    GEMM_PER_SEGMENT,      // one launch_gemm per weight segment (a tile must lie inside one segment)
#define DIGAT_GEMM_ENUM(id, ...) GEMM_##id,
    DIGAT_GEMM_KERNELS(DIGAT_GEMM_ENUM)
#undef DIGAT_GEMM_ENUM
};

static inline const char* gemm_kernel_name(int kernel) {
#define DIGAT_GEMM_NAME(id, ...) if (kernel == GEMM_##id) return #__VA_ARGS__;
    DIGAT_GEMM_KERNELS(DIGAT_GEMM_NAME)
#undef DIGAT_GEMM_NAME
    return kernel == GEMM_PER_SEGMENT ? "per segment" : "none";
}

struct GemmPlan {
    int status;            // DIGAT_OK, or the error the launch returns without launching anything
    int kernel;            // GemmKernel: the kernel the dispatch chose (also when the launch is refused)
    int mtiles, ntiles;    // the kernel's tile counts (GemmArgs::mtiles / ntiles)
    unsigned grid, block;
    int image_format;      // the format the kernel reads GemmArgs::wsplit in (the image must have been split in it); -1: no image
    int ragged;            // != 0: the kernel's ragged instantiation (the same symbol with RAG = true): ntiles = ceil(strips / 3), the
                           // last column tile has strips % 3 strips; the value is GemmArgs::ragged (the tile order)
};

static inline bool gemm_kernel_takes_row_list(int kernel) {
    return kernel == GEMM_F16F8C_3 || kernel == GEMM_F16F8C_1 || (kernel >= GEMM_STRIP_3_F16_64 && kernel <= GEMM_STRIP_1_BF16);
}

// The whole dispatch of launch_gemm, in its order of decisions.  `kind` (DIGAT_KERNEL_*) only names the large fp32 kernel's
// instantiation, so that profiles list the Eq. 8 projections under their own symbol.
static inline GemmPlan gemm_plan(const GemmArgs& g, int kind = DIGAT_KERNEL_LINEAR) {
    GemmPlan p = {DIGAT_OK, GEMM_NONE, 0, 0, 0, 256, -1, 0};
    const int Ntot = g.nseg * g.nsegs;
    const int Md = g.m_dispatch > 0 ? g.m_dispatch : g.M;
    const auto tiles = [&](int kernel, int mtiles, int ntiles, bool round8) {
        p.kernel = kernel; p.mtiles = mtiles; p.ntiles = ntiles;
        p.grid = round8 ? (unsigned)(((mtiles * ntiles + 7) / 8) * 8) : (unsigned)(mtiles * ntiles);
        if (g.rowidx && !gemm_kernel_takes_row_list(kernel)) p.status = DIGAT_ERR_ARG;
        return p;
    };

    // 1. DIGAT_GEMM_F16F8C: gemm_f16f8c_kernel at every row count (no other kernel reads its images; anything it does not
    //    implement is refused, never sent elsewhere).  Without an image (d % 80 != 0: nothing was split) the launch runs fp32,
    //    as fp16x3's would.
    if (g.format == DIGAT_GEMM_F16F8C && g.wsplit) {
        const bool ok = g.nseg % 80 == 0 && g.K % 4 == 0 && g.k0 == g.K && !g.a1 && !g.transW && g.lda0 % 4 == 0 &&
                        ((uintptr_t)g.a0 & 15) == 0 && g.ldy % 4 == 0 && g.lde0 % 4 == 0 &&
                        (g.epi == EPI_NONE || g.epi == EPI_RELU_RES || g.epi == EPI_ACCUM || g.epi == EPI_ADD_E0) &&
                        !g.x1_segs && !g.x3_segs && !g.bf16_segs && !g.fp8_segs && !g.dmask;
        if (!ok) { p.status = DIGAT_ERR_ARG; return p; }
        const int strips = Ntot / 80;
        p.image_format = DIGAT_GEMM_F16F8C;
        p.block = 512;
        return strips % 3 == 0 ? tiles(GEMM_F16F8C_3, (g.M + 127) / 128, strips / 3, true)
                               : tiles(GEMM_F16F8C_1, (g.M + 127) / 128, strips, true);
    }
    // 2. the input gradient of a [B,d] linear: the skinny kernel with the weight read as its transpose (16 us on the 32x64
    //    LDS-tiled kernel, 34 launches per training step)
    if (Md < 2048 && g.nseg % 80 == 0 && g.transW && g.nsegs == 1 && g.K % 16 == 0 && g.k0 == g.K && !g.radd && !g.a1) {
        const int ntiles = Ntot / 80;
        if (((g.M + 31) / 32) * ntiles >= 480 || g.K >= 800) return tiles(GEMM_SKINNY_TW_2, (g.M + 31) / 32, ntiles, false);
        return tiles(GEMM_SKINNY_TW_1, (g.M + 15) / 16, ntiles, false);
    }
    // 3. up to 2 048 rows, the [B,d] linears of the inference path on the weights' split images (the encoder's linears say which
    //    kernel they want through m_dispatch: 1 = this one at every row count — the gate's two-operand launch always does: the
    //    tiled split-operand kernel does not take [c_n | pooled], and at 4 096 rows it fell to the fp32 kernel on 160
    //    workgroups, 88 us against 33 us here)
    if (Md < 2048 && g.wsplit && g.nseg % 80 == 0 && !g.transW && g.K % 8 == 0 && g.k0 % 8 == 0 && !g.radd && !g.rowidx &&
        g.ldy % 4 == 0 && g.lda0 % 4 == 0 && (!g.a1 || g.lda1 % 4 == 0) && g.lde0 % 4 == 0 && g.lde1 % 4 == 0 && g.lde2 % 4 == 0 &&
        (g.epi == EPI_NONE || g.epi == EPI_RELU_RES || g.epi == EPI_GATE || g.epi == EPI_ACCUM)) {
        if (g.format != DIGAT_GEMM_BF16X6 && g.format != DIGAT_GEMM_F16X3) p.status = DIGAT_ERR_ARG;
        p.image_format = g.format;
        const int ntiles = Ntot / 80;
        // 32-row tiles (half the weight traffic) once that leaves at least 320 workgroups; the gate's K = 800 launch is faster on
        // 16-row tiles too (1.014 -> 1.010 ms per step): twice the workgroups for its long per-wave chain of K tiles
        const bool mt2 = ((g.M + 31) / 32) * ntiles >= 320;
        const bool f16 = g.format == DIGAT_GEMM_F16X3;
        return tiles(mt2 ? (f16 ? GEMM_SKINNY_SPLIT_F16_2 : GEMM_SKINNY_SPLIT_BF16_2) : (f16 ? GEMM_SKINNY_SPLIT_F16_1 : GEMM_SKINNY_SPLIT_BF16_1),
                     mt2 ? (g.M + 31) / 32 : (g.M + 15) / 16, ntiles, false);
    }
    // 4. the fp32 skinny kernel.  32-row tiles halve the weight traffic from L2 (what these launches wait for) and halve the
    //    workgroups: taken when that still leaves about two per CU, or when K is long (measured: 1024x1200x400 28.6 -> 26.0 us,
    //    1024x400x800 28.8 -> 25.7 us, 1024x400x400 17.8 -> 18.4 us)
    if (Md < 2048 && g.nseg % 80 == 0 && !g.transW && g.K % 4 == 0 && g.k0 % 16 == 0 && !g.radd) {
        const int ntiles = Ntot / 80;
        const bool ktail = (g.K & 15) != 0;
        if (((g.M + 31) / 32) * ntiles >= 480 || g.K >= 800)
            return tiles(ktail ? GEMM_SKINNY_2_KTAIL : GEMM_SKINNY_2, (g.M + 31) / 32, ntiles, false);
        return tiles(ktail ? GEMM_SKINNY_1_KTAIL : GEMM_SKINNY_1, (g.M + 15) / 16, ntiles, false);
    }
    // fp32 tile configuration: 128x80 for the big projections; below 2048 rows 32x64 (most workgroups), or 64x80 for
    // multi-segment launches whose segments are multiples of 80 columns (d = 400); the small-M shapes keep two K tiles in flight
    const int cfg = Md >= 2048 ? 0 : ((g.nsegs > 1 && g.nseg % 80 == 0) ? 1 : 2);
    const int bn = cfg == 2 ? 64 : 80;
    // 5. a tile must lie inside one weight segment; when the tile width does not divide the segment (only small test shapes),
    //    run the segments one launch each
    if (g.nsegs > 1 && g.nseg % bn != 0) return tiles(GEMM_PER_SEGMENT, 0, 0, false);
    // 6. the strip-mined kernel on the split images
    if (g.wsplit && cfg == 0 && g.nseg % 80 == 0 && g.K % 4 == 0 && g.K >= 32 && g.ldy % 4 == 0 && g.lde0 % 4 == 0 &&
        (g.epi == EPI_NONE || g.epi == EPI_RELU_RES || g.epi == EPI_ACCUM || g.epi == EPI_ADD_E0) && g.k0 == g.K && !g.transW) {
        if (g.format != DIGAT_GEMM_BF16X6 && g.format != DIGAT_GEMM_F16X3) p.status = DIGAT_ERR_ARG;
        // a row-list launch addresses its rows as 32-bit byte offsets from the operand's start (the kernel's LDS-DMA pieces)
        else if (g.rowidx && (unsigned long long)g.M * (unsigned long long)g.lda0 * 4ull >= (1ull << 32)) p.status = DIGAT_ERR_SHAPE;
        p.image_format = g.format;
        const bool f16 = g.format == DIGAT_GEMM_F16X3;
        const int strips = Ntot / 80;
        const bool three = strips % 3 == 0;                // 240-column tiles: the operand split is paid once per three strips
        const int ntiles = three ? strips / 3 : strips;
        // Launches that leave the chip under-filled at 128-row tiles (a 4 096-row pass's [B,d] linears and news-side projections:
        // 160 workgroups for 256 CUs, each a 13-step latency chain) take 64-row tiles: twice the workgroups, the same chain; the
        // same for the bf16x6 launches of a training step's news graph (3 200 rows: 125 workgroups at 128-row tiles) without a row list
        // (a launch that asks for ragged tiles counts its workgroups at m_dispatch, like the choice of this kernel: the same bits at every batching)
        const int Mfill = g.ragged ? Md : g.M;
        if (((Mfill + 127) / 128) * ntiles < 400 && (f16 || !g.rowidx)) {
            const int k = f16 ? (three ? GEMM_STRIP_3_F16_64 : GEMM_STRIP_1_F16_64) : (three ? GEMM_STRIP_3_BF16_64 : GEMM_STRIP_1_BF16_64);
            return tiles(k, (g.M + 63) / 64, ntiles, true);
        }
        // FULL: every segment takes all its products (what inference launches ask for)
        const int k = three ? (f16 ? (!g.x1_segs && !g.x3_segs ? GEMM_STRIP_3_F16_FULL : GEMM_STRIP_3_F16) : GEMM_STRIP_3_BF16)
                            : (f16 ? GEMM_STRIP_1_F16 : GEMM_STRIP_1_BF16);
        // Ragged 240-column tiles, for launches that ask (GemmArgs::ragged) and whose N is no multiple of 240: ceil(strips / 3) column
        // tiles, the last with strips % 3 strips, instead of one-strip tiles that fetch and split the A tile once per strip.  The
        // grid holds, per XCD, the XCD's share of the full-width tiles and then its share of the short ones (long tiles first).
        if (g.ragged && !three && strips > 3) {
            const int mt = (g.M + 127) / 128, nt = (strips + 2) / 3;
            tiles(f16 ? (!g.x1_segs && !g.x3_segs ? GEMM_STRIP_3_F16_FULL : GEMM_STRIP_3_F16) : GEMM_STRIP_3_BF16, mt, nt, true);
            p.grid = (unsigned)(8 * ((mt * (nt - 1) + 7) / 8 + (mt + 7) / 8));
            p.ragged = g.ragged;
            return p;
        }
        return tiles(k, (g.M + 127) / 128, ntiles, true);
    }
    // 7. the fp32 MFMA kernel
    const int bm = cfg == 0 ? 128 : (cfg == 1 ? 64 : 32);
    const int k = cfg == 0 ? (kind == DIGAT_KERNEL_PROJ ? GEMM_F32_128_PROJ : GEMM_F32_128) : (cfg == 1 ? GEMM_F32_64 : GEMM_F32_32);
    return tiles(k, (g.M + bm - 1) / bm, (Ntot + bn - 1) / bn, true);
}

// Does the kernel that runs this launch take a row list (rowidx / nrows_dev)?  Callers ask before they hand one over, or bf16 /
// e4m3 output segments (which the strip-mined kernel takes and the fp16-fp8c kernel refuses).
static inline bool gemm_takes_row_list(const GemmArgs& g) { return gemm_kernel_takes_row_list(gemm_plan(g).kernel); }
