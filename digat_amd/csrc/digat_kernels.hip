// digat_kernels.hip — hand-written gfx950 (MI355X / CDNA4) kernels for DIGAT's dual-graph
// interaction hot path, and the C ABI declared in include/digat_hip.h.
//
// One translation unit; the kernels live in the .inc files next to this one (DESIGN.md has the data layout and
// the roofline of each):
//   digat_gemm.inc     nn.Linear on the matrix cores: exact fp32 (v_mfma_f32_16x16x4_f32) with fused epilogues, the
//                      strip-mined "bf16x6" kernel of the node projections (LDS-DMA operands, optional row list),
//                      the skinny [B,d] linears
//   digat_xattn.inc    Eq. 8: relu(K3+K1+K2).a -> leaky_relu -> -1e9 mask -> softmax_j -> relu(alpha @ h) + X,
//                      never materialising [B,n,n,d]
//   digat_context.inc  ScaledDotProductAttention pooling (key projection folded into the query); torch_scatter's
//                      scatter_softmax + scatter_sum over history categories
//   digat_glue.inc     user-node build, group expansion, live-row lists, row logits
//   digat_train.inc    backward / training kernels;  digat_eval.inc  per-impression ranking + metrics
//   digat_news.inc     MSA news encoder (inference);  digat_gat.inc  vanilla-GAT layer of the ablation encoders
//   digat_user_graph.inc  user graphs and category masks from category indices
//   digat_train_input.inc  the training input: an epoch's negative samples, the index lists of a step
//   digat_dot_topk.inc  inner-product retrieval: fp32 matrix-core product fused with the top-k selection of digat_topk.inc
//   digat_dot_rank.inc  retrieval evaluation: the same product fused with the rank of given targets in the whole pool
//   digat_pool_softmax.inc  retrieval training: the same product fused with the softmax loss over the whole pool and its gradients
//   digat_mmr.inc  diversified top-k: a short list's Gram in LDS and the greedy maximal-marginal-relevance picks on it
//   digat_listq.inc  list quality: the same Gram reduced to a list's diversity, with category spread, overlap and exposure
//   digat_calibrate.inc  calibrated top-k: the greedy re-rank of a shortlist of up to 1024 towards the category mix of the history
//   digat_pl_sample.inc  stochastic lists: Plackett-Luce slates drawn from a list of up to 1024, with the probability of the draw
//   digat_pl_expect.inc  doubly robust off-policy value: a logged slate's per-step expectation of an item value under the target, beside Z_t
//   digat_rerank.inc  joint re-rank: diversity, calibration and a cap per category in one greedy pass over up to 1024 entries, no Gram
// This file: shared helpers, the per-kernel profiler, and the C ABI.  The encoder's orchestration is digat_encoder.inc (host
// code only), and every decision of an encoder call is made in digat_encoder_plan.h, every launch decision of Eq. 8 in
// digat_xattn_plan.h, every one of the GEMM in digat_gemm_plan.h (plain C++, pinned by CPU tests).
//
// gfx950 only: 64-wide wavefronts, 160 KiB LDS per CU, MFMA f32 16x16x4.  No CUDA shims.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <utility>

#include "../../include/digat_hip.h"
#include "digat_encoder_plan.h"
#include "digat_xattn_plan.h"

typedef float v4f __attribute__((ext_vector_type(4)));

#define DIGAT_CHECK_LAUNCH()                                   \
    do {                                                       \
        if (hipGetLastError() != hipSuccess) return DIGAT_ERR_LAUNCH; \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Bump allocator over a caller buffer in 256-byte-aligned regions; `ok` turns false on overflow.  Arena() only measures: no
// buffer, no limit, take() hands out nullptr and `used` ends as the size of the carve (the *_workspace_bytes queries run the
// carve of their entry this way, so a layout is written once).
struct Arena {
    char* base; size_t cap, used; bool ok;
    Arena() : base(nullptr), cap(SIZE_MAX), used(0), ok(true) {}
    Arena(void* p, size_t n) : base((char*)p), cap(n), used(0), ok(p != nullptr) {}
    template <class T> T* take(size_t count) {
        const size_t bytes = align_up(count * sizeof(T), 256);
        if (!ok || used + bytes > cap) { ok = false; return nullptr; }
        T* r = base ? (T*)(base + used) : nullptr;
        used += bytes;
        return r;
    }
    Arena sub(size_t bytes) {           // the next `bytes` as an arena of their own (a measuring arena hands out a measuring one)
        Arena r;
        r.base = take<char>(bytes); r.cap = bytes; r.ok = ok;
        return r;
    }
};
// the size of a buffer that two carves share (a training pair's workspace: the forward's layout or the backward's); an entry that
// has held its buffer to that size carves either layout without a further check
static inline size_t larger(const Arena& a, const Arena& b) { return a.used > b.used ? a.used : b.used; }
// {pointer, floats} pairs zero-filled on the stream: the gradients of a backward call over an empty batch
static int zero_floats(hipStream_t st, std::initializer_list<std::pair<float*, size_t>> bufs) {
    for (const auto& b : bufs)
        if (hipMemsetAsync(b.first, 0, b.second * 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    return DIGAT_OK;
}

// ---- optional per-kernel event timing (bench.py's roofline leg) ---------------------------------
// Between digat_profile_start and digat_profile_stop every launch is bracketed by two hipEvents
// recorded on the stream the kernel is launched on; stop() synchronises once and sums elapsed time
// and the algorithmic work (flops for the MFMA kernels, bytes for the others) per kernel kind.
static struct {
    int enabled, cap, used;
    hipEvent_t* ev;
    int* kind;
    double* work;
    unsigned long long* rows_dev;      // [kinds] row-list GEMM launches add the rows they actually processed (device counters)
    double flops_per_row[16]; double rows_nominal[16];
    unsigned kind_mask;                // only launches of these kinds are bracketed (digat_profile_set_kinds)
    double* bytes;                     // MFMA kinds: the operand + result bytes of the launch (digat_profile_gemm_bytes)
    double bytes_per_row[16];
    int* part;                         // DIGAT_KERNEL_XATTN launches: which Eq. 8 kernel (XPART_*; digat_profile_xattn_parts)
} g_prof = {0, 0, 0, nullptr, nullptr, nullptr, nullptr, {0.0}, {0.0}, ~0u, nullptr, {0.0}, nullptr};

// The Eq. 8 launches are three unlike kernels with their own byte budgets: they are timed and priced apart (bench.py:
// roofline_xattn.parts).  Device-side byte counts of a part (live-row lists: known on the device only) go to rows_dev[8 + part].
enum { XPART_TWIN = 0,      // user graph, layers >= 1: row-list launches (twin kernel / wave per live centre)
       XPART_L0 = 1,        // user graph, layer 0 of grouped rows (chunk kernel / wave per live centre through the group index)
       XPART_NEWS = 2,      // news graphs of <= 16 nodes, the graph in LDS (fused)
       XPART_OTHER = 3,     // everything else: dense score launches, larger news graphs on the sparse kernel
       XATTN_PARTS = 4 };

struct ProfScope {
    hipStream_t st; int slot;
    ProfScope(int kind, double work, hipStream_t s, double bytes = 0.0, int part = XPART_OTHER) : st(s), slot(-1) {
        if (g_prof.enabled && ((g_prof.kind_mask >> kind) & 1u) && g_prof.used < g_prof.cap) {
            slot = g_prof.used++;
            g_prof.kind[slot] = kind; g_prof.work[slot] = work; g_prof.bytes[slot] = bytes; g_prof.part[slot] = part;
            (void)hipEventRecord(g_prof.ev[2 * slot], st);
        }
    }
    ~ProfScope() { if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], st); }
};

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float f4_comp(const float4& v, int s) {
    return s == 0 ? v.x : (s == 1 ? v.y : (s == 2 ? v.z : v.w));
}
// Wave-wide reductions, result in every lane.  Within a row of 16 lanes the operands move by DPP (quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror: VALU modifiers, no LDS crossbar round trip as __shfl_xor / ds_bpermute has); the
// four row results are read back with v_readlane and combined.  Fixed order -> deterministic; every lane sees the same
// bits (each step adds the same two values in both partners; float + is commutative).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_bcast(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// Round 5: the four row sums S0..S3 meet by two more DPP steps instead of four v_readlane + two v_mov + three v_add on uniform
// values (9 vector instructions -> 3; the Eq. 8 kernels are vector-issue-bound and reduce once per (centre, neighbour) pair):
// row_bcast:15 adds lane 15 of row k to every lane of row k + 1 (rows 1 and 3: S0 + S1, S2 + S3), row_bcast:31 adds lane 31
// (= S0 + S1) to rows 2 and 3, so lane 63 holds (S3 + S2) + (S1 + S0) — THE BITS of the old (S0 + S1) + (S2 + S3): float + is
// commutative, the association is the same.  Disabled rows keep their value (row_mask).  The s_nop's are the DPP read-after-write
// wait states hipcc would insert itself for a builtin (inline asm is not padded: cdna_hip_programming.md section 5.7).
#ifndef DIGAT_WAVE_REDUCE_BCAST
#define DIGAT_WAVE_REDUCE_BCAST 1
#endif
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);      // row_half_mirror
    v += dpp_mov<0x140>(v);      // row_mirror: every lane holds the sum of its row of 16
#if DIGAT_WAVE_REDUCE_BCAST
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1" : "+v"(v));
    return lane_bcast(v, 63);
#else
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
#endif
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
#if DIGAT_WAVE_REDUCE_BCAST
    asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1" : "+v"(v));
    return lane_bcast(v, 63);
#else
    return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
#endif
}

// one 16-byte-per-lane global -> LDS copy; LDS address = lds_byte_addr (wave-uniform) + 16*lane.
// Invisible to hipcc's waitcnt bookkeeping: completion is counted by hand (wait_vmcnt below).
__device__ __forceinline__ void lds_dma16(const float* gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
// The same copy with the source as (wave-uniform 64-bit base in SGPRs) + (32-bit byte offset per lane): no 64-bit vector add per
// piece, and M0 is written but neither saved nor restored (round 5: the GEMM's main loop is bound by instruction ISSUE — 1.5
// non-MFMA instructions per MFMA — and a third of those were this helper's M0 save / restore and its callers' address adds).
// Only for kernels in which nothing else depends on M0 (gfx9 LDS instructions do not; the ISA of every user is checked for it).
__device__ __forceinline__ void lds_dma16_s(const void* sbase_any, unsigned voff, unsigned lds_byte_addr) {
    // the base IS wave-uniform; where the compiler cannot prove it (a row count loaded from memory) it is made so explicitly
    const unsigned long long bits = (unsigned long long)(uintptr_t)sbase_any;
    const void* sbase = (const void*)(uintptr_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bits >> 32)) << 32) |
                                                 (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)bits));
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt_imm() {        // s_waitcnt vmcnt(N) with a compile-time N (0 .. 63)
    // gfx9 encoding of the s_waitcnt immediate: vmcnt low bits [3:0], expcnt [6:4] = 7, lgkmcnt [11:8] = 15, vmcnt high bits [15:14]
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_vmcnt(int n) {      // n is wave-uniform
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;      // callers pass 0 .. 6; anything else waits for more than asked
    }
}

// Round 5: TWO twins per wave at five waves per SIMD (94 registers) instead of four at four (114): 280 against 305 us per 4 096-row
// launch alone, 460-510 against 535-570 inside the overlapped region (tools/exp/ab.py, alternating runs; three at five waves spill):
// DIGAT_TWIN_R = 2 (digat_xattn_plan.h, with the twin kernel's grid)
// leaky_relu(0.2) of a WAVE-UNIFORM score (a wave_sum result): e > 0 ? e : 0.2 e = max(e, 0.2 e), bit for bit (also for -0, inf, NaN),
// as one multiply and one v_max_f32 with the score as the scalar operand (fmaxf costs a third instruction that canonicalises e)
__device__ __forceinline__ float leaky02_uniform(float e) {
    const float t = 0.2f * e;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "s"(e), "v"(t));
    return r;
}
// Dropout of the training path: a counter-based hash of (seed, flat element index) against floor(p 2^32) — every kernel that applies a
// dropout (dropout_fwd_kernel and the fused sites: the Eq. 8 scores, the gate, the pooled topics) draws element e's bit from here,
// so a fused site lands on the elements the stand-alone launch would have (oracle/digat_oracle.py restates it for the tests)
__host__ __device__ __forceinline__ unsigned hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ unsigned drop_threshold(float p) { return (unsigned)(p * 4294967296.0); }
__device__ __forceinline__ bool drop_keep(unsigned seed, long e, unsigned thr) {
    return hash32((unsigned)e * 0x9E3779B9U + hash32(seed + (unsigned)(e >> 32))) >= thr;
}
constexpr int TWIN_R = DIGAT_TWIN_R;   // centres with equal adjacency rows served by one wave (user_live_flags_kernel, xattn_sparse_twin_kernel)
#include "digat_gemm.inc"
#include "digat_xattn.inc"
#include "digat_context.inc"
#include "digat_ctx0.inc"
#include "digat_ctxfused.inc"
#include "digat_glue.inc"

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int digat_version(void) { return DIGAT_ABI_VERSION; }

const char* digat_error_string(int code) {
    switch (code) {
        case DIGAT_OK: return "ok";
        case DIGAT_ERR_ARG: return "bad argument (null pointer or negative size)";
        case DIGAT_ERR_SHAPE: return "unsupported shape (d % 4 != 0, graph larger than DIGAT_MAX_NODES, depth too large)";
        case DIGAT_ERR_WORKSPACE: return "workspace too small";
        case DIGAT_ERR_LAUNCH: return "HIP kernel launch failed";
        default: return "unknown error";
    }
}

int digat_linear_f32(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                     int M, int N, int K, void* stream) {
    if (!x || !w || !y || M < 0 || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    if (K % 4 || ldx % 4) return DIGAT_ERR_SHAPE;
    return launch_gemm(gemm_plain(x, ldx, w, b, y, ldy, M, N, K, 0), (hipStream_t)stream);
}

// ---- a1 / a2 ------------------------------------------------------------------------------------
// Eq. 8 workspace: [h | P | Q] [B,n,d] back to back (one three-segment projection writes them), r [B,d] (K3), alpha [B,n,n]
struct XattnWs { float *h, *P, *Q, *r, *alpha; };
static XattnWs xattn_carve(Arena& a, int B, int n, int d) {
    const size_t nd = (size_t)B * n * d;
    XattnWs w{};
    w.h = a.take<float>(3 * nd);
    if (w.h) { w.P = w.h + nd; w.Q = w.P + nd; }
    w.r = a.take<float>((size_t)B * d);
    w.alpha = a.take<float>((size_t)B * n * n);
    return w;
}
size_t digat_xattn_workspace_bytes(int B, int n, int d) { Arena a; xattn_carve(a, B, n, d); return a.used; }

int digat_xattn_pairwise_fwd(const float* Pr, const float* Q, const float* h, const float* X,
                             const float* a, const uint8_t* A, float* out, float* alpha,
                             int B, int n, int d, void* stream) {
    if (!Pr || !Q || !h || !X || !a || !A || !out || !alpha) return DIGAT_ERR_ARG;
    return launch_xattn_pairwise(Pr, Q, h, X, a, A, out, alpha, B, n, d, (hipStream_t)stream);
}

struct TwinLists { const unsigned* word; const int* list; const int* count; };     // user_live_flags_kernel's twins (see there)

// xattn_core's optional inputs; what a caller does not set stays off
struct XattnOpts {
    const void* wsplit = nullptr;                                                   // split weight image: bf16x6 / f16x3 projections
    const int* rowidx = nullptr; const int* nrows_dev = nullptr; const uint8_t* live = nullptr;      // live-row lists
    int sparse_mode = DIGAT_XATTN_DENSE; const int* sparse_flag = nullptr;
    int pq_x3 = 0, pq_mode = 0, centre_limit = 0, gemm_format = 0, prof_part = 0;
    unsigned* range_flag = nullptr; const TwinLists* tw = nullptr;
};

// [h | P | Q] = X [W | F1 | F2]^T (+ bW on h): the three-segment node projection of an Eq. 8 layer, one pass over X on the matrix
// cores.  wsplit non-NULL: split operands in `format` on the bf16 / fp16 / fp8 matrix cores; pq_x3 (DIGAT_PROJ_PQ_X3): P and Q
// (segments 1, 2) with three products.  Every launch of this projection is built here; a caller adds only what differs
// (m_dispatch, a row list, xattn_core its K3 addend and the bf16 / fp8 output segments).
static GemmArgs proj3_args(const float* X, int M, int d, const float* W, const float* bW, const float* F1, const float* F2,
                           float* h, float* P, float* Q, const void* wsplit, int pq_x3, int format, unsigned* range_flag) {
    GemmArgs g = gemm_plain(X, d, W, bW, h, d, M, d, d, 0);
    g.w[1] = F1; g.bias[1] = nullptr; g.y[1] = P;
    g.w[2] = F2; g.bias[2] = nullptr; g.y[2] = Q;
    g.nsegs = 3;
    g.x3_segs = pq_x3 ? 6 : 0;
    g.wsplit = (const unsigned short*)wsplit;
    g.format = format; g.range_flag = range_flag;
    return g;
}

// Eq. 8 layer with K3 (r = ctx F3^T + b3) already computed; `r_given` may live anywhere.  The workspace is carved at this n
// (the encoder's is sized for the larger of its two graphs).
static int xattn_core(const float* X, const uint8_t* A, const float* r_given,
                      const float* W, const float* bW, const float* F1, const float* F2, const float* a,
                      float* out, float* alpha_out, int B, int n, int d, void* workspace, size_t workspace_bytes, hipStream_t st,
                      const XattnOpts& o = XattnOpts()) {
    Arena ar(workspace, workspace_bytes);
    const XattnWs w = xattn_carve(ar, B, n, d);
    if (!ar.ok) return DIGAT_ERR_WORKSPACE;
    const int* rowidx = o.rowidx; const int* nrows_dev = o.nrows_dev; const uint8_t* live = o.live;
    const int sparse_mode = o.sparse_mode, pq_mode = o.pq_mode;
    float *h = w.h, *P = w.P, *Q = w.Q, *alpha = alpha_out ? alpha_out : w.alpha;
    GemmArgs g = proj3_args(X, B * n, d, W, bW, F1, F2, h, P, Q, o.wsplit, o.pq_x3, o.gemm_format, o.range_flag);
    g.radd = r_given; g.radd_seg = 1; g.rows_per_b = n; // P' = K3 + K1: the reference's left-to-right order
    const bool sparse_fits = !alpha_out && eq8_sparse_graph(n) && eq8_row_fits_wave(d);      // see xattn_sparse_kernel
    // DIGAT_PQ_BF16 (pq_mode & 1): P' and Q stored in bf16, read by the wave-per-centre sparse kernel; & 2: one product for them
    const bool pq16 = (pq_mode & 1) && gemm_takes_row_list(g) && sparse_mode == DIGAT_XATTN_SPARSE && sparse_fits &&
                      d % 8 == 0 && (long)B * n >= 2048;
    // DIGAT_PQ_FP8 (pq_mode & 4): P' and Q stored as block-scaled e4m3 rows (one fp32 scale per 80-channel strip), same reader
    const bool pq8 = (pq_mode & 4) && !(pq_mode & 1) && gemm_takes_row_list(g) && sparse_mode == DIGAT_XATTN_SPARSE && sparse_fits &&
                     d % 80 == 0 && (long)B * n >= 2048;
    const long ld8 = (long)align_up((size_t)d + 4 * (size_t)(d / 80), 64);      // [d codes | d / 80 scales | pad]: whole 64-byte lines
    if (pq16) { g.bf16_segs = 6; if (pq_mode & 2) g.x1_segs = 6; }
    if (pq8) { g.fp8_segs = 6; g.ldy8 = ld8; if (pq_mode & 2) g.x1_segs = 6; }
    const bool listed = rowidx && gemm_takes_row_list(g);
    if (listed) { g.rowidx = rowidx; g.nrows_dev = nrows_dev; }                         // live rows only (see user_live_flags_kernel)
    const int rc = launch_gemm(g, st, DIGAT_KERNEL_PROJ);
    if (rc) return rc;
    const int* skip_if = nullptr;
    if (sparse_mode != DIGAT_XATTN_DENSE && sparse_fits) {
        SparseArgs sg = sparse_args(P, Q, h, X, a, A, out, B, n, d / 4);
        if (listed) sg.live = live;
        if (listed && live) { sg.rowidx = rowidx; sg.nrows_dev = nrows_dev; }
        if (sparse_mode == DIGAT_XATTN_AUTO) sg.run_if = o.sparse_flag;
        sg.pq16 = pq8 ? 2 : (pq16 ? 1 : 0);
        sg.ld8 = pq8 ? ld8 : 0;
        sg.centre_limit = o.centre_limit;
        sg.prof_part = o.prof_part;
        if (o.tw && listed && live) { sg.twin = o.tw->word; sg.twlist = o.tw->list; sg.twcount = o.tw->count; }
        const int rcs = launch_sparse(sg, st);
        if (rcs || sparse_mode == DIGAT_XATTN_SPARSE) return rcs;
        skip_if = o.sparse_flag;
    }
    PairOpts po;
    if (listed) po.live = live;
    po.alpha_wanted = alpha_out != nullptr; po.skip_if = skip_if;
    return launch_xattn_pairwise(P, Q, h, X, a, A, out, alpha, B, n, d, st, po);
}

// the xattn entries: r = ctx F3^T + b3 (K3) into the workspace's r, then the layer
static int xattn_fwd_k3(const float* X, const uint8_t* A, const float* ctx, const float* W, const float* bW, const float* F1,
                        const float* F2, const float* F3, const float* b3, const float* a, float* out, float* alpha_out,
                        int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream, const XattnOpts& o = XattnOpts()) {
    Arena ar(workspace, workspace_bytes);
    const XattnWs w = xattn_carve(ar, B, n, d);
    if (!ar.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_gemm(gemm_plain(ctx, d, F3, b3, w.r, d, B, d, d, 0), st);
    if (rc) return rc;
    return xattn_core(X, A, w.r, W, bW, F1, F2, a, out, alpha_out, B, n, d, workspace, workspace_bytes, st, o);
}

int digat_xattn_fwd(const float* X, const uint8_t* A, const float* ctx,
                    const float* W, const float* bW, const float* F1, const float* F2,
                    const float* F3, const float* b3, const float* a,
                    float* out, float* alpha_out, int B, int n, int d,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!X || !A || !ctx || !W || !F1 || !F2 || !F3 || !a || !out || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    return xattn_fwd_k3(X, A, ctx, W, bW, F1, F2, F3, b3, a, out, alpha_out, B, n, d, workspace, workspace_bytes, stream);
}

int digat_xattn_fwd_mode(const float* X, const uint8_t* A, const float* ctx,
                         const float* W, const float* bW, const float* F1, const float* F2,
                         const float* F3, const float* b3, const float* a,
                         float* out, int B, int n, int d, int mode,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (mode != DIGAT_XATTN_DENSE && mode != DIGAT_XATTN_SPARSE) return DIGAT_ERR_ARG;
    if (!X || !A || !ctx || !W || !F1 || !F2 || !F3 || !a || !out || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    XattnOpts o;
    o.sparse_mode = mode;
    return xattn_fwd_k3(X, A, ctx, W, bW, F1, F2, F3, b3, a, out, nullptr, B, n, d, workspace, workspace_bytes, stream, o);
}

int digat_xattn_fwd_lowprec(const float* X, const uint8_t* A, const float* ctx,
                            const float* W, const float* bW, const float* F1, const float* F2,
                            const float* F3, const float* b3, const float* a, const void* wsplit, int format,
                            float* out, int B, int n, int d, int pq,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (pq < 0 || pq > 2 || (format != 0 && format != 1 && format != DIGAT_GEMM_F16F8C) || (format == DIGAT_GEMM_F16F8C && pq != 0))
        return DIGAT_ERR_ARG;
    if (!X || !A || !ctx || !W || !F1 || !F2 || !F3 || !a || !wsplit || !out || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    // the low-precision rows are the sparse kernel's alone, written by the strip-mined projection (whole 80-column strips, from 2 048 rows)
    if (d % 80 || !eq8_row_fits_wave(d) || !eq8_sparse_graph(n) || n > DIGAT_MAX_NODES || (long)B * n < 2048) return DIGAT_ERR_SHAPE;
    XattnOpts o;
    o.wsplit = wsplit; o.sparse_mode = DIGAT_XATTN_SPARSE; o.pq_mode = pq == 1 ? 1 : (pq == 2 ? 4 : 0); o.gemm_format = format;
    return xattn_fwd_k3(X, A, ctx, W, bW, F1, F2, F3, b3, a, out, nullptr, B, n, d, workspace, workspace_bytes, stream, o);
}

// ---- bf16x6 weight preparation + a directly callable linear (tests, micro-benchmarks) --------------
size_t digat_split_weights_bytes(int rows, int K) {
    return (size_t)((rows + 79) / 80) * ((K + 31) / 32) * WS_SLOTS * 16;       // one 15 KB image per (80-row strip, K tile)
}
size_t digat_split_weights_bytes_format(int rows, int K, int format) {
    if (rows <= 0 || K <= 0) return 0;
    if (format == DIGAT_GEMM_BF16X6 || format == DIGAT_GEMM_F16X3) return digat_split_weights_bytes(rows, K);
    if (format == DIGAT_GEMM_F16F8C) return (size_t)((rows + 79) / 80) * ((K + 127) / 128) * F8C_IMG_BYTES;   // 41 KB per (strip, 128-deep K tile)
    return 0;
}

// A training entry that was handed a ready-made image of its weights (digat_split_jobs: every image of a step in one launch) passes
// the image where its helpers expect their split destination and names it here: the split launch for exactly that pointer is skipped.
static thread_local const void* tl_premade_image = nullptr;
struct PremadeImage {
    const void* prev;
    explicit PremadeImage(const void* image) : prev(tl_premade_image) { tl_premade_image = image; }
    ~PremadeImage() { tl_premade_image = prev; }
};
// format: DIGAT_GEMM_BF16X6 (three bf16 pieces; what every training entry uses), DIGAT_GEMM_F16X3 (two scaled fp16 pieces) or
// DIGAT_GEMM_F16F8C (w_hi in fp16 + MX-e4m3 q(w_hi), q(w_lo): digat_split_weights_bytes_format bytes; [N, K] weights only)
static int launch_split(const float* w0, const float* w1, const float* w2, int nseg, int nsegs, int K, void* wsplit, hipStream_t st,
                        int transposed = 0, int format = 0) {
    if (format != 0 && format != 1 && format != DIGAT_GEMM_F16F8C) return DIGAT_ERR_ARG;
    if (wsplit && wsplit == tl_premade_image) return format == 0 ? DIGAT_OK : DIGAT_ERR_ARG;
    if (format == DIGAT_GEMM_F16F8C) {
        if (transposed) return DIGAT_ERR_ARG;
        const long total = (long)((nseg * nsegs + 79) / 80) * ((K + 127) / 128) * 320;      // threads: one per (image, k group, row)
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        wsplit_note(wsplit, format);
        hipLaunchKernelGGL(split_weights_f8c_kernel, dim3(blocks), dim3(256), 0, st, w0, w1, w2, nseg, nsegs, K, (unsigned char*)wsplit);
        DIGAT_CHECK_LAUNCH();
        return DIGAT_OK;
    }
    const long total = (long)nseg * nsegs * K;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    wsplit_note(wsplit, format);
    hipLaunchKernelGGL(split_weights_tiled_kernel, dim3(blocks), dim3(256), 0, st, w0, w1, w2, nseg, nsegs, K, (unsigned short*)wsplit, transposed,
                       format == 1 ? 2 : 3);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// every split image of a training step in ONE launch (blockIdx.y = job): 20 split launches per 64 x 5-row step before
size_t digat_split_job_bytes(int rows, int cols, int layout, int matrices) {
    if (rows <= 0 || cols <= 0 || (matrices != 1 && matrices != 3)) return 0;
    if (layout == 0) return digat_split_weights_bytes(rows * matrices, cols);
    if (layout == 1) return matrices == 1 ? digat_split_weights_bytes(cols, rows) : digat_split_weights_bytes(cols, 3 * rows);
    return 0;
}
int digat_split_jobs(const digat_split_job* jobs, int njobs, void* stream) {
    if (!jobs || njobs < 0 || njobs > SPLIT_MAX_JOBS) return DIGAT_ERR_ARG;
    if (njobs == 0) return DIGAT_OK;
    SplitJobsDev all;
    memset(&all, 0, sizeof(all));
    long most = 0;
    for (int k = 0; k < njobs; ++k) {
        const digat_split_job& j = jobs[k];
        const bool three = j.w1 != nullptr || j.w2 != nullptr;
        if (!j.w0 || !j.image || j.rows <= 0 || j.cols <= 0 || (three && (!j.w1 || !j.w2)) || (j.layout != 0 && j.layout != 1)) return DIGAT_ERR_ARG;
        SplitJobDev& o = all.j[k];
        o.w0 = j.w0; o.w1 = three ? j.w1 : j.w0; o.w2 = three ? j.w2 : j.w0; o.out = (unsigned short*)j.image;
        if (j.layout == 0) { o.nseg = j.rows; o.nsegs = three ? 3 : 1; o.K = j.cols; o.transposed = 0; }
        else { o.nseg = j.cols; o.nsegs = 1; o.K = three ? 3 * j.rows : j.rows; o.transposed = three ? 2 : 1; }
        const long total = (long)((o.nseg * o.nsegs + 79) / 80) * 80 * ((o.K + 31) / 32) * 4;      // 16-byte slots of the image's three planes / 3
        if (total > most) most = total;
        wsplit_note(j.image, 0);
    }
    long bx = (most + 255) / 256;
    if (bx > 2048) bx = 2048;
    hipLaunchKernelGGL(split_weights_jobs_kernel, dim3((unsigned)bx, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream, all);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_forget_split_image(const void* wsplit) { return wsplit && wsplit_forget(wsplit) ? DIGAT_OK : DIGAT_ERR_ARG; }

int digat_gather_tables(const digat_gather_job* jobs, int njobs, void* stream) {
    if (!jobs || njobs < 0 || njobs > GATHER_MAX_JOBS) return DIGAT_ERR_ARG;
    if (njobs == 0) return DIGAT_OK;
    GatherTableJobs all;
    memset(&all, 0, sizeof(all));
    long most = 0;
    for (int k = 0; k < njobs; ++k) {
        const digat_gather_job& j = jobs[k];
        if (j.rows < 0 || j.row_bytes <= 0 || (j.rows > 0 && (!j.src || !j.dst || !j.idx)) || (j.idx2 && j.inner <= 0)) return DIGAT_ERR_ARG;
        all.job[k] = j;
        if (!j.idx2) all.job[k].inner = 1;
        const long units = (j.row_bytes & 15) == 0 ? j.rows * (j.row_bytes >> 4) : j.rows * j.row_bytes;
        if (units > most) most = units;
    }
    if (most == 0) return DIGAT_OK;
    long bx = (most + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(gather_tables_kernel, dim3((unsigned)bx, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream, all);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_user_row_runs(const float* ue, const uint8_t* Au, const uint8_t* cat_mask, const int64_t* cat_idx, int B, int H, int U, int C1, int d,
                        int32_t* row_group, int64_t* leaders, int32_t* n_runs, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ue || !Au || !cat_mask || !cat_idx || !row_group || !leaders || !n_runs || !workspace || B <= 0 || H < 0 || U <= 0 || C1 <= 0 || d <= 0)
        return DIGAT_ERR_ARG;
    if (d % 4 || ((long)H * d) % 4) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < (size_t)B) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* same = (uint8_t*)workspace;
    ProfScope prof(DIGAT_KERNEL_GLUE, (double)B * ((double)H * d * 4 + (double)U * U + C1 + 8.0 * H), st);
    hipLaunchKernelGGL(user_rows_same_kernel, dim3(B), dim3(256), 0, st, (const uint4*)ue, Au, cat_mask, cat_idx, B, (long)H * d / 4, U * U, C1, H, same);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(user_row_runs_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t*)same, B, row_group, leaders, n_runs);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_split_proj_weights(const float* W, const float* F1, const float* F2, int d, void* wsplit, int format, void* stream) {
    if (!W || !F1 || !F2 || !wsplit || d <= 0) return DIGAT_ERR_ARG;
    return launch_split(W, F1, F2, d, 3, d, wsplit, (hipStream_t)stream, 0, format);
}

size_t digat_split_ctx_fused_bytes(int d) { return d > 0 ? ctxfused_image_bytes(d) : 0; }
int digat_split_ctx_fused_weights(const float* W, int d, void* image, void* stream) {
    if (!W || !image || d <= 0) return DIGAT_ERR_ARG;
    if (d % 8) return DIGAT_ERR_SHAPE;
    const long total = (long)(ctxfused_image_bytes(d) / 16);
    hipLaunchKernelGGL(split_weights_ctxfused_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, d, (uint4*)image);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_split_weights(const float* W, int N, int K, void* wsplit, int format, void* stream) {
    if (!W || !wsplit || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    return launch_split(W, W, W, N, 1, K, wsplit, (hipStream_t)stream, 0, format);
}

#ifdef DIGAT_CF_TIMERS
extern "C" int digat_debug_cf_timers(double* out16) {
    unsigned long long h[16];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_cf_timers), sizeof(h)) != hipSuccess) return DIGAT_ERR_LAUNCH;
    for (int k = 0; k < 16; ++k) { out16[k] = (double)h[k]; h[k] = 0; }
    return hipMemcpyToSymbol(HIP_SYMBOL(g_cf_timers), h, sizeof(h)) == hipSuccess ? DIGAT_OK : DIGAT_ERR_LAUNCH;
}
#endif
#ifdef DIGAT_GEMM_TIMERS
int digat_debug_gemm_timers(double* out8) {
    unsigned long long h[8];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_gemm_timers), sizeof(h)) != hipSuccess) return DIGAT_ERR_LAUNCH;
    for (int k = 0; k < 8; ++k) { out8[k] = (double)h[k]; h[k] = 0; }
    return hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_timers), h, sizeof(h)) == hipSuccess ? DIGAT_OK : DIGAT_ERR_LAUNCH;
}
#endif

// BASELINE configs[4], training half: the >= 2048-row GEMMs of the training path (projections, featureAffine, input
// gradients) with ONE bf16 product per fp32 product — plain bf16 mixed precision: fp32 master weights and activations, bf16
// matrix-core operands, fp32 accumulation — instead of the six of the fp32-grade split (the >= 2048-row weight gradients included: gemm_tn_bf16x6_kernel<true>).
static std::atomic<int> g_train_bf16{0};      // set once per training run (Trainer.__init__); read by every training GEMM
int digat_set_train_precision(int bf16) { return g_train_bf16.exchange(bf16 ? 1 : 0); }

int digat_linear_f32x3(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                       int M, int N, int K, void* wsplit, int format, void* stream) {
    if (!x || !w || !y || !wsplit || M < 0 || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    if (K % 8 || ldx % 4 || N % 80) return DIGAT_ERR_SHAPE;
    const int rcs = launch_split(w, w, w, N, 1, K, wsplit, (hipStream_t)stream, 0, format);
    if (rcs) return rcs;
    GemmArgs g = gemm_plain(x, ldx, w, b, y, ldy, M, N, K, 0);
    g.wsplit = (const unsigned short*)wsplit; g.format = format;
    if (g_train_bf16 && format != DIGAT_GEMM_F16F8C) g.x1_segs = 7;
    // M >= 2048: the strip-mined kernel; below: the skinny kernel on the same split image (gemm_skinny_split_kernel)
    return launch_gemm(g, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}

// digat_linear_f32x3 with what the encoder's row-list launches add: one or two weight segments (w1 non-NULL: y1 = x w1^T + b1,
// columns [nseg, 2 nseg) of the image), a row list, relu + residual (e0 non-NULL), the K3 addend on segment 1 (radd, one row per
// rows_per_b rows), m_dispatch and the request for ragged 240-column tiles (GemmArgs::ragged).  The tests' way to those launches.
int digat_linear_rows_f32x3(const float* x, int64_t ldx, const float* w0, const float* w1, const float* b0, const float* b1,
                            float* y0, float* y1, int64_t ldy, int M, int nseg, int K, void* wsplit, int format,
                            const int* rowidx, const int* nrows_dev, const float* e0, int64_t lde0,
                            const float* radd, int rows_per_b, int m_dispatch, int ragged, void* stream) {
    if (!x || !w0 || !y0 || !wsplit || M < 0 || nseg <= 0 || K <= 0 || (w1 && !y1) || (radd && (!w1 || rows_per_b <= 0))) return DIGAT_ERR_ARG;
    if (ragged < 0 || ragged > DIGAT_GEMM_RAGGED_ROWMAJOR || (rowidx && !nrows_dev)) return DIGAT_ERR_ARG;
    if (K % 8 || ldx % 4 || nseg % 80) return DIGAT_ERR_SHAPE;
    const int nsegs = w1 ? 2 : 1;
    const int rcs = launch_split(w0, w1 ? w1 : w0, w0, nseg, nsegs, K, wsplit, (hipStream_t)stream, 0, format);
    if (rcs) return rcs;
    GemmArgs g = gemm_plain(x, ldx, w0, b0, y0, ldy, M, nseg, K, 0);
    g.w[1] = w1; g.bias[1] = b1; g.y[1] = y1; g.nsegs = nsegs;
    g.wsplit = (const unsigned short*)wsplit; g.format = format;
    if (e0) { g.epi = EPI_RELU_RES; g.e0 = e0; g.lde0 = lde0; }
    g.radd = radd; g.radd_seg = 1; g.rows_per_b = rows_per_b;
    g.m_dispatch = m_dispatch; g.ragged = ragged;
    if (rowidx) {
        if (!gemm_takes_row_list(g)) return DIGAT_ERR_ARG;
        g.rowidx = rowidx; g.nrows_dev = nrows_dev;
    }
    return launch_gemm(g, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}

// Any launch launch_gemm takes, for the tests that hold every GEMM kernel alone to an fp64 product (tests/test_gemm_fp64_gpu.py):
// `args` is a GemmArgs (args_bytes guards a mirror of the struct that has drifted); wsplit_scratch non-NULL: the weight segments
// are split into it in args->format and the launch reads that image.  *kernel_out receives the GemmKernel gemm_plan chose, for
// refused launches too.  exec_rows, mtiles, ntiles and strips are launch_gemm's own: whatever the caller put there is dropped.
int digat_gemm_launch(const void* args, size_t args_bytes, int kind, void* wsplit_scratch, int* kernel_out, void* stream) {
    if (!args || !kernel_out || args_bytes != sizeof(GemmArgs) || (kind != DIGAT_KERNEL_PROJ && kind != DIGAT_KERNEL_LINEAR)) return DIGAT_ERR_ARG;
    GemmArgs g = *static_cast<const GemmArgs*>(args);
    *kernel_out = GEMM_NONE;
    if (g.nsegs < 1 || g.nsegs > 3 || g.M < 0 || g.nseg <= 0 || g.K <= 0 || g.k0 < 0 || g.k0 > g.K || !g.a0 || (g.k0 < g.K && !g.a1)) return DIGAT_ERR_ARG;
    for (int s = 0; s < g.nsegs; ++s) if (!g.w[s] || !g.y[s]) return DIGAT_ERR_ARG;
    if ((g.rowidx && !g.nrows_dev) || (g.radd && (g.rows_per_b <= 0 || g.radd_seg < 0 || g.radd_seg >= g.nsegs))) return DIGAT_ERR_ARG;
    g.exec_rows = nullptr; g.mtiles = g.ntiles = g.strips = 0;
    if (wsplit_scratch) g.wsplit = (const unsigned short*)wsplit_scratch;
    *kernel_out = gemm_plan(g, kind).kernel;
    if (wsplit_scratch) {
        const int rcs = launch_split(g.w[0], g.w[g.nsegs > 1 ? 1 : 0], g.w[g.nsegs > 2 ? 2 : 0], g.nseg, g.nsegs, g.K, wsplit_scratch,
                                     (hipStream_t)stream, 0, g.format);
        if (rcs) return rcs;
    }
    return launch_gemm(g, (hipStream_t)stream, kind);
}

// ---- a3 -----------------------------------------------------------------------------------------
// query, K^T query and the global context, [B,d] each
struct NewsCtxWs { float *qv, *kq, *glob; };
static NewsCtxWs news_ctx_carve(Arena& a, int B, int d) {
    const size_t bd = (size_t)B * d;
    return NewsCtxWs{a.take<float>(bd), a.take<float>(bd), a.take<float>(bd)};      // braces: taken left to right
}
size_t digat_news_ctx_workspace_bytes(int B, int N, int d) { (void)N; Arena a; news_ctx_carve(a, B, d); return a.used; }

int digat_news_ctx_fwd(const float* X, const uint8_t* mask, const float* Kc, const float* Qc, const float* bQc,
                       const float* Wg, const float* bg, const float* addend, float* out, int B, int N, int d,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!X || !mask || !Kc || !Qc || !Wg || !out || !workspace || B < 0 || N <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || N > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    Arena ar(workspace, workspace_bytes);
    const NewsCtxWs w = news_ctx_carve(ar, B, d);
    if (!ar.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    float *qv = w.qv, *kq = w.kq, *glob = w.glob;
    const long ldx = (long)N * d;      // node 0 of every row: the local context (graphEncoders.py:110)
    int rc;
    rc = launch_gemm(gemm_plain(X, ldx, Qc, bQc, qv, d, B, d, d, 0), st);           // Q(query)
    if (rc) return rc;
    rc = launch_gemm(gemm_plain(qv, d, Kc, nullptr, kq, d, B, d, d, 1), st);         // K^T q
    if (rc) return rc;
    rc = launch_pool(X, ldx, kq, mask, nullptr, glob, B, N, d, st);                  // global context
    if (rc) return rc;
    GemmArgs g = gemm_plain(X, ldx, Wg, bg, out, d, B, d, 2 * d, 0);                 // gate([local ; global])
    g.k0 = d; g.a1 = glob; g.lda1 = d;
    g.epi = EPI_GATE; g.e0 = X; g.lde0 = ldx; g.e1 = glob; g.lde1 = d; g.e2 = addend; g.lde2 = d;
    return launch_gemm(g, st);
}

// ---- a4 -----------------------------------------------------------------------------------------
// query and K^T query [B,d], the pooled topics T and featureAffine's T2 [B,C1,d]
struct UserCtxWs { float *qv, *kq, *T, *T2; };
static UserCtxWs user_ctx_carve(Arena& a, int B, int C1, int d) {
    const size_t bd = (size_t)B * d, bcd = (size_t)B * C1 * d;
    return UserCtxWs{a.take<float>(bd), a.take<float>(bd), a.take<float>(bcd), a.take<float>(bcd)};
}
size_t digat_user_ctx_workspace_bytes(int B, int U, int H, int C1, int d) { (void)U; (void)H; Arena a; user_ctx_carve(a, B, C1, d); return a.used; }

int digat_topic_pool_fwd(const float* Xu, const float* kq, const int64_t* cat_idx, float* out,
                         int B, int U, int H, int C1, int d, void* stream) {
    if (!Xu || !kq || !cat_idx || !out || B < 0 || H < 0 || U < H || C1 <= 0 || d <= 0) return DIGAT_ERR_ARG;
    return launch_topic(Xu, (long)U * d, kq, cat_idx, out, B, H, C1, d, (hipStream_t)stream);
}

// the launches of compute_user_graph_context on a carved workspace.  group (optional, [B]): row b's nodes live at
// Xu + group[b] * U * d (rows of one impression share them: digat_user_ctx_fwd_grouped); everything else is per row
static int user_ctx_run(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const int* group, const float* c_n,
                        const float* Ku, const float* Qu, const float* bQu, const float* Fa, const float* bFa,
                        const float* Kua, const float* Qua, const float* bQua, const float* addend, float* out,
                        int B, int U, int H, int C1, int d, const UserCtxWs& w, hipStream_t st) {
    float *qv = w.qv, *kq = w.kq, *T = w.T, *T2 = w.T2;
    int rc;
    // topic-level attention (:126-130)
    rc = launch_gemm(gemm_plain(c_n, d, Qu, bQu, qv, d, B, d, d, 0), st);
    if (rc) return rc;
    rc = launch_gemm(gemm_plain(qv, d, Ku, nullptr, kq, d, B, d, d, 1), st);
    if (rc) return rc;
    rc = launch_topic(Xu, (long)U * d, kq, cat_idx, T, B, H, C1, d, st, group);
    if (rc) return rc;
    // featureAffine + relu + residual (:131)
    GemmArgs g = gemm_plain(T, d, Fa, bFa, T2, d, B * C1, d, d, 0);
    g.epi = EPI_RELU_RES; g.e0 = T; g.lde0 = d;
    rc = launch_gemm(g, st);
    if (rc) return rc;
    // user-level attention (:133)
    rc = launch_gemm(gemm_plain(c_n, d, Qua, bQua, qv, d, B, d, d, 0), st);
    if (rc) return rc;
    rc = launch_gemm(gemm_plain(qv, d, Kua, nullptr, kq, d, B, d, d, 1), st);
    if (rc) return rc;
    return launch_pool(T2, (long)C1 * d, kq, cat_mask, addend, out, B, C1, d, st);
}

int digat_user_ctx_fwd(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n,
                       const float* Ku, const float* Qu, const float* bQu, const float* Fa, const float* bFa,
                       const float* Kua, const float* Qua, const float* bQua, const float* addend, float* out,
                       int B, int U, int H, int C1, int d, void* workspace, size_t workspace_bytes, void* stream) {
    if (!Xu || !cat_mask || !cat_idx || !c_n || !Ku || !Qu || !Fa || !Kua || !Qua || !out || !workspace)
        return DIGAT_ERR_ARG;
    if (B < 0 || H < 0 || U < H || C1 <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || C1 > DIGAT_MAX_NODES || H > TOPIC_MAX_H) return DIGAT_ERR_SHAPE;
    Arena ar(workspace, workspace_bytes);
    const UserCtxWs w = user_ctx_carve(ar, B, C1, d);
    if (!ar.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    return user_ctx_run(Xu, cat_mask, cat_idx, nullptr, c_n, Ku, Qu, bQu, Fa, bFa, Kua, Qua, bQua, addend, out, B, U, H, C1, d, w,
                        (hipStream_t)stream);
}

// ---- the inference launchers of the context stage alone (tests/test_hip_ctx_fp64.py): arguments checked, then forwarded one for one ----
int digat_pool_fwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, const float* addend, float* out,
                   int B, int n, int d, void* stream) {
    if (!feat || !kq || !mask || !out || B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (ld_b % 4) return DIGAT_ERR_SHAPE;
    return launch_pool(feat, (long)ld_b, kq, mask, addend, out, B, n, d, (hipStream_t)stream);
}

int digat_topic_pool_lists_fwd(const float* Xu, int64_t ld_b, const float* kq, const int64_t* cat_idx, const int32_t* row_group,
                               const uint8_t* live, int live_ld, const int32_t* hlast, float* out,
                               int B, int H, int C1, int d, void* stream) {
    if (!Xu || !kq || !cat_idx || !out || B < 0 || H < 0 || C1 <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if ((hlast && !live) || (live && live_ld < H)) return DIGAT_ERR_ARG;       // the kernels ignore hlast without live
    if (ld_b % 4) return DIGAT_ERR_SHAPE;
    return launch_topic(Xu, (long)ld_b, kq, cat_idx, out, B, H, C1, d, (hipStream_t)stream, row_group, live, live_ld, hlast);
}

int digat_user_ctx_fused_fwd(const float* Xu, int64_t ld_b, const int32_t* row_group, const uint8_t* live, int live_ld,
                             const int32_t* hlast, const float* kq_topic, const float* kq_user, const int64_t* cat_idx,
                             const uint8_t* cat_mask, const float* addend, float* out, const void* image, const float* bFa,
                             uint32_t* range_flag, int B, int H, int C1, int d, void* stream) {
    if (!Xu || !kq_topic || !kq_user || !cat_idx || !cat_mask || !out || !image || !bFa) return DIGAT_ERR_ARG;
    if (B < 0 || H < 0 || C1 <= 0 || d <= 0 || (hlast && !live) || (live && live_ld < H)) return DIGAT_ERR_ARG;
    if (!ctxfused_ok(H, C1, d) || ld_b % 4) return DIGAT_ERR_SHAPE;
    const CtxFusedArgs g{Xu, (long)ld_b, row_group, live, live_ld, hlast, kq_topic, kq_user, cat_idx, cat_mask, addend, out,
                         (const uint4*)image, bFa, range_flag, B, H, C1, d, sqrtf((float)d)};
    return launch_user_ctx_fused(g, (hipStream_t)stream);
}

// the initial user context alone: F x = ue Fa^T + user_ctx0_kernel (digat_ctx0.inc), the encoder's first context launch for launch
int digat_user_ctx0_fwd(const float* ue, const int32_t* row_group, int G, const float* kq_topic, const float* kq_user,
                        const uint8_t* cat_mask, const int64_t* cat_idx, const float* Fa, const float* bFa,
                        const void* fa_wsplit, int format, const float* addend, float* out, int B, int H, int C1, int d,
                        void* scratch, size_t scratch_bytes, void* stream) {
    if (!ue || !kq_topic || !kq_user || !cat_mask || !cat_idx || !Fa || !bFa || !out || !scratch) return DIGAT_ERR_ARG;
    if (B < 0 || H < 0 || C1 <= 0 || d <= 0 || (row_group && G <= 0)) return DIGAT_ERR_ARG;
    if (!ctx0_fits(H, C1, d)) return DIGAT_ERR_SHAPE;
    const long rows = row_group ? G : B;
    if (scratch_bytes < (size_t)rows * H * d * 4) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    return launch_user_ctx0(ue, rows, row_group, kq_topic, kq_user, cat_idx, cat_mask, Fa, bFa, fa_wsplit, format, nullptr, 0, addend, out,
                            (float*)scratch, B, H, C1, d, (hipStream_t)stream);
}

// ---- folded attention queries (inference): (K x).(Q c + b) = x.(K^T Q c + K^T b) ------------------
__global__ void __launch_bounds__(256) transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int d) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int y = by + r, x = bx + threadIdx.x;
        if (y < d && x < d) tile[r][threadIdx.x] = in[(long)y * d + x];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int y = bx + r, x = by + threadIdx.x;
        if (y < d && x < d) out[(long)y * d + x] = tile[threadIdx.x][r];
    }
}

size_t digat_fold_workspace_bytes(int d) { return 2 * align_up((size_t)d * d * 4, 256); }

int digat_fold_attention(const float* K, const float* Q, const float* bQ, float* Wf, float* bf, int d,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!K || !Q || !Wf || !bf || !workspace || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < digat_fold_workspace_bytes(d)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* Kt = (float*)workspace;
    float* Qt = (float*)((char*)workspace + align_up((size_t)d * d * 4, 256));
    const dim3 grid((d + 31) / 32, (d + 31) / 32), block(32, 8);
    hipLaunchKernelGGL(transpose_kernel, grid, block, 0, st, K, Kt, d);
    hipLaunchKernelGGL(transpose_kernel, grid, block, 0, st, Q, Qt, d);
    DIGAT_CHECK_LAUNCH();
    // Wf[c][i] = sum_o K[o][c] Q[o][i]  = linear(x = K^T [c,o], w = Q^T [i,o])
    int rc = launch_gemm(gemm_plain(Kt, d, Qt, nullptr, Wf, d, d, d, d, 0), st);
    if (rc) return rc;
    // bf[c] = sum_o K[o][c] bQ[o]       = linear(x = bQ [1,o], w = K^T [c,o])
    if (bQ) return launch_gemm(gemm_plain(bQ, d, Kt, nullptr, bf, d, 1, d, d, 0), st);
    return hipMemsetAsync(bf, 0, (size_t)d * 4, st) == hipSuccess ? DIGAT_OK : DIGAT_ERR_LAUNCH;
}

// ---- a5 -----------------------------------------------------------------------------------------
#include "digat_encoder.inc"

static double g_prof_last_live_fraction = -1.0;
double digat_profile_live_row_fraction(void) { return g_prof_last_live_fraction; }
static double g_prof_last_gemm_bytes[DIGAT_KERNEL_KINDS] = {0.0};
static double g_prof_last_part_ms[XATTN_PARTS] = {0.0}, g_prof_last_part_bytes[XATTN_PARTS] = {0.0};
static int g_prof_last_part_launches[XATTN_PARTS] = {0};
// After digat_profile_stop: the DIGAT_KERNEL_XATTN launches by kernel — [0] user graph layers >= 1 (row lists: twin kernel),
// [1] user graph layer 0 of grouped rows, [2] news graphs in LDS (n <= 16), [3] everything else; ms, algorithmic bytes, launches.
int digat_profile_xattn_parts(double* ms, double* bytes, int* launches) {
    for (int p = 0; p < XATTN_PARTS; ++p) {
        if (ms) ms[p] = g_prof_last_part_ms[p];
        if (bytes) bytes[p] = g_prof_last_part_bytes[p];
        if (launches) launches[p] = g_prof_last_part_launches[p];
    }
    return DIGAT_OK;
}
int digat_profile_gemm_bytes(double* bytes_per_kind) {
    if (!bytes_per_kind) return DIGAT_ERR_ARG;
    for (int k = 0; k < DIGAT_KERNEL_KINDS; ++k) bytes_per_kind[k] = g_prof_last_gemm_bytes[k];
    return DIGAT_OK;
}

// recording costs two hipEventRecord calls per launch on the host: a caller that wants per-kernel times over a long
// region without slowing it down samples it — pause(1) ... pause(0) around the steps it does not want recorded
int digat_profile_pause(int paused) {
    if (!g_prof.ev) return DIGAT_ERR_ARG;
    g_prof.enabled = paused ? 0 : 1;
    return DIGAT_OK;
}

// A one-thread kernel whose only purpose is to be visible in a kernel trace (rocprofv3 --kernel-trace): bench.py launches one
// at each end of its timed region, so that per-kernel averages of exactly that region can be cut out of the trace
// (tools/trace_region.py) and held against the library's own event timings.
__global__ void digat_region_marker_kernel(int id, int* sink) { if (sink && id < 0) *sink = id; }
int digat_profile_marker(int id, void* stream) {
    hipLaunchKernelGGL(digat_region_marker_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, id, (int*)nullptr);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// Which kernel kinds get their two events: every event pair is a pair of marker packets in the launch's queue and costs the
// overlapped encoder about 1 % of a step per 10 pairs; a measurement that only needs the dominant kernels says so.
int digat_profile_set_kinds(unsigned mask) {
    const unsigned prev = g_prof.kind_mask;
    g_prof.kind_mask = mask;
    return (int)prev;
}

int digat_profile_start(int max_launches) {
    if (max_launches <= 0) return DIGAT_ERR_ARG;
    if (g_prof.ev) return DIGAT_ERR_ARG;          // already running
    g_prof.ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * 2 * max_launches);
    g_prof.kind = (int*)malloc(sizeof(int) * max_launches);
    g_prof.work = (double*)malloc(sizeof(double) * max_launches);
    g_prof.bytes = (double*)malloc(sizeof(double) * max_launches);
    g_prof.part = (int*)malloc(sizeof(int) * max_launches);
    if (!g_prof.ev || !g_prof.kind || !g_prof.work || !g_prof.bytes || !g_prof.part) return DIGAT_ERR_ARG;
    for (int i = 0; i < 2 * max_launches; ++i)
        if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return DIGAT_ERR_LAUNCH;
    if (hipMalloc((void**)&g_prof.rows_dev, 16 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(g_prof.rows_dev, 0, 16 * sizeof(unsigned long long)) != hipSuccess) return DIGAT_ERR_LAUNCH;
    for (int k = 0; k < 16; ++k) { g_prof.flops_per_row[k] = 0.0; g_prof.rows_nominal[k] = 0.0; g_prof.bytes_per_row[k] = 0.0; }
    g_prof.cap = max_launches; g_prof.used = 0; g_prof.enabled = 1;
    return DIGAT_OK;
}

int digat_profile_stop(double* ms_per_kind, double* work_per_kind, int* launches_per_kind) {
    if (!g_prof.ev) return DIGAT_ERR_ARG;
    g_prof.enabled = 0;
    for (int k = 0; k < DIGAT_KERNEL_KINDS; ++k) {
        if (ms_per_kind) ms_per_kind[k] = 0;
        if (work_per_kind) work_per_kind[k] = 0;
        if (launches_per_kind) launches_per_kind[k] = 0;
        g_prof_last_gemm_bytes[k] = 0.0;
    }
    for (int p = 0; p < XATTN_PARTS; ++p) { g_prof_last_part_ms[p] = 0.0; g_prof_last_part_bytes[p] = 0.0; g_prof_last_part_launches[p] = 0; }
    int rc = DIGAT_OK;
    for (int i = 0; i < g_prof.used; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess ||
            hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) { rc = DIGAT_ERR_LAUNCH; continue; }
        const int k = g_prof.kind[i];
        if (ms_per_kind) ms_per_kind[k] += ms;
        if (work_per_kind) work_per_kind[k] += g_prof.work[i];
        if (launches_per_kind) launches_per_kind[k] += 1;
        g_prof_last_gemm_bytes[k] += g_prof.bytes[i];
        if (k == DIGAT_KERNEL_XATTN) {
            const int p = g_prof.part[i] >= 0 && g_prof.part[i] < XATTN_PARTS ? g_prof.part[i] : XPART_OTHER;
            g_prof_last_part_ms[p] += ms; g_prof_last_part_bytes[p] += g_prof.work[i]; g_prof_last_part_launches[p] += 1;
        }
    }
    g_prof_last_live_fraction = -1.0;
    if (g_prof.rows_dev) {
        unsigned long long rows[16];
        if (hipMemcpy(rows, g_prof.rows_dev, sizeof(rows), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int k = 0; k < DIGAT_KERNEL_KINDS; ++k) {
                if (work_per_kind) work_per_kind[k] += (double)rows[k] * g_prof.flops_per_row[k];
                if (k == DIGAT_KERNEL_PROJ || k == DIGAT_KERNEL_LINEAR) g_prof_last_gemm_bytes[k] += (double)rows[k] * g_prof.bytes_per_row[k];
            }
            for (int p = 0; p < XATTN_PARTS; ++p) {         // Eq. 8 launches on live-row lists: BYTES counted on the device
                if (work_per_kind) work_per_kind[DIGAT_KERNEL_XATTN] += (double)rows[8 + p];
                g_prof_last_part_bytes[p] += (double)rows[8 + p];
            }
            if (g_prof.rows_nominal[DIGAT_KERNEL_PROJ] > 0)
                g_prof_last_live_fraction = (double)rows[DIGAT_KERNEL_PROJ] / g_prof.rows_nominal[DIGAT_KERNEL_PROJ];
        }
        (void)hipFree(g_prof.rows_dev);
        g_prof.rows_dev = nullptr;
    }
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    free(g_prof.ev); free(g_prof.kind); free(g_prof.work); free(g_prof.bytes); free(g_prof.part);
    g_prof.ev = nullptr; g_prof.kind = nullptr; g_prof.work = nullptr; g_prof.bytes = nullptr; g_prof.part = nullptr; g_prof.cap = g_prof.used = 0;
    return rc;
}

int digat_row_logits(const float* news_ctx, const float* user_ctx, float* logits, int B, int d, void* stream) {
    if (!news_ctx || !user_ctx || !logits || B < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    hipLaunchKernelGGL(row_logits_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, news_ctx, user_ctx,
                       logits, B, d);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"

#include "digat_train.inc"
#include "digat_train_abi.inc"
#include "digat_eval.inc"
#include "digat_topk.inc"
#include "digat_news.inc"
#include "digat_news_train.inc"
#include "digat_mhsa.inc"
#include "digat_cnn.inc"
#include "digat_gat.inc"
#include "digat_sag.inc"
#include "digat_user_graph.inc"
#include "digat_train_input.inc"
#include "digat_ablation.inc"
#include "digat_dot_topk.inc"
#include "digat_shortlist.inc"
#include "digat_qdot.inc"
#include "digat_dot_rank.inc"
#include "digat_pool_softmax.inc"
#include "digat_list_softmax.inc"
#include "digat_list_pairwise.inc"
#include "digat_mmr.inc"
#include "digat_listq.inc"
#include "digat_bootstrap.inc"
#include "digat_calibrate.inc"
#include "digat_pl_sample.inc"
#include "digat_pl_expect.inc"
#include "digat_list_pl.inc"
#include "digat_list_plrank.inc"
#include "digat_rerank.inc"
#include "digat_capped.inc"
