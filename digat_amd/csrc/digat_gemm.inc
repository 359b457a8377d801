// digat_gemm.inc — the GEMMs of the path: fp32 MFMA, strip-mined bf16x6 (LDS-DMA), skinny [B,d] linears, and launch_gemm, which runs
// every GEMM the way gemm_plan (digat_gemm_plan.h) decides
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

#include "digat_gemm_plan.h"         // GemmArgs, the EPI_* epilogues and gemm_plan: which kernel below runs a launch

// =================================================================================================
// 1. fp32 MFMA GEMM:  y_s[M, nseg] = A[M,K] @ w_s[nseg,K]^T (+ bias_s), s < nsegs, fused epilogue
// =================================================================================================
// LDS image: float4 tile[k4][row ^ k4]  (k4 = 4-float column group of the 32-deep K tile).
// A lane quarter q reads column group 4*kk+q with ds_read_b128 and feeds element s of it to the
// s-th MFMA k-step (A and B use the same k assignment, so the sum over k is complete); the XOR of
// the low row bits makes both that read and the staging ds_write_b128 bank-conflict free.
// TAG only names the instantiation (0 = nn.Linear, 1 = the Eq. 8 node projections) so that profiles
// list the projection launches under their own kernel symbol.
template <int BM, int BN, int WAVES_M, int WAVES_N, int PF, int TAG>
__global__ void __launch_bounds__(256) gemm_f32_kernel(const GemmArgs g) {
    constexpr int BK4 = 8;
    constexpr int MT = BM / WAVES_M / 16;
    constexpr int NT = BN / WAVES_N / 16;
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
    static_assert(BM % (WAVES_M * 16) == 0 && BN % (WAVES_N * 16) == 0, "wave tile");
    static_assert(BM % 8 == 0 && BN % 8 == 0, "xor swizzle needs 8-row groups");
    constexpr int A_PER_T = (BM * BK4 + 255) / 256;
    constexpr int B_PER_T = (BN * BK4 + 255) / 256;
    __shared__ float4 As[BK4 * BM];
    __shared__ float4 Bs[BK4 * BN];

    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give each XCD a
    // contiguous run of tiles; consecutive tiles share the same rows of A (its L2 keeps them).
    const int total = g.mtiles * g.ntiles;
    const int chunk = (total + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (tile >= total) return;
    const int mtile = tile / g.ntiles, ntile = tile - mtile * g.ntiles;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int m0 = mtile * BM, n0 = ntile * BN;
    const int Ntot = g.nseg * g.nsegs;
    // one weight segment per tile (launch_gemm guarantees tiles never straddle segments), chosen with
    // scalar arithmetic: a per-lane select of g.w[] makes hipcc fetch the pointer from kernarg memory
    // with a vector load and a vmcnt(0) in front of every tile load
    const int seg = n0 / g.nseg;
    const int nbase = n0 - seg * g.nseg;          // column of this tile inside its segment
    const float* const wseg = g.w[seg];
    const int ktiles = ((g.K >> 2) + BK4 - 1) / BK4;

    // PF register sets: PF = 1 overlaps one tile's loads with the MFMAs of the previous tile (enough when
    // a tile carries >= 2k MFMA cycles); PF = 2 keeps two tiles in flight for the small-M shapes whose
    // per-tile MFMA time is far below the load latency
    float4 ra0[A_PER_T], rb0[B_PER_T], ra1[PF == 2 ? A_PER_T : 1], rb1[PF == 2 ? B_PER_T : 1];

    auto load_tiles = [&](int kt, float4* ra, float4* rb) {
#pragma unroll
        for (int u = 0; u < A_PER_T; ++u) {
            const int i = tid + u * 256;
            float4 v = f4_zero();
            if (i < BM * BK4) {
                const int r = i / BK4, c4 = i % BK4;
                const int gm = m0 + r, k = (kt * BK4 + c4) * 4;
                if (gm < g.M && k < g.K) {
                    const float* p = (k < g.k0) ? g.a0 + (long)gm * g.lda0 + k
                                                : g.a1 + (long)gm * g.lda1 + (k - g.k0);
                    v = *reinterpret_cast<const float4*>(p);
                }
            }
            ra[u] = v;
        }
#pragma unroll
        for (int u = 0; u < B_PER_T; ++u) {
            const int i = tid + u * 256;
            float4 v = f4_zero();
            if (i < BN * BK4) {
                const int r = g.transW ? i % BN : i / BK4;
                const int c4 = g.transW ? i / BN : i % BK4;
                const int gn = n0 + r, k = (kt * BK4 + c4) * 4;
                const int nn = nbase + r;
                if (nn < g.nseg && gn < Ntot && k < g.K) {
                    if (!g.transW) {
                        v = *reinterpret_cast<const float4*>(wseg + (long)nn * g.K + k);
                    } else {
                        const float* p = wseg + (long)k * g.nseg + nn;
                        v = make_float4(p[0], p[g.nseg], p[2 * (long)g.nseg], p[3 * (long)g.nseg]);
                    }
                }
            }
            rb[u] = v;
        }
    };
    auto store_tiles = [&](const float4* ra, const float4* rb) {
#pragma unroll
        for (int u = 0; u < A_PER_T; ++u) {
            const int i = tid + u * 256;
            if (i < BM * BK4) {
                const int r = i / BK4, c4 = i % BK4;
                As[c4 * BM + (r ^ c4)] = ra[u];
            }
        }
#pragma unroll
        for (int u = 0; u < B_PER_T; ++u) {
            const int i = tid + u * 256;
            if (i < BN * BK4) {
                const int r = g.transW ? i % BN : i / BK4;
                const int c4 = g.transW ? i / BN : i % BK4;
                Bs[c4 * BN + (r ^ c4)] = rb[u];
            }
        }
    };

    v4f acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (v4f){0.f, 0.f, 0.f, 0.f};

    auto compute_tile = [&]() {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int k4 = kk * 4 + (lane >> 4);
            float4 af[MT], bf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int r = wm * (MT * 16) + mt * 16 + (lane & 15);
                af[mt] = As[k4 * BM + (r ^ k4)];
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int r = wn * (NT * 16) + nt * 16 + (lane & 15);
                bf[nt] = Bs[k4 * BN + (r ^ k4)];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            f4_comp(af[mt], s), f4_comp(bf[nt], s), acc[mt][nt], 0, 0, 0);
        }
    };

    if (PF == 1) {
        load_tiles(0, ra0, rb0);
        store_tiles(ra0, rb0);
        __syncthreads();
        for (int kt = 0; kt < ktiles; ++kt) {
            const bool more = kt + 1 < ktiles;
            if (more) load_tiles(kt + 1, ra0, rb0);          // global loads fly under this tile's MFMAs
            compute_tile();
            __syncthreads();
            if (more) {
                store_tiles(ra0, rb0);
                __syncthreads();
            }
        }
    } else {
        load_tiles(0, ra0, rb0);
        if (ktiles > 1) load_tiles(1, ra1, rb1);
        store_tiles(ra0, rb0);
        __syncthreads();
        for (int kt = 0; kt < ktiles; kt += 2) {
            // tile kt is in LDS, set 1 holds kt+1 (in flight), set 0 is free
            if (kt + 2 < ktiles) load_tiles(kt + 2, ra0, rb0);
            compute_tile();
            __syncthreads();
            if (kt + 1 >= ktiles) break;
            store_tiles(ra1, rb1);
            __syncthreads();
            // tile kt+1 is in LDS, set 0 holds kt+2 (in flight), set 1 is free
            if (kt + 3 < ktiles) load_tiles(kt + 3, ra1, rb1);
            compute_tile();
            __syncthreads();
            if (kt + 2 < ktiles) {
                store_tiles(ra0, rb0);
                __syncthreads();
            }
        }
    }

    // epilogue: D[row = 4*(lane>>4) + r][col = lane&15]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int nn = nbase + wn * (NT * 16) + nt * 16 + (lane & 15);
            if (nn >= g.nseg) continue;
            const float* bp = g.bias[seg];
            float* yp = g.y[seg];
            const float bv = bp ? bp[nn] : 0.f;
            const float* radd = seg == g.radd_seg ? g.radd : nullptr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wm * (MT * 16) + mt * 16 + (lane >> 4) * 4 + r;
                if (gm >= g.M) continue;
                float v = acc[mt][nt][r] + bv;
                if (radd) v = radd[(long)(gm / g.rows_per_b) * g.nseg + nn] + v;
                if (g.epi == EPI_RELU_RES) {
                    v = fmaxf(v, 0.f) + g.e0[(long)gm * g.lde0 + nn];
                } else if (g.epi == EPI_GATE) {
                    const float gate = 1.f / (1.f + expf(-v));
                    const float loc = g.e0[(long)gm * g.lde0 + nn];
                    const float glo = g.e1[(long)gm * g.lde1 + nn];
                    v = gate * loc + (1.f - gate) * glo;
                    if (g.e2) v = g.e2[(long)gm * g.lde2 + nn] + v;
                } else if (g.epi == EPI_ACCUM) {
                    v = yp[(long)gm * g.ldy + nn] + v;
                }
                yp[(long)gm * g.ldy + nn] = v;
            }
        }
    }
}

// =================================================================================================
// 1b. "bf16x6" GEMM: exact-fp32-quality product on the bf16 matrix cores
// =================================================================================================
// Every fp32 operand is split into three bf16 pieces (x = x1 + x2 + x3 exactly: 3 x 8 mantissa bits);
// the six partial products whose weight is >= 2^-16 (x1w1, x1w2, x2w1, x1w3, x2w2, x3w1) are summed in
// the fp32 MFMA accumulator (v_mfma_f32_16x16x32_bf16).  Dropped terms are <= 3 * 2^-24 relative, i.e.
// the result is as accurate as an fp32 fma chain (measured: mean error 0.6x that of an fp32 GEMM) at
// 6/16 of the fp32-MFMA cost.  Weights are split once per weight version (split_weights_tiled_kernel),
// activations while they pass through the kernel.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Exact 3-way split by TRUNCATION: x1 = top 16 bits of v, r1 = v - x1 (exact, <= 16 significant bits),
// x2 = top 16 bits of r1, x3 = r1 - x2 (<= 8 significant bits, already a bf16).  Round-to-nearest is not
// needed for exactness and costs 2x the VALU work (measured: 217 vs ~110 VALU instructions per K tile).
struct Split3f { float a, b, c; };           // each value has its low 16 bits clear
__device__ __forceinline__ Split3f split3f(float v) {
    Split3f o;
    o.a = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & 0xffff0000u);
    const float r1 = v - o.a;
    o.b = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r1) & 0xffff0000u);
    o.c = r1 - o.b;
    return o;
}
// two bf16 (upper halves of lo and hi) packed into one dword: [hi16(lo) | hi16(hi) << 16], one v_perm_b32
// two floats -> two bf16 (round to nearest even; finite inputs), low half = the first
__device__ __forceinline__ unsigned pack_bf16_rne(float lo, float hi) {
    unsigned a = __builtin_bit_cast(unsigned, lo), b = __builtin_bit_cast(unsigned, hi);
    a += 0x7fffu + ((a >> 16) & 1u);
    b += 0x7fffu + ((b >> 16) & 1u);
    return (a >> 16) | (b & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack_hi16(float lo, float hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, hi), __builtin_bit_cast(unsigned, lo), 0x07060302u);
}
constexpr float F16_WEIGHT_SCALE = 1024.f;      // fp16x3 format: the split weights carry this factor ...
constexpr float F16_ACT_SCALE = 16.f;           // ... and the activations, split in the kernel, this one
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
// two floats -> two fp16 (round toward zero) in one dword, low half = the first; and back
__device__ __forceinline__ unsigned pack_half_rtz(float lo, float hi) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(lo, hi)); }
__device__ __forceinline__ unsigned half_bits_rtz(float v) { return pack_half_rtz(v, 0.f) & 0xffffu; }
__device__ __forceinline__ float half_bits_to_float(unsigned bits) {
    const fp16x2 h = __builtin_bit_cast(fp16x2, bits);
    return (float)h[0];
}
struct Split3 { unsigned short a, b, c; };
__device__ __forceinline__ Split3 split3(float v) {
    const Split3f f = split3f(v);
    Split3 o;
    o.a = (unsigned short)(__builtin_bit_cast(unsigned, f.a) >> 16);
    o.b = (unsigned short)(__builtin_bit_cast(unsigned, f.b) >> 16);
    o.c = (unsigned short)(__builtin_bit_cast(unsigned, f.c) >> 16);
    return o;
}

// Kernel design (what the counters asked for: a first version with 128x80 tiles and register-staged operands
// spent 3.8 non-MFMA vector instructions per MFMA — operand split, address arithmetic, bounds checks — while a
// 16-cycle MFMA leaves issue room for two; its dword epilogue cost another third of the run time):
//  * the four waves of a workgroup are stacked along M; a wave keeps its 32 rows of A for THREE 80-column
//    strips of the weights (wave tile 32 x 240, 120 accumulator registers), so the split is paid once per
//    180 MFMAs;
//  * the split weights are stored as ready-made LDS images, one per (80-column strip, 32-deep K tile):
//    [plane][k group][row] 16-byte slots, K zero-padded to 32.  An image is 15 KB and goes global -> LDS by
//    LDS-DMA (no registers, no address arithmetic, no bounds checks) into a ring of three: two images are in
//    flight behind the one the 60 MFMAs of a step read; the fp32 A tile (128 x 32) takes the same road once
//    per K tile and is split from LDS in the shadow of strips 1 and 2.  Every global read being a DMA, the
//    vector-memory queue is counted by hand: one "s_waitcnt vmcnt(4)" + one s_barrier per step;
//  * the weights are the MFMA's ROW operand and the activations its COLUMN operand, so a lane ends with four
//    consecutive output columns of one row: float4 bias/residual loads and float4 stores;
//  * tiles may span weight segments (bias/output picked per strip; segments are multiples of 80 columns).
// Measured (M=68 608, N=1 200, K=400): 373 us = 177 TFLOP/s fp32-equivalent = 1.06 PFLOP/s bf16; the 128x80
// version ran 467 us, the exact fp32-MFMA kernel (single segment) 770 us, rocBLAS fp32 addmm 680 us.
constexpr int WS_SLOTS = 960;            // 16-byte slots of one strip image: 3 planes x 4 k groups x 80 rows

// transposed != 0 (one segment): the weight is stored [K, nseg] and used as its transpose (dX = dY @ W); 2: three such matrices of
// K / 3 rows each, given separately, stacked along K (dX = [dh | dP | dQ] @ [W; F1; F2] without concatenating the weights)
// planes = 3: the three bf16 pieces; planes = 2: two fp16 pieces (hi = v truncated to fp16, lo = the remainder truncated: 22
// significant bits; "fp16x3", see gemm_bf16x6s_kernel<., true, ., .>), images of 2 x 320 slots
__device__ __forceinline__ void split_weights_tiled_body(const float* w0, const float* w1, const float* w2,
                                                         int nseg, int nsegs, int K, unsigned short* out, int transposed, int planes) {
    const int KT = (K + 31) >> 5, Kp = KT * 32;
    const int Ntot = nseg * nsegs;
    const int strips = (Ntot + 79) / 80;
    const long total = (long)strips * 80 * Kp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / Kp), k = (int)(i - (long)n * Kp);
        float v = 0.f;
        if (n < Ntot && k < K) {
            const int seg = n / nseg;
            const float* w = seg == 0 ? w0 : (seg == 1 ? w1 : w2);
            if (transposed == 2) {           // [w0; w1; w2] stacked along K, each [K / 3, nseg], used as the transpose of the stack
                const int kseg = K / 3, ks = k / kseg;
                const float* wk = ks == 0 ? w0 : (ks == 1 ? w1 : w2);
                v = wk[(long)(k - ks * kseg) * nseg + n];
            } else
            v = transposed ? w[(long)k * nseg + n] : w[(long)(n - seg * nseg) * K + k];
        }
        const int strip = n / 80, r = n - strip * 80, kt = k >> 5, kq = (k >> 3) & 3, e = k & 7;
        const long base = ((long)strip * KT + kt) * (planes * 320) * 8;
        if (planes == 3) {
            const Split3 sp = split3(v);
            out[base + ((0 * 4 + kq) * 80 + r) * 8 + e] = sp.a;
            out[base + ((1 * 4 + kq) * 80 + r) * 8 + e] = sp.b;
            out[base + ((2 * 4 + kq) * 80 + r) * 8 + e] = sp.c;
        } else {
            // weights are split once: round to nearest for both pieces; scaled by 2^10 (exact; undone in the GEMM's epilogue) so
            // that the low piece of a weight of ordinary size (|w| ~ 0.05: 2e-5) is a NORMAL fp16 — as a subnormal its 2^-24
            // quantum was the product's dominant error; |w| < 63 keeps the high piece finite
            const float vs = v * F16_WEIGHT_SCALE;
            const _Float16 h = (_Float16)vs;
            const _Float16 l = (_Float16)(vs - (float)h);
            const unsigned hi = __builtin_bit_cast(unsigned short, h), lo = __builtin_bit_cast(unsigned short, l);
            out[base + ((0 * 4 + kq) * 80 + r) * 8 + e] = (unsigned short)hi;
            out[base + ((1 * 4 + kq) * 80 + r) * 8 + e] = (unsigned short)lo;
        }
    }
}
__global__ void __launch_bounds__(256) split_weights_tiled_kernel(const float* w0, const float* w1, const float* w2,
                                                                  int nseg, int nsegs, int K, unsigned short* out, int transposed, int planes) {
    split_weights_tiled_body(w0, w1, w2, nseg, nsegs, K, out, transposed, planes);
}
// several bf16x6 images in one launch (digat_split_jobs: a training step's weights): blockIdx.y = job
constexpr int SPLIT_MAX_JOBS = 24;
struct SplitJobDev { const float *w0, *w1, *w2; unsigned short* out; int nseg, nsegs, K, transposed; };
struct SplitJobsDev { SplitJobDev j[SPLIT_MAX_JOBS]; };
// the bf16x6 image a 16-byte slot at a time: a thread owns the 8 consecutive k of one weight row's slot — eight reads (32
// contiguous bytes, or eight rows of the transposed layouts with the threads of a wave on consecutive columns) and three 16-byte
// stores, one per piece plane, where the element-wise body does six 2-byte stores per element (46 -> ~20 us for a step's 14 images)
__device__ __forceinline__ void split_weights_slots_body(const float* w0, const float* w1, const float* w2, int nseg, int nsegs, int K,
                                                         unsigned short* out, int transposed) {
    const int KT = (K + 31) >> 5;
    const int Ntot = nseg * nsegs;
    const int strips = (Ntot + 79) / 80;
    const int k8s = KT * 4;                                    // slots per weight row (K zero-padded to 32)
    const long total = (long)strips * 80 * k8s;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        // transposed layouts: consecutive threads take consecutive rows n (their reads are then contiguous); else consecutive slots
        const int n = transposed ? (int)(i % (strips * 80)) : (int)(i / k8s);
        const int k8 = transposed ? (int)(i / (strips * 80)) : (int)(i - (long)n * k8s);
        const int k0 = k8 * 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        if (n < Ntot) {
            if (!transposed) {
                const int seg = n / nseg;
                const float* row = (seg == 0 ? w0 : (seg == 1 ? w1 : w2)) + (long)(n - seg * nseg) * K;
                if (k0 + 8 <= K && ((uintptr_t)(row + k0) & 15) == 0) {
                    const float4 a = *reinterpret_cast<const float4*>(row + k0), b = *reinterpret_cast<const float4*>(row + k0 + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (k0 + e < K) v[e] = row[k0 + e];
                }
            } else if (transposed == 2) {
                const int kseg = K / 3;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + e;
                    if (k < K) {
                        const int ks = k / kseg;
                        v[e] = (ks == 0 ? w0 : (ks == 1 ? w1 : w2))[(long)(k - ks * kseg) * nseg + n];
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) if (k0 + e < K) v[e] = w0[(long)(k0 + e) * nseg + n];
            }
        }
        const int strip = n / 80, r = n - strip * 80, kt = k8 >> 2, kq = k8 & 3;
        const long base = ((long)strip * KT + kt) * (3 * 320) * 8;
        unsigned pa[4], pb[4], pc[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const Split3 s0 = split3(v[2 * h]), s1 = split3(v[2 * h + 1]);
            pa[h] = (unsigned)s0.a | ((unsigned)s1.a << 16);
            pb[h] = (unsigned)s0.b | ((unsigned)s1.b << 16);
            pc[h] = (unsigned)s0.c | ((unsigned)s1.c << 16);
        }
        *reinterpret_cast<uint4*>(out + base + ((0 * 4 + kq) * 80 + r) * 8) = make_uint4(pa[0], pa[1], pa[2], pa[3]);
        *reinterpret_cast<uint4*>(out + base + ((1 * 4 + kq) * 80 + r) * 8) = make_uint4(pb[0], pb[1], pb[2], pb[3]);
        *reinterpret_cast<uint4*>(out + base + ((2 * 4 + kq) * 80 + r) * 8) = make_uint4(pc[0], pc[1], pc[2], pc[3]);
    }
}
__global__ void __launch_bounds__(256) split_weights_jobs_kernel(const SplitJobsDev a) {
    const SplitJobDev& j = a.j[blockIdx.y];
    split_weights_slots_body(j.w0, j.w1, j.w2, j.nseg, j.nsegs, j.K, j.out, j.transposed);
}

// F16 ("fp16x3"): the operands as TWO fp16 pieces (hi = truncation to fp16, lo = the remainder: 22 significant bits) and the
// three products hi.hi, hi.lo, lo.hi on v_mfma_f32_16x16x32_f16 — half the matrix-core work of the six bf16 products.  Relative
// With the weights scaled by 2^10 and the activations by 2^4 (powers of two: exact, undone in the epilogue) the low pieces of
// operands of ordinary size are normal fp16 numbers; measured against fp64 (tests/test_hip_lowprec.py) the mean error is 0.75x
// and the largest 0.7x an fp32 fma chain's.  Range: |w| < 63, |x| < 4094 (beyond: inf); pieces below 6e-5 after scaling are
// subnormals (an absolute floor of 2^-24 per term).  digat_set_gemm_format(1) / env DIGAT_GEMM_F16X3; the C ABI's default is bf16x6.
#ifdef DIGAT_GEMM_TIMERS
// experiment builds only (tools/exp/gemm_lab.py): cycles the sampled waves spend waiting for the DMA queue, in the barrier, and
// in the rest of a step; [3] = steps sampled, [5] = epilogue, [6] = waves, [7] = whole kernel
__device__ unsigned long long g_gemm_timers[8];
#define GT_NOW() __builtin_amdgcn_s_memtime()
#else
#define GT_NOW() 0ull
#endif
// The instantiations gemm_plan launches: NSUB = 3 (240-column tiles) or 1; F16 (fp16x3) or bf16x6; MT = 2 (128-row tiles) or 1
// (64-row tiles for launches that would leave the chip under-filled); FULL (round 5, fp16x3 with 240-column tiles): every segment
// of the launch takes all its products (x1_segs == x3_segs == 0: what inference launches ask for) — the per-strip product
// selector becomes a compile-time constant, the wave-uniform branch around each 16-column block's extra products (five per strip)
// goes, and a strip's 30 MFMAs + 10 fragment reads are ONE basic block for the scheduler.  The variants measured and rejected
// (pre-split A rows, the spread DMA issue, 64-row "fat" wave tiles) are in docs/REJECTED.md.
// RAG (ragged 240-column tiles, GemmPlan::ragged): the last column tile of a launch whose N is no multiple of 240 has ns = 1 or 2
// strips; ns is wave-uniform and drives the step count, the ring indices and where the A tile is issued and split.  The steps
// themselves (DMA pieces, MFMA order, split) are those of the full-width tile, so every output element keeps its product chain
// — and the launches without ragged tiles keep their code: RAG = false folds every ns to NSUB.
template <int NSUB, bool F16, int MT, bool FULL, bool RAG = false>      // MT: 16-row blocks per wave (wave tile 16 MT x 80 NSUB)
__global__ void __launch_bounds__(256, MT == 1 ? 3 : 2) gemm_bf16x6s_kernel(const GemmArgs g) {
    static_assert(MT == 1 || MT == 2, "wave tiles of 16 or 32 rows");
    static_assert(!RAG || (NSUB == 3 && MT == 2), "ragged tiles: 128 rows x up to three strips");
    constexpr int NT = 5;
    constexpr int WROWS = 16 * MT, TROWS = 4 * WROWS;      // rows of a wave tile / of the workgroup's tile (four waves stacked along M)
    constexpr int APW = 2 * MT;                             // 1 KB DMA pieces (8 rows x 32 k fp32) of the A tile per wave
    // One-strip tiles (NSUB == 1: featureAffine, N not a multiple of 240): the A tile travels ABUF - 1 steps ahead, the strip
    // images RING - 1, and the operand split of step k + 1 runs in the shadow of step k's MFMAs (it used to open every step:
    // 16.0 -> 14.7 us on 7 000 x 400 x 400).  Deeper rings measured no better (3 / 3: 16.2 us; 5 / 4 at one workgroup per CU:
    // 24.8 us): the phase timers show these launches waiting 7 % of a step — what is left is launch, prologue and epilogue.
    constexpr int RING = 3;                   // strip images in LDS: RING - 1 in flight behind the one being read
    constexpr int ABUF = NSUB == 1 || RAG ? 2 : 1;   // fp32 A tiles (128 rows x 32 k) in LDS (three 15 KB bf16 planes per image leave
                                              // room for two: 77 KB, two workgroups per CU); ragged: a one-strip tile needs the second
    constexpr int PL = F16 ? 2 : 3;          // operand pieces
    constexpr int WS_SLOTS = PL * 320;       // 16-byte slots of one strip image (shadows the bf16 constant)
    constexpr int PIECES = WS_SLOTS / 64;    // 1 KB DMA pieces of an image: 15 / 10
    constexpr int IMG_I = (PIECES + 3) / 4;  // DMA instructions per wave and image: 4 / 3
    __shared__ uint4 Bs[RING][WS_SLOTS];
    __shared__ uint4 As[ABUF][TROWS * 8];    // slot r*8 + (c4 ^ ((r>>1)&7)): conflict-free 32-byte row pieces

    // With a row list (rowidx / *nrows_dev, written on the device) the grid is sized for all M rows and the tile
    // count comes from the live row count, so the live tiles still spread over the 8 XCDs evenly.
    const int Mv = g.nrows_dev ? __builtin_amdgcn_readfirstlane(*g.nrows_dev) : g.M;      // scalar: the tile index and every base address that follows from it stay in SGPRs
    if (g.exec_rows && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(g.exec_rows, (unsigned long long)Mv);
    int mtile, ntile;
    if (!RAG || g.ragged == DIGAT_GEMM_RAGGED_ROWMAJOR) {
        const int total = ((Mv + TROWS - 1) / TROWS) * g.ntiles;
        const int chunk = (total + 7) >> 3;
        if ((int)(blockIdx.x >> 3) >= chunk) return;
        const int tile = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
        if (tile >= total) return;
        mtile = tile / g.ntiles; ntile = tile - mtile * g.ntiles;
    } else {
        // Long tiles first: an XCD's chunk is its share of the full-width tiles (row-tile-major) followed by its share of the short
        // last-column tiles, so the workgroups that start late — behind the first wave of two per CU — are the short ones.
        const int mlive = (Mv + TROWS - 1) / TROWS, nfw = g.ntiles - 1;
        const int nfull = mlive * nfw, cf = (nfull + 7) >> 3, cs = (mlive + 7) >> 3;
        const int xcd = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
        if (j < cf) {
            const int t = xcd * cf + j;
            if (t >= nfull) return;
            mtile = t / nfw; ntile = t - mtile * nfw;
        } else {
            const int t = xcd * cs + (j - cf);
            if (j - cf >= cs || t >= mlive) return;
            mtile = t; ntile = nfw;
        }
    }
    // strips of this column tile: wave-uniform (SGPR); without ragged tiles the constant NSUB
    const int ns = RAG ? __builtin_amdgcn_readfirstlane(g.strips - NSUB * ntile < NSUB ? g.strips - NSUB * ntile : NSUB) : NSUB;

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int kg = lane >> 4, lr = lane & 15;
    const int m0 = mtile * TROWS;
    const int strip0 = ntile * NSUB;
#ifdef DIGAT_GEMM_TIMERS
    const unsigned long long gt_enter = GT_NOW();
    unsigned long long gt_wait = 0, gt_bar = 0, gt_body = 0, gt_steps = 0, gt_last = 0;
#endif
    const int KT = (g.K + 31) >> 5;
    const int nsteps = KT * ns;
    const unsigned ldsB = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Bs[0][0];
    const unsigned ldsA = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&As[0][0];
    const char* const wimg = reinterpret_cast<const char*>(g.wsplit);      // wave-uniform: the pieces' sources are (scalar base) + lane x 16
    const unsigned wlane = (unsigned)lane * 16u;
    const int wu = __builtin_amdgcn_readfirstlane(wm);          // the DMA's LDS address goes through M0: provably uniform

    // Every global read of the loop is an LDS-DMA, four wave-instructions per wave and image, so the vector-memory
    // queue holds whole images in issue order and "s_waitcnt vmcnt(4)" means "all but the youngest image".
    auto issue_b_at = [&](int kt, int s, int buf) {      // strip image of step (kt, s) -> Bs[buf]; 15 instructions + 1 repeat
        const char* src = wimg + ((long)(strip0 + s) * KT + kt) * (WS_SLOTS * 16);
#pragma unroll
        for (int k = 0; k < IMG_I; ++k) {
            int q = wu + 4 * k;
            q = q < PIECES ? q : PIECES - 1;                     // the last piece is copied more than once: IMG_I per wave, always
            lds_dma16_s(src + q * 1024, wlane, ldsB + (unsigned)((buf * WS_SLOTS + q * 64) * 16));
        }
    };
    auto issue_b = [&](int step) {           // full-width tiles: step = kt * NSUB + s, ring slot step % RING
        const int kt = step / NSUB;
        issue_b_at(kt, step - kt * NSUB, step % RING);
    };
    // ragged tiles: the image that goes out next — two steps ahead of the one being read — as (K tile, strip, ring slot),
    // carried along in SGPRs instead of divided out of the step at every issue
    int nb_kt = 0, nb_s = 0, nb_buf = 0;
    auto issue_b_next = [&]() {
        issue_b_at(nb_kt, nb_s, nb_buf);
        if (++nb_s == ns) { nb_s = 0; ++nb_kt; }
        nb_buf = nb_buf == RING - 1 ? 0 : nb_buf + 1;
    };
    // this lane's source of A-tile piece q = wu + 4k at K tile 0, as a 32-bit byte offset from a scalar base: the tile's first row
    // (contiguous rows: the offsets stay below 128 rows), or the operand's start for a row-list launch, whose rows then have to span
    // less than 4 GB (checked by the launcher; 439 MB for the 274 k x 400 user nodes of a 4 096-row pass)
    const long arow0 = g.rowidx ? 0 : (long)(m0 < Mv ? m0 : Mv - 1);
    const char* const abase = reinterpret_cast<const char*>(g.a0 + arow0 * g.lda0);
    unsigned aoff[APW];
    int ac4[APW];
#pragma unroll
    for (int k = 0; k < APW; ++k) {
        const int sl = (wm + 4 * k) * 64 + lane;
        const int r = sl >> 3, c4 = (sl & 7) ^ ((r >> 1) & 7);
        int gm = m0 + r;
        gm = gm < Mv ? gm : Mv - 1;                              // rows >= Mv are never stored
        if (g.rowidx) gm = g.rowidx[gm];
        aoff[k] = (unsigned)((((long)gm - arow0) * g.lda0 + c4 * 4) * 4);
        ac4[k] = c4 * 4;
    }
    auto issue_a_piece = [&](int kt, int abuf, int k) {      // piece k (0 .. APW - 1) of this wave's share of the A tile
        // K % 4 == 0, K >= 32; a float4 past K reads the row start instead (finite) and meets zero weights: only the LAST K tile can
        // reach past K (wave-uniform test), every other tile's K offset is scalar
        unsigned vo = aoff[k];
        long sk = (long)kt * 128;
        if (kt * 32 + 32 > g.K) { vo += kt * 32 + ac4[k] < g.K ? (unsigned)kt * 128u : 0u; sk = 0; }
        lds_dma16_s(abase + sk, vo, ldsA + (unsigned)((abuf * (TROWS * 8) + (wu + 4 * k) * 64) * 16));
    };
    auto issue_a = [&](int kt, int abuf) {
#pragma unroll
        for (int k = 0; k < APW; ++k) issue_a_piece(kt, abuf, k);
    };
    auto split_half = [&](const float4& v, unsigned (&o)[3][2]) {
        const Split3f s0 = split3f(v.x), s1 = split3f(v.y), s2 = split3f(v.z), s3 = split3f(v.w);
        o[0][0] = pack_hi16(s0.a, s1.a); o[0][1] = pack_hi16(s2.a, s3.a);
        o[1][0] = pack_hi16(s0.b, s1.b); o[1][1] = pack_hi16(s2.b, s3.b);
        o[2][0] = pack_hi16(s0.c, s1.c); o[2][1] = pack_hi16(s2.c, s3.c);
    };
    float amax = 0.f;                        // fp16x3: largest |activation| x 2^4 seen by this lane (range check)
    auto split_mt = [&](int mt, int abuf, bf16x8 (&dst)[3][MT]) {     // this lane's 8 k of row (mt, lr): LDS -> 3 bf16 (2 fp16) fragments
        const int r = wm * WROWS + mt * 16 + lr;
        const int sw = (r >> 1) & 7;
        const float4 v0 = __builtin_bit_cast(float4, As[abuf][r * 8 + ((kg * 2) ^ sw)]);
        const float4 v1 = __builtin_bit_cast(float4, As[abuf][r * 8 + ((kg * 2 + 1) ^ sw)]);
        if constexpr (F16) {
            // activations scaled by 2^4 (exact; undone in the epilogue): the low piece is a normal fp16 down to |x| = 0.008
            // (unscaled: 0.125); |x| < 4094 keeps the high piece finite
            constexpr float xs = F16_ACT_SCALE;
            const float raw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            const float v[8] = {v0.x * xs, v0.y * xs, v0.z * xs, v0.w * xs, v1.x * xs, v1.y * xs, v1.z * xs, v1.w * xs};
            // the largest scaled magnitude this lane has split (v_max3_f32 with |.| modifiers: four instructions per row piece):
            // past fp16's 65504 the high piece saturates and the product silently loses bits, then overflows — reported through
            // g.range_flag at the end of the kernel so that the host can redo the run in the range-free bf16x6 format
            amax = fmaxf(fmaxf(amax, fabsf(v[0])), fabsf(v[1])); amax = fmaxf(fmaxf(amax, fabsf(v[2])), fabsf(v[3]));
            amax = fmaxf(fmaxf(amax, fabsf(v[4])), fabsf(v[5])); amax = fmaxf(fmaxf(amax, fabsf(v[6])), fabsf(v[7]));
            unsigned hi[4], lo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                hi[e] = pack_half_rtz(v[2 * e], v[2 * e + 1]);
                const fp16x2 h = __builtin_bit_cast(fp16x2, hi[e]);
                // lo = x 2^4 - hi, exact in fp32, rounded to nearest: written as an fma of the UNSCALED value so that hipcc emits one
                // v_fma_mixlo_f16 per element (fp16 operand read in place, fp16 result) instead of cvt + sub + cvt — the operand
                // split shares the SIMD's vector issue with the partner wave's MFMAs (1.9 vector instructions per MFMA before)
                const _Float16 l0 = (_Float16)__builtin_fmaf(raw[2 * e], xs, -(float)h[0]), l1 = (_Float16)__builtin_fmaf(raw[2 * e + 1], xs, -(float)h[1]);
                lo[e] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
            }
            dst[0][mt] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
            dst[1][mt] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
        } else {
            unsigned lo[3][2], hi[3][2];
            split_half(v0, lo);
            split_half(v1, hi);
#pragma unroll
            for (int p = 0; p < 3; ++p) dst[p][mt] = __builtin_bit_cast(bf16x8, make_uint4(lo[p][0], lo[p][1], hi[p][0], hi[p][1]));
        }
    };
    auto mma = [&](const bf16x8 w, const bf16x8 a, const v4f c) -> v4f {      // fragments are typed bf16x8 for storage only
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, w), __builtin_bit_cast(half8, a), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0);
    };

    int lite[NSUB];                           // products of the strip's segment (wave-uniform): 0 = six, 1 = three, 2 = one
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        const int seg = ((strip0 + s) * 80) / g.nseg;
        // wave-uniform, and made so explicitly: the division above goes through the vector unit, and with `lite` in a VGPR hipcc
        // wrapped the MFMAs of every 16-column block in an exec-mask branch (s_and_saveexec ... s_or_b64 exec + s_nop: 15 per K tile)
        lite[s] = FULL ? 0 : __builtin_amdgcn_readfirstlane(((g.x1_segs >> seg) & 1) ? 2 : ((g.x3_segs >> seg) & 1));
    }
    v4f acc[NSUB][MT][NT];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[s][mt][nt] = (v4f){0.f, 0.f, 0.f, 0.f};

    bf16x8 af[3][MT], afn[3][MT];
    if constexpr (NSUB == 1) {
#pragma unroll
        // every A buffer is filled before the loop: with a single K tile (K = 32) the second one takes a copy of it.  The last step
        // splits the buffer after its own (unused products) — never written, its LDS garbage reached fp16x3's range check (amax)
        // and raised range_flag on operands of ordinary size
        for (int j = 0; j < ABUF; ++j) issue_a(j < KT ? j : KT - 1, j);
#pragma unroll
        for (int j = 0; j < RING - 1; ++j) if (j < nsteps) issue_b(j);
    } else if constexpr (RAG) {
        issue_a(0, 0);
        if (ns == 1 && KT > 1) issue_a(1, 1);      // a one-strip tile keeps its A tiles two steps ahead (as the NSUB == 1 kernel does)
        issue_b_next();
        if (nsteps > 1) issue_b_next();
    } else {
        issue_a(0, 0);
        issue_b(0);
        if (nsteps > 1) issue_b(1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) split_mt(mt, 0, af);

    // The K loop.  ONE (ragged launches only, a compile-time flag so that a strip stays one basic block): this is a one-strip
    // tile — A(kt + 2) is issued at step kt into the buffer A(kt) was split from a step ago, and A(kt + 1) is split during step
    // kt.  Ragged tiles of two or three strips issue A(kt + 1) at strip 0 and split it at strip 1 like the full-width kernel,
    // into the other A buffer; their ring slot and step number are counted along, since kt * ns + s is no constant modulo RING.
    auto k_loop = [&](auto one_strip) __attribute__((always_inline)) {
        constexpr bool ONE = decltype(one_strip)::value;
        constexpr int SMAX = ONE ? 1 : NSUB;
        int step_r = 0, buf_r = 0;
        for (int kt = 0; kt < KT; ++kt) {
            const bool more = kt + 1 < KT;
            const int sbuf = RAG ? ((more ? kt + 1 : kt) & 1) : 0;      // the A tile the step splits (after the last K tile: the stale one)
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                if constexpr (RAG && !ONE) { if (s == 2 && ns == 2) break; }
                const bool split_here = ONE ? s == 0 : s == 1;
                const int step = RAG ? step_r : kt * NSUB + s;
                const int buf = RAG ? buf_r : step % RING;
                // queue, oldest first: image(step) | A tile requested a step ago | image(step+1): only the last may stay in flight
#ifdef DIGAT_GEMM_TIMERS
                const unsigned long long gt0 = GT_NOW();
                if (step > 0) gt_body += gt0 - gt_last;
#endif
                if constexpr (NSUB == 1) {
                    // needed now: image(kt) (issued RING - 1 steps ago) and A(kt + 1) (issued ABUF - 1 steps ago); a step issues
                    // [A, image].  With L = min(RING - 1, ABUF - 1) whole steps younger than both — plus, when the A tile is the
                    // younger of the two, the image issued right behind it — (4 + IMG_I) L (+ IMG_I) requests may stay in flight.
                    // The last steps issue less than that: they drain the queue.
                    constexpr int L = (RING - 1 < ABUF - 1 ? RING - 1 : ABUF - 1) - 1;
                    constexpr int KEEP = (APW + IMG_I) * (L < 0 ? 0 : L) + ((ABUF - 1 < RING - 1) ? IMG_I : 0);
                    static_assert(KEEP <= 63, "vmcnt is six bits");
                    if (kt + (RING - 1 > ABUF ? RING - 1 : ABUF) < KT) wait_vmcnt_imm<KEEP>();
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else if (step + 1 < nsteps) {
                    if constexpr (IMG_I == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef DIGAT_GEMM_TIMERS
                const unsigned long long gt1 = GT_NOW();
#endif
                __builtin_amdgcn_s_barrier();                          // landed for every wave; image(step-1) and the old A tile are free
#ifdef DIGAT_GEMM_TIMERS
                gt_last = GT_NOW();
                gt_wait += gt1 - gt0; gt_bar += gt_last - gt1; ++gt_steps;
#endif
                if (NSUB == 1) {
                    if (kt + ABUF < KT) issue_a(kt + ABUF, kt % ABUF);  // the buffer of A(kt): split during step kt - 1
                    if (step + RING - 1 < nsteps) issue_b(step + RING - 1);
                } else if constexpr (RAG) {
                    if constexpr (ONE) { if (kt + 2 < KT) issue_a(kt + 2, kt & 1); }
                    else if (s == 0 && more) issue_a(kt + 1, (kt + 1) & 1);
                    if (step + 2 < nsteps) issue_b_next();
                } else {
                    if (s == 0 && more) issue_a(kt + 1, 0);   // read at strip 1, after the next barrier
                    if (step + 2 < nsteps) issue_b(step + 2);
                }
                const uint4* Bi = Bs[buf];
                const int lslot = kg * 80 + lr;
                bf16x8 bq[2][3];
#pragma unroll
                for (int p = 0; p < PL; ++p) bq[0][p] = __builtin_bit_cast(bf16x8, Bi[p * 320 + lslot]);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    if (nt + 1 < NT) {
#pragma unroll
                        for (int p = 0; p < PL; ++p) bq[(nt + 1) & 1][p] = __builtin_bit_cast(bf16x8, Bi[p * 320 + lslot + (nt + 1) * 16]);
                    }
                    const bf16x8 b1 = bq[nt & 1][0], b2 = bq[nt & 1][1], b3 = bq[nt & 1][PL - 1];
                    v4f c[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) c[mt] = acc[s][mt][nt];
                    // the MT accumulators of a column block are independent chains: the products go round them (mt innermost)
                    if (!F16 && (FULL || !lite[s])) {
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b1, af[2][mt], c[mt]);   // x3 w1
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b2, af[1][mt], c[mt]);   // x2 w2
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b3, af[0][mt], c[mt]);   // x1 w3
                    }
                    if (FULL || lite[s] < 2) {        // fp16x3: lo.hi and hi.lo
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b1, af[1][mt], c[mt]);   // x2 w1
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b2, af[0][mt], c[mt]);   // x1 w2
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) c[mt] = mma(b1, af[0][mt], c[mt]);       // x1 w1
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[s][mt][nt] = c[mt];
                    if (NSUB > 1) {      // the next K tile's rows landed at this step's wait (requested at strip 0); after the last
                                         // K tile the split runs on the stale tile (unused) so that the strip stays one basic block
                        if (split_here && nt == 0) split_mt(0, sbuf, afn);
                        if constexpr (MT > 1) { if (split_here && nt == 2) split_mt(1, sbuf, afn); }
                    } else {             // one-strip tiles: A(kt + 1) landed at this step's wait (after the last K tile: a stale buffer, unused)
                        if (nt == 0) split_mt(0, (kt + 1) % ABUF, afn);
                        if constexpr (MT > 1) { if (nt == 2) split_mt(1, (kt + 1) % ABUF, afn); }
                    }
                }
                if (NSUB == 1 || split_here) {
                    // the ~100 vector instructions of the operand split go two per MFMA (an MFMA holds the SIMD's vector issue for
                    // 8 of its 16 cycles: two 4-cycle instructions fit in the gap) instead of two bursts that stall the matrix pipe
#pragma unroll
                    for (int i = 0; i < 56; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    }
                }
                if constexpr (RAG) { ++step_r; buf_r = buf_r == RING - 1 ? 0 : buf_r + 1; }
            }
            if (more) {
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) af[p][mt] = afn[p][mt];
            }
        }
    };
    if constexpr (RAG) {
        if (ns == 1) k_loop(std::true_type{});
        else k_loop(std::false_type{});
    } else k_loop(std::false_type{});

#ifdef DIGAT_GEMM_TIMERS
    const unsigned long long gt_loop_end = GT_NOW();
    gt_body += gt_loop_end - gt_last;
#endif
    if constexpr (F16) {
        // inf and |x| >= 4094 raise the flag.  A NaN activation does not (fmaxf drops NaN operands): it reaches the outputs as NaN,
        // as it does in the reference.  Rows past Mv are clamped copies of a real row.
        if (g.range_flag && __builtin_amdgcn_ballot_w64(!(amax < 65504.f)) != 0 && lane == 0) atomicOr(g.range_flag, 1u);
    }
    // The weights are the MFMA's row operand, the activations its column operand, so a lane ends up with four
    // CONSECUTIVE output columns (4*kg .. 4*kg+3 of each 16-column block) of one row (lr): float4 bias / residual
    // loads and float4 stores, a quarter of the instructions of the row-major accumulator layout.
    // Every global READ of the epilogue — row index, bias, the K3 addend, the residual / accumulate operand — is requested in
    // batches of NT behind WAVE-UNIFORM conditions (a strip lies in one segment) and consumed afterwards; with a per-lane
    // condition in front of every load ("row in range ? ...") hipcc waited after each one.  Rows past Mv are clamped copies of
    // row Mv - 1: computed, never stored.  (The phase timers of tools/exp/gemm_lab.py put the epilogue at a fifth of the kernel:
    // 165 MB of results leave at HBM write speed while the matrix cores idle — all workgroups of a round finish together.)
    int gmv[MT];
    bool rok[MT];
    {
        const int* const ri = (g.rowidx && !g.gather_only) ? g.rowidx : nullptr;      // wave-uniform
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int gv = m0 + wm * WROWS + mt * 16 + lr;
            rok[mt] = gv < Mv;
            const int gvc = rok[mt] ? gv : Mv - 1;
            gmv[mt] = ri ? ri[gvc] : gvc;
        }
    }
    const bool has_e0 = g.epi == EPI_RELU_RES || g.epi == EPI_ADD_E0;
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        if constexpr (RAG) { if (s >= ns) break; }       // a short tile's missing strips lie past N (or in nobody's segment)
        const int ncol0 = (strip0 + s) * 80;             // first column of this strip in the stacked output
        const int seg = ncol0 / g.nseg;
        const int nbase = ncol0 - seg * g.nseg + kg * 4;
        const float* const bp = g.bias[seg];
        const bool radd_here = g.radd && seg == g.radd_seg;
        const bool y16 = (g.bf16_segs >> seg) & 1;
        const bool y8 = (g.fp8_segs >> seg) & 1;
        float4 bv[NT];
        if (bp) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(bp + nbase + nt * 16);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int gm = gmv[mt];
            float* const yrow = g.y[seg] + (long)gm * g.ldy;
            float4 rv[NT], ev[NT];
            if (radd_here) {
                const float* rrow = g.radd + (long)(gm / g.rows_per_b) * g.nseg + nbase;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) rv[nt] = *reinterpret_cast<const float4*>(rrow + nt * 16);
            }
            if (y8) {
                // P' / Q of Eq. 8 as block-scaled OCP e4m3 (BASELINE configs[4]; CDNA4's block-scaled layout): the wave tile owns
                // whole 80-column strips of its rows — row lr's 80 results sit in the four lanes (kg, lr), 20 each — so the
                // block is (row, strip), its scale the block's absmax / 448 (e4m3's largest finite value), found with two lane
                // exchanges and no second pass over the results.  4-byte stores of four codes + one fp32 scale per block.
                float4 vv[NT];
                float amx = 0.f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const v4f a = acc[s][mt][nt];
                    float4 v = make_float4(a[0], a[1], a[2], a[3]);
                    if constexpr (F16) {
                        constexpr float u = 1.f / (F16_WEIGHT_SCALE * F16_ACT_SCALE);
                        v = make_float4(v.x * u, v.y * u, v.z * u, v.w * u);
                    }
                    if (bp) v = f4_add(v, bv[nt]);
                    if (radd_here) v = f4_add(rv[nt], v);
                    vv[nt] = v;
                    amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
                }
                amx = fmaxf(amx, __shfl_xor(amx, 16, 64));
                amx = fmaxf(amx, __shfl_xor(amx, 32, 64));
                const float scale = amx > 0.f ? amx * (1.f / 448.f) : 1.f;
                const float inv = 1.f / scale;
                unsigned char* const row8 = reinterpret_cast<unsigned char*>(g.y[seg]) + (long)gm * g.ldy8;
                if (rok[mt]) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        int w = 0;
                        w = __builtin_amdgcn_cvt_pk_fp8_f32(vv[nt].x * inv, vv[nt].y * inv, w, false);
                        w = __builtin_amdgcn_cvt_pk_fp8_f32(vv[nt].z * inv, vv[nt].w * inv, w, true);
                        *reinterpret_cast<int*>(row8 + nbase + nt * 16) = w;
                    }
                    if (kg == 0) *reinterpret_cast<float*>(row8 + g.nseg + 4 * ((ncol0 - seg * g.nseg) / 80)) = scale;
                }
                continue;
            }
            if (has_e0) {
                const float* erow = g.e0 + (long)gm * g.lde0 + nbase;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) ev[nt] = *reinterpret_cast<const float4*>(erow + nt * 16);
            } else if (g.epi == EPI_ACCUM) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) ev[nt] = *reinterpret_cast<const float4*>(yrow + nbase + nt * 16);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int nn = nbase + nt * 16;
                const v4f a = acc[s][mt][nt];
                float4 v = make_float4(a[0], a[1], a[2], a[3]);
                if constexpr (F16) {                 // the operands carry 2^10 and 2^4
                    constexpr float u = 1.f / (F16_WEIGHT_SCALE * F16_ACT_SCALE);
                    v = make_float4(v.x * u, v.y * u, v.z * u, v.w * u);
                }
                if (bp) v = f4_add(v, bv[nt]);
                if (radd_here) v = f4_add(rv[nt], v);
                if (y16) {            // P' / Q of Eq. 8 kept in bf16 (they only feed the score): 8-byte stores
                    if (rok[mt])
                        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(g.y[seg]) + (long)gm * g.ldy + nn) =
                            make_uint2(pack_bf16_rne(v.x, v.y), pack_bf16_rne(v.z, v.w));
                    continue;
                }
                if (g.epi == EPI_RELU_RES) {
                    const float4 x = ev[nt];
                    v = make_float4(fmaxf(v.x, 0.f) + x.x, fmaxf(v.y, 0.f) + x.y, fmaxf(v.z, 0.f) + x.z, fmaxf(v.w, 0.f) + x.w);
                }
                if (g.epi == EPI_ACCUM || g.epi == EPI_ADD_E0) v = f4_add(ev[nt], v);
                if constexpr (!F16) {                // training only (bf16x6): the input dropout's backward on the way out
                    if (g.dmask && rok[mt] && (g.dmask_cols == 0 || nn < g.dmask_cols)) {
                        const unsigned mk = *reinterpret_cast<const unsigned*>(g.dmask + (long)gm * g.lddm + nn);
                        v = make_float4((mk & 0xffu) ? v.x * g.dscale : 0.f, (mk & 0xff00u) ? v.y * g.dscale : 0.f,
                                        (mk & 0xff0000u) ? v.z * g.dscale : 0.f, (mk & 0xff000000u) ? v.w * g.dscale : 0.f);
                    }
                }
                if (rok[mt]) *reinterpret_cast<float4*>(yrow + nn) = v;
            }
        }
    }
#ifdef DIGAT_GEMM_TIMERS
    if (lane == 0 && (blockIdx.x & 15) < 8) {
        const unsigned long long gt_end = GT_NOW();
        atomicAdd(&g_gemm_timers[0], gt_wait); atomicAdd(&g_gemm_timers[1], gt_bar); atomicAdd(&g_gemm_timers[2], gt_body);
        atomicAdd(&g_gemm_timers[3], gt_steps); atomicAdd(&g_gemm_timers[5], gt_end - gt_loop_end);
        atomicAdd(&g_gemm_timers[6], 1ull); atomicAdd(&g_gemm_timers[7], gt_end - gt_enter);
    }
#endif
}

// 1c. skinny linear for the [B,d] projections (M < 2048): a latency chain, not a throughput problem
// =================================================================================================
// 32x80 output tile per workgroup; the four waves split K (16-wide k blocks, wave w takes blocks
// w, w+4, ...) and load their MFMA operand fragments straight from global memory as float4 — lane
// (row l&15, quarter q) holds k = 16*kb + 4q .. +3 of its row and feeds element s to the s-th
// v_mfma_f32_16x16x4_f32 k-step, for A and B alike — with the next block's loads in flight under the
// current block's 40 MFMAs.  No LDS staging, no barrier in the K loop; one LDS reduction at the end.
// A may be two K-segments split at a multiple of 16 (the gate's [local ; global]); epilogues as gemm_f32.
// TW: the weight is stored [K, nseg] and used as its transpose (the input gradient dX = dY W of a [B,d] linear): a lane's four k of
// a column are then nseg floats apart — four scalar loads, each 64 contiguous bytes across the 16 lanes of a quarter.
template <int MT, bool KTAIL, bool TW = false>   // MT: 16-row tiles of A per workgroup: 2 (32x80 output tiles) or 1 (16x80: twice the
                                // workgroups, half the LDS); KTAIL: K % 16 != 0 (the last k block is partly past K and must be zeroed)
__global__ void __launch_bounds__(256) gemm_skinny_kernel(const GemmArgs g) {
    __shared__ float red[4][MT * 20][64];
    const int tile = blockIdx.x;
    const int mtile = tile / g.ntiles, ntile = tile - mtile * g.ntiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int m0 = mtile * (MT * 16), n0 = ntile * 80;
    const int seg = n0 / g.nseg;
    const int nbase = n0 - seg * g.nseg;
    const float* const wseg = g.w[seg];
    const int nkb = (g.K + 15) >> 4;

    const float* arow[MT][2];    // [mt][A segment]
    bool aok[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int gm = m0 + mt * 16 + lr;
        aok[mt] = gm < g.M;
        arow[mt][0] = g.a0 + (long)(aok[mt] ? gm : 0) * g.lda0;
        arow[mt][1] = g.a1 ? g.a1 + (long)(aok[mt] ? gm : 0) * g.lda1 : arow[mt][0];
    }
    const float* brow[5];
    bool bok[5];
#pragma unroll
    for (int nt = 0; nt < 5; ++nt) {
        const int nn = nbase + nt * 16 + lr;
        bok[nt] = nn < g.nseg;
        brow[nt] = TW ? wseg + (bok[nt] ? nn : 0) : wseg + (long)(bok[nt] ? nn : 0) * g.K;
    }
    // Straight-line loads.  Rows past M and weight rows past nseg were clamped to row 0 above: what they produce lands in
    // output rows / columns that are never stored (an MFMA row or column only feeds its own outputs).  A k block past K
    // (KTAIL) re-reads the row's last float4 and is zeroed by a multiply — not a select, which lets the compiler make the
    // load conditional again.  With a branch per load ("in range ? load : 0") hipcc cannot count the requests in flight and
    // drains the queue (vmcnt(0)) before every block's MFMAs: the prefetch then buys nothing and every k block costs a
    // full global round trip (1.8 us per block measured, 17 us per launch).
    auto load_block = [&](int kb, float4* a, float4* b) {
        const int k = kb * 16 + 4 * lq;
        const int kc = (KTAIL && k >= g.K) ? g.K - 4 : k;
        const float mk = (KTAIL && k >= g.K) ? 0.f : 1.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float* p = kc < g.k0 ? arow[mt][0] + kc : arow[mt][1] + (kc - g.k0);
            const float4 v = *reinterpret_cast<const float4*>(p);
            a[mt] = KTAIL ? make_float4(v.x * mk, v.y * mk, v.z * mk, v.w * mk) : v;
        }
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) {
            float4 v;
            if constexpr (TW) {
                const float* c = brow[nt] + (long)kc * g.nseg;
                v = make_float4(c[0], c[g.nseg], c[2 * (long)g.nseg], c[3 * (long)g.nseg]);
            } else {
                v = *reinterpret_cast<const float4*>(brow[nt] + kc);
            }
            b[nt] = KTAIL ? make_float4(v.x * mk, v.y * mk, v.z * mk, v.w * mk) : v;
        }
    };

    v4f acc[MT][5];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = (v4f){0.f, 0.f, 0.f, 0.f};

    // A wave takes PAIRS of adjacent k blocks (2w, 2w+1), (8+2w, 8+2w+1), ...: a lane's two float4 of a pair are the two
    // halves of one 128-byte line quarter-group, requested back to back, so the second half hits in the CU's L1 — with
    // blocks w, w+4, ... the other half came four blocks later, after 48 KB of other lines, and was fetched from L2 again
    // (these launches move 50-100 MB from L2 for < 1 GFLOP: L2 bandwidth is what they wait for).
    auto blk = [&](int q) { return 8 * (q >> 1) + 2 * wave + (q & 1); };
    float4 a0[MT], b0[5], a1[MT], b1[5];
    int q = 0;
    if (blk(0) < nkb) load_block(blk(0), a0, b0);
    while (blk(q) < nkb) {
        if (blk(q + 1) < nkb) load_block(blk(q + 1), a1, b1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 5; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_comp(a0[mt], s), f4_comp(b0[nt], s), acc[mt][nt], 0, 0, 0);
        ++q;
        if (blk(q) >= nkb) break;
        if (blk(q + 1) < nkb) load_block(blk(q + 1), a0, b0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 5; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_comp(a1[mt], s), f4_comp(b1[nt], s), acc[mt][nt], 0, 0, 0);
        ++q;
    }
    // K-split reduction in wave order 0..3 (deterministic); wave w finalises accumulator registers [5 MT w, 5 MT (w+1))
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(mt * 5 + nt) * 4 + r][lane] = acc[mt][nt][r];
    __syncthreads();
    const float* bp = g.bias[seg];
    float* yp = g.y[seg];
    for (int q = 0; q < MT * 5; ++q) {
        const int reg = wave * (MT * 5) + q;
        const int mt = reg / 20, nt = (reg / 4) % 5, r = reg & 3;
        const int gm = m0 + mt * 16 + lq * 4 + r;
        const int nn = nbase + nt * 16 + lr;
        if (gm >= g.M || nn >= g.nseg) continue;
        float v = ((red[0][reg][lane] + red[1][reg][lane]) + red[2][reg][lane]) + red[3][reg][lane];
        v += bp ? bp[nn] : 0.f;
        if (g.epi == EPI_RELU_RES) {
            v = fmaxf(v, 0.f) + g.e0[(long)gm * g.lde0 + nn];
        } else if (g.epi == EPI_GATE) {
            const float gate = 1.f / (1.f + expf(-v));
            const float loc = g.e0[(long)gm * g.lde0 + nn];
            const float glo = g.e1[(long)gm * g.lde1 + nn];
            v = gate * loc + (1.f - gate) * glo;
            if (g.e2) v = g.e2[(long)gm * g.lde2 + nn] + v;
        } else if (g.epi == EPI_ACCUM) {
            v = yp[(long)gm * g.ldy + nn] + v;
        }
        yp[(long)gm * g.ldy + nn] = v;
    }
}

// 1d. skinny linear on pre-split weight images (round 3): the [B,d] linears of the inference path
// =================================================================================================
// The fp32 skinny kernel above fetches its weight fragments as 64-byte row pieces — 16 cache lines per wave-instruction, half of
// each used — and issues 8 fp32 MFMAs (32 cycles each) per 32 k: 12-25 us per launch for 0.3-1 GFLOP, thirteen launches per
// scoring step.  Neither more loads in flight (every k block of a wave requested up front) nor eight waves splitting K moved it
// (measured: 15.2 -> 16.6 us, 14.9 -> 16.0 us): the fragments' request rate is what it waits for.  Here the weights come from the
// SAME split images the strip-mined kernel uses (digat_split_weights*: one image per 80-column strip and 32-deep K tile,
// [plane][k group][row] 16-byte slots): a lane's fragment is one 16-byte load and a wave-instruction reads four contiguous
// 256-byte runs; the activations are split in registers exactly as there (two scaled fp16 pieces / three bf16 pieces), and a
// 32-deep K tile is 3 (6) 16-cycle MFMAs per 16 x 16 outputs.  Same tile as before — (16 MT) rows x 80 columns per workgroup,
// the four waves splitting K by K tiles, one ordered LDS reduction — and the same epilogues.  fp32-grade like the projections.
template <int MT, bool F16>
__global__ void __launch_bounds__(256) gemm_skinny_split_kernel(const GemmArgs g) {
    constexpr int PL = F16 ? 2 : 3;
    constexpr int IMG_BYTES = PL * 320 * 16;
    __shared__ v4f red[4][MT * 5][64];
    const int tile = blockIdx.x;
    const int mtile = tile / g.ntiles, strip = tile - mtile * g.ntiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kg = lane >> 4, lr = lane & 15;
    const int m0 = mtile * (MT * 16), n0 = strip * 80;
    const int seg = n0 / g.nseg;
    const int nbase = n0 - seg * g.nseg;
    const int KT = (g.K + 31) >> 5;
    const char* const wimg = reinterpret_cast<const char*>(g.wsplit) + (long)strip * KT * IMG_BYTES + (long)(kg * 80 + lr) * 16;

    const float* arow[MT][2];    // [mt][A segment]; rows past M are clamped (computed, never stored)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int gm = min(m0 + mt * 16 + lr, g.M - 1);
        arow[mt][0] = g.a0 + (long)gm * g.lda0;
        arow[mt][1] = g.a1 ? g.a1 + (long)gm * g.lda1 : arow[mt][0];
    }
    // this lane's 8 k of K tile kt: k = 32 kt + 8 kg .. + 7 (k0 is a multiple of 8: the two float4 lie in one A segment); a k
    // past K re-reads the row's first float4 (finite) and meets the zero padding of the weight image
    auto load_tile = [&](int kt, uint4 (&b)[PL][5], float4 (&a)[MT][2]) {
        const char* src = wimg + (long)kt * IMG_BYTES;
#pragma unroll
        for (int p = 0; p < PL; ++p)
#pragma unroll
            for (int nt = 0; nt < 5; ++nt) b[p][nt] = *reinterpret_cast<const uint4*>(src + (p * 320 + nt * 16) * 16);
        const int k = kt * 32 + kg * 8;
        const bool in = k < g.K;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float* pa = !in ? arow[mt][0] : (k < g.k0 ? arow[mt][0] + k : arow[mt][1] + (k - g.k0));
            a[mt][0] = *reinterpret_cast<const float4*>(pa);
            a[mt][1] = *reinterpret_cast<const float4*>(pa + (in ? 4 : 0));
        }
    };
    float amax = 0.f;
    auto split = [&](const float4& v0, const float4& v1, bf16x8 (&dst)[3]) {
        if constexpr (F16) {
            constexpr float xs = F16_ACT_SCALE;
            const float raw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            const float v[8] = {v0.x * xs, v0.y * xs, v0.z * xs, v0.w * xs, v1.x * xs, v1.y * xs, v1.z * xs, v1.w * xs};
            amax = fmaxf(fmaxf(amax, fabsf(v[0])), fabsf(v[1])); amax = fmaxf(fmaxf(amax, fabsf(v[2])), fabsf(v[3]));
            amax = fmaxf(fmaxf(amax, fabsf(v[4])), fabsf(v[5])); amax = fmaxf(fmaxf(amax, fabsf(v[6])), fabsf(v[7]));
            unsigned hi[4], lo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                hi[e] = pack_half_rtz(v[2 * e], v[2 * e + 1]);
                const fp16x2 h = __builtin_bit_cast(fp16x2, hi[e]);
                const _Float16 l0 = (_Float16)__builtin_fmaf(raw[2 * e], xs, -(float)h[0]), l1 = (_Float16)__builtin_fmaf(raw[2 * e + 1], xs, -(float)h[1]);
                lo[e] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
            }
            dst[0] = __builtin_bit_cast(bf16x8, make_uint4(hi[0], hi[1], hi[2], hi[3]));
            dst[1] = __builtin_bit_cast(bf16x8, make_uint4(lo[0], lo[1], lo[2], lo[3]));
        } else {
            const Split3f s0 = split3f(v0.x), s1 = split3f(v0.y), s2 = split3f(v0.z), s3 = split3f(v0.w);
            const Split3f t0 = split3f(v1.x), t1 = split3f(v1.y), t2 = split3f(v1.z), t3 = split3f(v1.w);
            dst[0] = __builtin_bit_cast(bf16x8, make_uint4(pack_hi16(s0.a, s1.a), pack_hi16(s2.a, s3.a), pack_hi16(t0.a, t1.a), pack_hi16(t2.a, t3.a)));
            dst[1] = __builtin_bit_cast(bf16x8, make_uint4(pack_hi16(s0.b, s1.b), pack_hi16(s2.b, s3.b), pack_hi16(t0.b, t1.b), pack_hi16(t2.b, t3.b)));
            dst[2] = __builtin_bit_cast(bf16x8, make_uint4(pack_hi16(s0.c, s1.c), pack_hi16(s2.c, s3.c), pack_hi16(t0.c, t1.c), pack_hi16(t2.c, t3.c)));
        }
    };
    auto mma = [](const bf16x8 w, const bf16x8 a, const v4f c) -> v4f {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, w), __builtin_bit_cast(half8, a), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, c, 0, 0, 0);
    };
    v4f acc[MT][5];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) acc[mt][nt] = (v4f){0.f, 0.f, 0.f, 0.f};
    auto compute = [&](const uint4 (&b)[PL][5], const float4 (&a)[MT][2]) {
        bf16x8 af[MT][3];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) split(a[mt][0], a[mt][1], af[mt]);
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) {
            const bf16x8 b1 = __builtin_bit_cast(bf16x8, b[0][nt]), b2 = __builtin_bit_cast(bf16x8, b[1][nt]),
                         b3 = __builtin_bit_cast(bf16x8, b[PL - 1][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                v4f c = acc[mt][nt];
                if constexpr (!F16) {
                    c = mma(b1, af[mt][2], c);    // x3 w1
                    c = mma(b2, af[mt][1], c);    // x2 w2
                    c = mma(b3, af[mt][0], c);    // x1 w3
                }
                c = mma(b1, af[mt][1], c);        // x2 w1   (fp16x3: lo . hi)
                c = mma(b2, af[mt][0], c);        // x1 w2   (fp16x3: hi . lo)
                c = mma(b1, af[mt][0], c);        // x1 w1
                acc[mt][nt] = c;
            }
        }
    };
    // wave w takes K tiles w, w + 4, ...: the next tile's fragments are in flight under the current tile's MFMAs
    uint4 b0[PL][5], b1[PL][5];
    float4 a0[MT][2], a1[MT][2];
    int kt = wave;
    if (kt < KT) load_tile(kt, b0, a0);
    while (kt < KT) {
        if (kt + 4 < KT) load_tile(kt + 4, b1, a1);
        compute(b0, a0);
        kt += 4;
        if (kt >= KT) break;
        if (kt + 4 < KT) load_tile(kt + 4, b0, a0);
        compute(b1, a1);
        kt += 4;
    }
    if constexpr (F16) {
        if (g.range_flag && __builtin_amdgcn_ballot_w64(!(amax < 65504.f)) != 0 && lane == 0) atomicOr(g.range_flag, 1u);
    }
    // K-split reduction in wave order 0..3 (deterministic); wave w finalises the 16 x 16 tiles t = w, w + 4, ...
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 5; ++nt) red[wave][mt * 5 + nt][lane] = acc[mt][nt];
    __syncthreads();
    const float* bp = g.bias[seg];
    float* yp = g.y[seg];
    for (int t = wave; t < MT * 5; t += 4) {
        const int mt = t / 5, nt = t - mt * 5;
        const int gm = m0 + mt * 16 + lr;                 // accumulator lane (kg, lr): row lr, columns 4 kg .. 4 kg + 3 of the tile
        const int nn = nbase + nt * 16 + kg * 4;
        if (gm >= g.M) continue;
        const v4f r0 = red[0][t][lane], r1 = red[1][t][lane], r2 = red[2][t][lane], r3 = red[3][t][lane];
        float4 v = make_float4(((r0[0] + r1[0]) + r2[0]) + r3[0], ((r0[1] + r1[1]) + r2[1]) + r3[1],
                               ((r0[2] + r1[2]) + r2[2]) + r3[2], ((r0[3] + r1[3]) + r2[3]) + r3[3]);
        if constexpr (F16) {
            constexpr float u = 1.f / (F16_WEIGHT_SCALE * F16_ACT_SCALE);
            v = make_float4(v.x * u, v.y * u, v.z * u, v.w * u);
        }
        if (bp) v = f4_add(v, *reinterpret_cast<const float4*>(bp + nn));
        if (g.epi == EPI_RELU_RES) {
            const float4 x = *reinterpret_cast<const float4*>(g.e0 + (long)gm * g.lde0 + nn);
            v = make_float4(fmaxf(v.x, 0.f) + x.x, fmaxf(v.y, 0.f) + x.y, fmaxf(v.z, 0.f) + x.z, fmaxf(v.w, 0.f) + x.w);
        } else if (g.epi == EPI_GATE) {
            const float4 loc = *reinterpret_cast<const float4*>(g.e0 + (long)gm * g.lde0 + nn);
            const float4 glo = *reinterpret_cast<const float4*>(g.e1 + (long)gm * g.lde1 + nn);
            const float4 gt = make_float4(1.f / (1.f + expf(-v.x)), 1.f / (1.f + expf(-v.y)), 1.f / (1.f + expf(-v.z)), 1.f / (1.f + expf(-v.w)));
            v = make_float4(gt.x * loc.x + (1.f - gt.x) * glo.x, gt.y * loc.y + (1.f - gt.y) * glo.y,
                            gt.z * loc.z + (1.f - gt.z) * glo.z, gt.w * loc.w + (1.f - gt.w) * glo.w);
            if (g.e2) v = f4_add(*reinterpret_cast<const float4*>(g.e2 + (long)gm * g.lde2 + nn), v);
        } else if (g.epi == EPI_ACCUM) {
            v = f4_add(*reinterpret_cast<const float4*>(yp + (long)gm * g.ldy + nn), v);
        }
        *reinterpret_cast<float4*>(yp + (long)gm * g.ldy + nn) = v;
    }
}

// =================================================================================================
// 1e. "fp16-fp8c": the Eq. 8 node projections with the two correction products on the fp8 matrix cores
// =================================================================================================
// fp16x3 (above) computes x.w as x_hi w_hi + x_hi w_lo + x_lo w_hi, all three on v_mfma_f32_16x16x32_f16.  The two corrections
// are each ~2^-11 of the result, so they can carry e4m3's 2^-4 relative step and still land at ~2^-15 of it: here they run on
// the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 as q(w_lo) q(x_hi) + q(w_hi) q(x_lo), q = OCP e4m3 with one E8M0 (power of
// two) scale per 32 consecutive K values — the instruction's own MX block — chosen so that the block's largest magnitude maps to
// at most 448 (no saturation).  x_hi w_hi stays on fp16, exactly as fp16x3 makes it (same 2^10 / 2^4 scaling, same pieces:
// w_hi rounded to nearest, x_hi truncated; the corrections quantise the fp32 remainders w - w_hi, x - x_hi directly).
//
// Operand layout of the 16x16x128 form, measured on gfx950 with exact data (NOT one 32-deep block per lane): lane l (row /
// column l & 15, group g = l >> 4) holds K 16 g .. 16 g + 15 in bytes 0-15 and K 64 + 16 g .. + 15 in bytes 16-31, and the scale
// of MX block b (K 32 b .. 32 b + 31) is read from the scale VGPR of lane group b (byte chosen by op_sel).  A block's 32 values
// therefore sit in two lanes (g, g ^ 1): a block scale costs one lane exchange (l ^ 16), and handing each lane group its
// block's scale one more (l ^ 48: groups 1 and 2 supply the blocks of the other pair).
// The fp16 product's four 32-deep k-steps are fed the same 32 K values per lane, in a PERMUTED k order — value v of a lane
// (v < 16: K 16 g + v, else K 64 + 16 g + v - 16) is element v % 8 of k-step v / 8, for both operands, so the sum is unchanged —
// so the activation split is lane-local but for the two exchanges of the scales.
//
// Image of one (80-column strip, 128-deep K tile), K zero-padded to a multiple of 128 (F8C_IMG_BYTES = 41 984 bytes, 41 DMA pieces):
//   slots    0 .. 1279: w_hi fp16,       [s 4][k group 4][row 80] x 8 halves   (values 8 s .. 8 s + 7 of lane (group, row))
//   slots 1280 .. 1919: q(w_hi) e4m3,    [half 2][k group 4][row 80] x 16 bytes (K 64 half + 16 group + j)
//   slots 1920 .. 2559: q(w_lo) e4m3,    same
//   bytes 40960 .. 41983: E8M0 scales,   [plane 2][block 4][row & 15][row >> 4, padded to 8] bytes
// Every fragment read is a 16-byte slot on consecutive slots for consecutive lanes (the shipped kernel's conflict-free pattern),
// and a lane's scales for the five 16-column blocks of a strip are one 8-byte read per plane (byte = block, picked by op_sel).
constexpr int F8C_IMG_BYTES = 41984;
constexpr int F8C_PIECES = F8C_IMG_BYTES / 1024;
typedef int v8i __attribute__((ext_vector_type(8)));

// E8M0 exponent (biased) of the block scale of a block whose largest magnitude is amax: the least power of two 2^(x - 127) with
// amax / 2^(x - 127) <= 448 (e4m3's largest finite value: 1.75 x 2^8); amax = 0 gives x = 0 (any scale would do)
__device__ __forceinline__ int f8c_e8m0(float amax) {
    const unsigned u = __builtin_bit_cast(unsigned, amax);
    int x = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return x < 0 ? 0 : (x > 253 ? 253 : x);
}
__device__ __forceinline__ float f8c_inv_scale(int x) { return __builtin_bit_cast(float, (unsigned)(254 - x) << 23); }   // 2^(127 - x)
// 32 values (scaled by 2^(127 - x), |v| <= 448) -> 32 e4m3 codes, round to nearest even
__device__ __forceinline__ v8i f8c_codes(const float (&v)[32], float inv) {
    v8i o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, w, true);
        o[i] = w;
    }
    return o;
}

// the scaled MFMA on e4m3 operands; byte `ba` of the A scale word and byte OB of the B scale word (op_sel: compile-time; `ba` is
// one after unrolling)
template <int OB>
__device__ __forceinline__ v4f f8c_mma(int ba, const v8i a, const v8i b, const v4f c, int sa, int sb) {
    switch (ba) {
        case 0: return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, sa, OB, sb);
        case 1: return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 1, sa, OB, sb);
        case 2: return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 2, sa, OB, sb);
        default: return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 3, sa, OB, sb);
    }
}

// the same with values 0 .. 15 and 16 .. 31 under two scales (the two MX blocks a lane's operand touches)
__device__ __forceinline__ v8i f8c_codes2(const float (&v)[32], float inv0, float inv1) {
    v8i o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float inv = i < 4 ? inv0 : inv1;
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, w, true);
        o[i] = w;
    }
    return o;
}

// one thread per (strip, K tile, MX block, row): that row's 32 K values of the block -> its slots in the three planes (two lanes'
// halves) + the block's two scale bytes
__global__ void __launch_bounds__(256) split_weights_f8c_kernel(const float* w0, const float* w1, const float* w2, int nseg, int nsegs,
                                                                int K, unsigned char* out) {
    const int KT = (K + 127) >> 7;
    const int Ntot = nseg * nsegs;
    const int strips = (Ntot + 79) / 80;
    const long total = (long)strips * KT * 320;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i % 80), bk = (int)((i / 80) & 3);
        const long img = i / 320;                       // strip * KT + kt
        const int strip = (int)(img / KT), kt = (int)(img - (long)strip * KT);
        const int n = strip * 80 + r, k0 = kt * 128 + bk * 32;
        float hi[32], lo[32];
        float ah = 0.f, al = 0.f;
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            float v = 0.f;
            if (n < Ntot && k0 + e < K) {
                const int seg = n / nseg;
                v = (seg == 0 ? w0 : (seg == 1 ? w1 : w2))[(long)(n - seg * nseg) * K + k0 + e];
            }
            const float vs = v * F16_WEIGHT_SCALE;       // as fp16x3: w_hi = fp16(w 2^10), round to nearest
            const float h = (float)(_Float16)vs;
            hi[e] = h; lo[e] = vs - h;                   // exact in fp32
            ah = fmaxf(ah, fabsf(h)); al = fmaxf(al, fabsf(lo[e]));
        }
        unsigned char* const base = out + img * F8C_IMG_BYTES;
        uint4* const slots = reinterpret_cast<uint4*>(base);
        // block bk = K 32 bk + [0, 32) is half (bk >> 1) of lane groups 2 (bk & 1) + e, e = 0, 1: their values 16 (bk >> 1) + [0, 16)
        const int half = bk >> 1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int kgx = 2 * (bk & 1) + e;
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {             // k-step 2 half + ss takes values 8 ss .. 8 ss + 7 of this half
                unsigned p[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned a = __builtin_bit_cast(unsigned short, (_Float16)hi[16 * e + 8 * ss + 2 * q]);
                    const unsigned b = __builtin_bit_cast(unsigned short, (_Float16)hi[16 * e + 8 * ss + 2 * q + 1]);
                    p[q] = a | (b << 16);
                }
                slots[((2 * half + ss) * 4 + kgx) * 80 + r] = make_uint4(p[0], p[1], p[2], p[3]);
            }
        }
        const int xh = f8c_e8m0(ah), xl = f8c_e8m0(al);
        const v8i ch = f8c_codes(hi, f8c_inv_scale(xh)), cl = f8c_codes(lo, f8c_inv_scale(xl));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int kgx = 2 * (bk & 1) + e;
            slots[1280 + (half * 4 + kgx) * 80 + r] = make_uint4(ch[4 * e], ch[4 * e + 1], ch[4 * e + 2], ch[4 * e + 3]);
            slots[1920 + (half * 4 + kgx) * 80 + r] = make_uint4(cl[4 * e], cl[4 * e + 1], cl[4 * e + 2], cl[4 * e + 3]);
        }
        unsigned char* const sc = base + 40960;          // read by lane group bk: the group that supplies block bk's scale
        sc[((0 * 4 + bk) * 16 + (r & 15)) * 8 + (r >> 4)] = (unsigned char)xh;
        sc[((1 * 4 + bk) * 16 + (r & 15)) * 8 + (r >> 4)] = (unsigned char)xl;
        if (r < 16) {                                    // the padding bytes 5 .. 7 of each 8-byte record: zero, deterministically
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int b = 5; b < 8; ++b) sc[((p * 4 + bk) * 16 + r) * 8 + b] = 0;
        }
    }
}

// Strip-mined projection kernel on that image: gemm_bf16x6s_kernel<NSUB, true, ., .>'s structure (strip images go global -> LDS by
// LDS-DMA into a ring, the activations are split in the kernel, float4 epilogue with bias, K3 addend and segments, row lists,
// the range flag) with 128-deep K tiles.  Eight waves stacked along M (16 rows each: a 128 x 80 NSUB tile per workgroup) share a
// ring of two 41 KB images (one workgroup per CU, two waves per SIMD).  The activations do not pass through LDS: a lane's 32
// K values of its row are two 64-byte runs (the four k groups of a row: two 256-byte runs), loaded as eight float4 one K tile ahead.
// Any M: rows past M (or past *nrows_dev) are clamped copies of the last row, computed and never stored.
template <int NSUB>
__global__ void __launch_bounds__(512, 1) gemm_f16f8c_kernel(const GemmArgs g) {
    constexpr int NT = 5, WAVES = 8, TROWS = 16 * WAVES;
    constexpr int IMG_I = (F8C_PIECES + WAVES - 1) / WAVES;   // DMA instructions per wave and image (the last piece repeats)
    constexpr int SLOTS = F8C_IMG_BYTES / 16;
    __shared__ uint4 Bs[2][SLOTS];

    const int Mv = g.nrows_dev ? __builtin_amdgcn_readfirstlane(*g.nrows_dev) : g.M;
    if (g.exec_rows && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(g.exec_rows, (unsigned long long)Mv);
    const int total = ((Mv + TROWS - 1) / TROWS) * g.ntiles;
    const int chunk = (total + 7) >> 3;
    if ((int)(blockIdx.x >> 3) >= chunk) return;
    const int tile = (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
    if (tile >= total) return;
    const int mtile = tile / g.ntiles, ntile = tile - mtile * g.ntiles;

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int kg = lane >> 4, lr = lane & 15;
    const int m0 = mtile * TROWS;
    const int strip0 = ntile * NSUB;
    const int KT = (g.K + 127) >> 7;
    const int nsteps = KT * NSUB;
    const unsigned ldsB = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)&Bs[0][0];
    const char* const wimg = reinterpret_cast<const char*>(g.wsplit);
    const unsigned wlane = (unsigned)lane * 16u;
    const int wu = __builtin_amdgcn_readfirstlane(wm);

    auto issue_b = [&](int step) {           // strip image of step (kt, s) -> Bs[step & 1]
        const int kt = step / NSUB, s = step - kt * NSUB;
        const char* src = wimg + ((long)(strip0 + s) * KT + kt) * F8C_IMG_BYTES;
#pragma unroll
        for (int k = 0; k < IMG_I; ++k) {
            int q = wu + WAVES * k;
            q = q < F8C_PIECES ? q : F8C_PIECES - 1;
            lds_dma16_s(src + q * 1024, wlane, ldsB + (unsigned)((step & 1) * F8C_IMG_BYTES + q * 1024));
        }
    };
    // this lane's activation row (clamped; through the row list when there is one)
    int gma = m0 + wm * 16 + lr;
    gma = gma < Mv ? gma : Mv - 1;
    if (g.rowidx) gma = g.rowidx[gma];
    const float* const arow = g.a0 + (long)gma * g.lda0 + kg * 16;
    float4 xr[8];                            // values 4 i .. 4 i + 3: K 16 kg + 4 i (i < 4), K 64 + 16 kg + 4 (i - 4) (i >= 4)
    auto load_x = [&](int kt) {              // K % 4 == 0: a float4 is wholly inside K or wholly past it (zero)
        const float* p = arow + kt * 128;
        if (kt * 128 + 128 <= g.K) {
#pragma unroll
            for (int i = 0; i < 8; ++i) xr[i] = *reinterpret_cast<const float4*>(p + 4 * i + (i >= 4 ? 48 : 0));
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ko = 4 * i + (i >= 4 ? 48 : 0);
                xr[i] = kt * 128 + kg * 16 + ko < g.K ? *reinterpret_cast<const float4*>(p + ko) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    float amax = 0.f;                        // largest |activation| x 2^4 this lane has split (range flag)
    bf16x8 xh[4];                            // x_hi, fp16, k-step s (bf16x8: storage type only)
    v8i xq1, xq2;                            // q(x_hi), q(x_lo)
    int xsc = 0;                             // E8M0 of q(x_hi) in byte 0, of q(x_lo) in byte 1
    auto split_x = [&]() {
        constexpr float xs = F16_ACT_SCALE;
        float hi[32], lo[32];
        unsigned xhw[16];
        float ah[2] = {0.f, 0.f}, al[2] = {0.f, 0.f};       // per half of the lane's values (= its share of one MX block each)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v[4] = {xr[i].x * xs, xr[i].y * xs, xr[i].z * xs, xr[i].w * xs};
            amax = fmaxf(fmaxf(amax, fabsf(v[0])), fabsf(v[1])); amax = fmaxf(fmaxf(amax, fabsf(v[2])), fabsf(v[3]));
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const unsigned hb = pack_half_rtz(v[2 * e], v[2 * e + 1]);      // x_hi: fp16, round toward zero (as fp16x3)
                const fp16x2 h = __builtin_bit_cast(fp16x2, hb);
                hi[4 * i + 2 * e] = (float)h[0]; hi[4 * i + 2 * e + 1] = (float)h[1];
                xhw[(i >> 1) * 4 + (i & 1) * 2 + e] = hb;                       // k-step i >> 1, dword (i & 1) * 2 + e of it
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lo[4 * i + e] = v[e] - hi[4 * i + e];                          // exact
                ah[i >> 2] = fmaxf(ah[i >> 2], fabsf(hi[4 * i + e])); al[i >> 2] = fmaxf(al[i >> 2], fabsf(lo[4 * i + e]));
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) xh[k] = __builtin_bit_cast(bf16x8, make_uint4(xhw[4 * k], xhw[4 * k + 1], xhw[4 * k + 2], xhw[4 * k + 3]));
        // a block's other 16 values are in lane l ^ 16
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ah[h] = fmaxf(ah[h], __shfl_xor(ah[h], 16, 64));
            al[h] = fmaxf(al[h], __shfl_xor(al[h], 16, 64));
        }
        const int eh0 = f8c_e8m0(ah[0]), eh1 = f8c_e8m0(ah[1]), el0 = f8c_e8m0(al[0]), el1 = f8c_e8m0(al[1]);
        xq1 = f8c_codes2(hi, f8c_inv_scale(eh0), f8c_inv_scale(eh1));
        xq2 = f8c_codes2(lo, f8c_inv_scale(el0), f8c_inv_scale(el1));
        // lane group g supplies block g's scale: groups 0 / 3 hold it (their pair's low / high half), groups 1 / 2 take it from
        // the other pair (l ^ 48)
        const int mine = eh0 | (eh1 << 8) | (el0 << 16) | (el1 << 24);
        const int other = __shfl_xor(mine, 48, 64);
        const int w = (kg == 0 || kg == 3) ? mine : other;
        const int sh = kg < 2 ? 0 : 8;                   // groups 0, 1: low halves; 2, 3: high halves
        xsc = ((w >> sh) & 0xff) | (((w >> (16 + sh)) & 0xff) << 8);
    };

    v4f acc[NSUB][NT];
#pragma unroll
    for (int s = 0; s < NSUB; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[s][nt] = (v4f){0.f, 0.f, 0.f, 0.f};

    load_x(0);
    issue_b(0);
    for (int kt = 0; kt < KT; ++kt) {
        const int krel = g.K - kt * 128;
        const int nks = krel >= 32 ? 4 : (krel + 7) >> 3;        // fp16 k-steps that meet a K value below K (the tail skips the rest)
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
            const int step = kt * NSUB + s;
            // the queue holds image(step) and (s == 0) this K tile's activations: both needed now
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                          // landed for every wave; image(step - 1)'s buffer is free
            if (s == 0) split_x();
            if (step + 1 < nsteps) issue_b(step + 1);
            if (s == NSUB - 1 && kt + 1 < KT) load_x(kt + 1);       // in flight under this step's MFMAs
            const uint4* Bi = Bs[step & 1];
            const int lslot = kg * 80 + lr;
            const uint2 sch = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(Bi) + 40960 + ((0 * 4 + kg) * 16 + lr) * 8);
            const uint2 scl = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(Bi) + 40960 + ((1 * 4 + kg) * 16 + lr) * 8);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int sl = lslot + nt * 16;
                const uint4 q1a = Bi[1280 + sl], q1b = Bi[1280 + 320 + sl];
                const uint4 q2a = Bi[1920 + sl], q2b = Bi[1920 + 320 + sl];
                const v8i wq1 = (v8i){(int)q1a.x, (int)q1a.y, (int)q1a.z, (int)q1a.w, (int)q1b.x, (int)q1b.y, (int)q1b.z, (int)q1b.w};
                const v8i wq2 = (v8i){(int)q2a.x, (int)q2a.y, (int)q2a.z, (int)q2a.w, (int)q2b.x, (int)q2b.y, (int)q2b.z, (int)q2b.w};
                const int sh = (int)(nt < 4 ? sch.x : sch.y), sl8 = (int)(nt < 4 ? scl.x : scl.y);
                v4f c = acc[s][nt];
                // the corrections first (small terms), then the leading product; byte (nt & 3) of the weights' scale word
                c = f8c_mma<0>(nt & 3, wq2, xq1, c, sl8, xsc);    // q(w_lo) q(x_hi)
                c = f8c_mma<1>(nt & 3, wq1, xq2, c, sh, xsc);     // q(w_hi) q(x_lo)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < nks) {
                        const bf16x8 wh = __builtin_bit_cast(bf16x8, Bi[ks * 320 + sl]);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, wh), __builtin_bit_cast(half8, xh[ks]), c, 0, 0, 0);
                    }
                }
                acc[s][nt] = c;
            }
        }
    }

    if (g.range_flag && __builtin_amdgcn_ballot_w64(!(amax < 65504.f)) != 0 && lane == 0) atomicOr(g.range_flag, 1u);
    // epilogue as gemm_bf16x6s_kernel's (fp32 outputs only): a lane holds four consecutive output columns of one row
    const int gv = m0 + wm * 16 + lr;
    const bool rok = gv < Mv;
    const int gvc = rok ? gv : Mv - 1;
    const int gm = (g.rowidx && !g.gather_only) ? g.rowidx[gvc] : gvc;
    const bool has_e0 = g.epi == EPI_RELU_RES || g.epi == EPI_ADD_E0;
    constexpr float u = 1.f / (F16_WEIGHT_SCALE * F16_ACT_SCALE);      // the operands carry 2^10 and 2^4
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        const int ncol0 = (strip0 + s) * 80;
        const int seg = ncol0 / g.nseg;
        const int nbase = ncol0 - seg * g.nseg + kg * 4;
        const float* const bp = g.bias[seg];
        const bool radd_here = g.radd && seg == g.radd_seg;
        float* const yrow = g.y[seg] + (long)gm * g.ldy;
        float4 bv[NT], rv[NT], ev[NT];
        if (bp) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(bp + nbase + nt * 16);
        }
        if (radd_here) {
            const float* rrow = g.radd + (long)(gm / g.rows_per_b) * g.nseg + nbase;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) rv[nt] = *reinterpret_cast<const float4*>(rrow + nt * 16);
        }
        if (has_e0) {
            const float* erow = g.e0 + (long)gm * g.lde0 + nbase;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) ev[nt] = *reinterpret_cast<const float4*>(erow + nt * 16);
        } else if (g.epi == EPI_ACCUM) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) ev[nt] = *reinterpret_cast<const float4*>(yrow + nbase + nt * 16);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const v4f a = acc[s][nt];
            float4 v = make_float4(a[0] * u, a[1] * u, a[2] * u, a[3] * u);
            if (bp) v = f4_add(v, bv[nt]);
            if (radd_here) v = f4_add(rv[nt], v);
            if (g.epi == EPI_RELU_RES) {
                const float4 x = ev[nt];
                v = make_float4(fmaxf(v.x, 0.f) + x.x, fmaxf(v.y, 0.f) + x.y, fmaxf(v.z, 0.f) + x.z, fmaxf(v.w, 0.f) + x.w);
            }
            if (g.epi == EPI_ACCUM || g.epi == EPI_ADD_E0) v = f4_add(ev[nt], v);
            if (rok) *reinterpret_cast<float4*>(yrow + nbase + nt * 16) = v;
        }
    }
}

// The split format of the strip-mined kernel's operands — 0 = three bf16 pieces, six products (fp32-grade); 1 = two fp16 pieces,
// three products (gemm_bf16x6s_kernel<., true, ., .>) — is a property of the split IMAGE: whoever splits the weights says which
// (GemmArgs.format travels with GemmArgs.wsplit; digat_params.flags & DIGAT_PARAMS_GEMM_F16X3 for the encoder's images), there is no
// process-wide setting.  Every split records its image's format here and every launch checks it, so an image can never be read
// by the other format's kernel (DIGAT_ERR_ARG).  The training entries split their weights per call, always in format 0:
// gradients have no lower bound (1e-6 and below is ordinary) and fp16 pieces of such values are subnormal or zero.
static std::mutex g_wsplit_mu;
static std::unordered_map<const void*, int> g_wsplit_format;
static void wsplit_note(const void* image, int format) {
    std::lock_guard<std::mutex> lock(g_wsplit_mu);
    g_wsplit_format[image] = format;
}
static int wsplit_forget(const void* image) {              // the buffer is about to be freed / reused: its address means nothing any more
    std::lock_guard<std::mutex> lock(g_wsplit_mu);
    return g_wsplit_format.erase(image) ? 1 : 0;
}
static int wsplit_format_of(const void* image) {          // -1: not an image this library has split
    std::lock_guard<std::mutex> lock(g_wsplit_mu);
    const auto it = g_wsplit_format.find(image);
    return it == g_wsplit_format.end() ? -1 : it->second;
}
// compulsory HBM bytes of a launch per row of A: the row itself, its results (fp32, bf16 or block-scaled e4m3 per segment) and
// the epilogue's row operands; the weights (a few hundred KB, L2-resident) are not counted
static double gemm_row_bytes(const GemmArgs& g) {
    double out = 0.0;
    for (int sgm = 0; sgm < g.nsegs; ++sgm)
        out += ((g.fp8_segs >> sgm) & 1) ? (double)g.nseg + 4.0 * (g.nseg / 80) : (((g.bf16_segs >> sgm) & 1) ? 2.0 * g.nseg : 4.0 * g.nseg);
    double in = 4.0 * g.K;
    if (g.epi == EPI_RELU_RES || g.epi == EPI_ADD_E0 || g.epi == EPI_ACCUM) in += 4.0 * g.nseg;
    if (g.epi == EPI_GATE) in += 4.0 * g.nseg * (g.e2 ? 3 : 2);
    if (g.radd) in += 4.0 * g.nseg / (g.rows_per_b > 0 ? g.rows_per_b : 1);
    return in + out;
}

// Every GEMM launch: gemm_plan (digat_gemm_plan.h) decides the kernel, its tiles and grid, and what is refused
static int launch_gemm(GemmArgs g, hipStream_t st, int kind = DIGAT_KERNEL_LINEAR) {
    if (g.M <= 0) return DIGAT_OK;
    const GemmPlan p = gemm_plan(g, kind);
    if (p.status) return p.status;
    if (p.kernel == GEMM_PER_SEGMENT) {
        for (int sgm = 0; sgm < g.nsegs; ++sgm) {
            GemmArgs one = g;
            one.w[0] = g.w[sgm]; one.bias[0] = g.bias[sgm]; one.y[0] = g.y[sgm]; one.nsegs = 1;
            if (sgm == g.radd_seg) one.radd_seg = 0; else one.radd = nullptr;
            const int rc = launch_gemm(one, st, kind);
            if (rc) return rc;
        }
        return DIGAT_OK;
    }
    if (p.image_format >= 0) {
        const int made_as = wsplit_format_of(g.wsplit);
        if (made_as >= 0 && made_as != p.image_format) return DIGAT_ERR_ARG;       // the image was split for another kernel
    }
    // a row-list launch does the work of its live rows only: the kernel adds that count to a device counter and
    // digat_profile_stop prices it; the launch itself is recorded with zero work
    const int Ntot = g.nseg * g.nsegs;
    const bool listed = g.rowidx != nullptr && !g.gather_only;
    if (listed && g_prof.enabled) {
        g.exec_rows = g_prof.rows_dev + kind;
        g_prof.flops_per_row[kind] = 2.0 * (double)Ntot * g.K; g_prof.rows_nominal[kind] += g.M;
        g_prof.bytes_per_row[kind] = gemm_row_bytes(g);
    }
    ProfScope prof(kind, listed ? 0.0 : 2.0 * g.M * (double)Ntot * g.K, st, listed ? 0.0 : (double)g.M * gemm_row_bytes(g));
    g.mtiles = p.mtiles; g.ntiles = p.ntiles;
    g.ragged = p.ragged; g.strips = p.ragged ? Ntot / 80 : 0;
    if (p.ragged) {          // the chosen kernel's ragged instantiation (the same symbol with RAG = true)
        void (*ragged)(const GemmArgs) = nullptr;
        if (p.kernel == GEMM_STRIP_3_F16_FULL) ragged = gemm_bf16x6s_kernel<3, true, 2, true, true>;
        else if (p.kernel == GEMM_STRIP_3_F16) ragged = gemm_bf16x6s_kernel<3, true, 2, false, true>;
        else if (p.kernel == GEMM_STRIP_3_BF16) ragged = gemm_bf16x6s_kernel<3, false, 2, false, true>;
        else return DIGAT_ERR_ARG;
        hipLaunchKernelGGL(ragged, dim3(p.grid), dim3(p.block), 0, st, g);
        DIGAT_CHECK_LAUNCH();
        return DIGAT_OK;
    }
    switch (p.kernel) {
#define DIGAT_GEMM_LAUNCH(id, ...) case GEMM_##id: hipLaunchKernelGGL((__VA_ARGS__), dim3(p.grid), dim3(p.block), 0, st, g); break;
        DIGAT_GEMM_KERNELS(DIGAT_GEMM_LAUNCH)
#undef DIGAT_GEMM_LAUNCH
        default: return DIGAT_ERR_ARG;
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

static GemmArgs gemm_plain(const float* x, long ldx, const float* w, const float* b, float* y, long ldy,
                           int M, int N, int K, int transW) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.a0 = x; g.lda0 = ldx; g.k0 = K; g.a1 = nullptr; g.lda1 = 0;
    g.w[0] = w; g.bias[0] = b; g.y[0] = y; g.ldy = ldy;
    g.nseg = N; g.nsegs = 1; g.M = M; g.K = K; g.transW = transW; g.epi = EPI_NONE;
    return g;
}

