// digat_ctxfused.inc — compute_user_graph_context (graphEncoders.py:123-134) as ONE launch (round 6).
// Included by digat_kernels.hip.
//
// The inference path ran it as three launches — topic pooling (topic_pool_resident_kernel: scatter_softmax + scatter_sum of :126-130),
// featureAffine on the unmasked buckets (the one-strip projection GEMM: T' = relu(T Fa^T + b) + T of :131) and the SDPA pooling of :133
// (attn_pool_resident_kernel) — with the pooled topics T [B,C+1,d] and T' crossing HBM four times per call, four calls per pass:
// 0.73 ms of a 3.3 ms pass solo, and the kinds that inflate most when passes share the chip (VERDICT r05 weak 6).
// Here a workgroup of seven waves (wave w owns channels 64 w .. 64 w + 63) takes R = 4 rows through all three steps:
//  1. topic pooling of one row at a time, exactly topic_pool_resident_kernel's arithmetic (rows of the next history in flight while
//     the current one is pooled); the categories that occur AND can carry weight (unmasked, or every one when the row has no
//     unmasked category: the attention is uniform then) are numbered densely into 16 SLOTS of the row's tile; a lane ends with
//     T[slot 4 lq + r][channel 64 w + 4 lr + s] (the fp32 MFMA's output layout) and also stores it to LDS as the two scaled fp16
//     pieces of the fp16x3 format ([slot][8-channel group] 16-byte pieces, hi and lo planes);
//  2. featureAffine on the matrix cores for the R tiles at once (M = 16 R slots): T from LDS is the MFMA's ROW operand and the
//     weights — a lane-ordered image made once per weight version (split_weights_ctxfused_kernel: column j of the wave's tile s is
//     output channel 64 w + 4 j + s) — stream global -> registers as its COLUMN operand, so the product lands in the layout of
//     step 1 and the residual T is the lane's own fp32 registers: bias, ReLU and "+ T" are the GEMM epilogue's, bit for bit;
//     the three fp16 products per K tile go in the GEMM's order (lo.hi, hi.lo, hi.hi);
//  3. the SDPA pooling over the C + 1 buckets from registers: slot scores are channel sums over lanes and waves, a bucket without a
//     slot is relu(b) (its T is zero: no history row has the category), masked buckets weigh exactly 0, out = sum + addend.
// T and T' never leave the CU.  A row with more than 16 slots (17 categories all read, or 18 buckets under an all-false mask) keeps
// its slots 16 .. 19 in a fifth tile shared by the R rows, computed by a second pass over the weights that only such workgroups run
// (its residual is rebuilt from the two fp16 pieces: 22 bits).  Shapes: H <= 52, d <= 448, d % 8 == 0, C + 1 <= 20, fp16x3 format
// (the caller falls back to the three launches otherwise).
struct CtxFusedArgs {
    const float* Xu; long ld_b; const int* group; const uint8_t* live; int live_ld; const int* hlast;
    const float* kq_topic; const float* kq_user; const int64_t* idx; const uint8_t* cat_mask; const float* addend; float* out;
    const uint4* wimg; const float* bFa; unsigned* range_flag;
    int B, H, C1, d; float sqrt_d;
};
constexpr int CF_R = 4;                  // rows per workgroup
constexpr int CF_STEPS = 13;             // 4-row steps of a history held in registers: H <= 52
constexpr int CF_MAXC = 20;              // buckets (C + 1): 16 slots + 4 overflow slots per row
constexpr int CF_OV = 4;                 // overflow slots per row (the fifth tile holds R x 4)

__host__ __device__ constexpr int cf_kt(int d) { return (d + 31) >> 5; }
__host__ __device__ constexpr int cf_kgp(int d) { return (4 * cf_kt(d)) | 1; }        // 16-byte pieces per slot row in LDS: odd (bank spread), >= 4 KT
static size_t ctxfused_image_bytes(int d) { return (size_t)((d + 63) / 64) * 4 * cf_kt(d) * 2 * 64 * 16; }
static size_t ctxfused_lds_bytes(int d, int H) {
    (void)H;
    const size_t kgp = cf_kgp(d);
    return (size_t)(CF_R * 16 + 16) * kgp * 16 * 2            // T tiles (hi, lo) + the overflow tile
           + (size_t)2 * 7 * 64 * 4                           // part [2][7][64]
           + (size_t)CF_R * 64 * 8                            // (alpha, slot) per history row
           + (size_t)CF_R * (64 + 64 + 24 + 32) * 4           // sidx, slive, scat, per-row info
           + (size_t)7 * CF_R * 24 * 4 + (size_t)CF_R * 24 * 4;   // part3, alpha3
}

// the weights in the fused kernel's lane order: slot (((w 4 + s) KT + kt) 2 + plane) 64 + kq 16 + j  holds the eight halfs
// W[n = 64 w + 4 j + s][k = 32 kt + 8 kq + e] x 2^10 (plane 0: rounded to fp16; plane 1: the remainder, rounded — the pieces of
// split_weights_tiled_kernel's fp16x3 format), zero past d
__global__ void __launch_bounds__(256) split_weights_ctxfused_kernel(const float* W, int d, uint4* out) {
    const int KT = cf_kt(d), groups = (d + 63) / 64;
    const long total = (long)groups * 4 * KT * 2 * 64;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int lane = (int)(i & 63), plane = (int)((i >> 6) & 1);
        const long rest = i >> 7;
        const int kt = (int)(rest % KT), ws = (int)(rest / KT), s = ws & 3, w = ws >> 2;
        const int kq = lane >> 4, j = lane & 15, n = 64 * w + 4 * j + s;
        unsigned short h8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 32 * kt + 8 * kq + e;
            const float vs = (n < d && k < d) ? W[(long)n * d + k] * F16_WEIGHT_SCALE : 0.f;
            const _Float16 h = (_Float16)vs;
            const _Float16 l = (_Float16)(vs - (float)h);
            h8[e] = plane ? __builtin_bit_cast(unsigned short, l) : __builtin_bit_cast(unsigned short, h);
        }
        out[i] = make_uint4(h8[0] | ((unsigned)h8[1] << 16), h8[2] | ((unsigned)h8[3] << 16), h8[4] | ((unsigned)h8[5] << 16), h8[6] | ((unsigned)h8[7] << 16));
    }
}

// sum over the four 16-lane rows of a wave, result in every lane (v_permlane16_swap / v_permlane32_swap by inline asm: hipcc of
// ROCm 7.2 reads both results of the builtins from the first register — tools/exp/eq8_packed/README.md)
__device__ __forceinline__ float cf_rows_sum(const float v) {
    float x = v, y = v;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    const float s = x + y;
    float x2 = s, y2 = s;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x2), "+v"(y2));
    return x2 + y2;
}
__device__ __forceinline__ float cf_row16_sum(float p) {      // sum over the 16 lanes of a row, in every lane of it
    p += dpp_mov<0xB1>(p); p += dpp_mov<0x4E>(p); p += dpp_mov<0x141>(p); p += dpp_mov<0x140>(p);
    return p;
}
// four consecutive channels -> their two scaled fp16 pieces (gemm_bf16x6s_kernel<., true, ., .>::split_mt's arithmetic), 8 bytes each
__device__ __forceinline__ void cf_split4(const float a, const float b, const float c, const float d4, uint2& hi, uint2& lo, float& amax) {
    constexpr float xs = F16_ACT_SCALE;
    const float s0 = a * xs, s1 = b * xs, s2 = c * xs, s3 = d4 * xs;
    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(s0), fabsf(s1))), fmaxf(fabsf(s2), fabsf(s3)));
    const unsigned h01 = pack_half_rtz(s0, s1), h23 = pack_half_rtz(s2, s3);
    const fp16x2 p = __builtin_bit_cast(fp16x2, h01), q = __builtin_bit_cast(fp16x2, h23);
    const _Float16 l0 = (_Float16)__builtin_fmaf(a, xs, -(float)p[0]), l1 = (_Float16)__builtin_fmaf(b, xs, -(float)p[1]);
    const _Float16 l2 = (_Float16)__builtin_fmaf(c, xs, -(float)q[0]), l3 = (_Float16)__builtin_fmaf(d4, xs, -(float)q[1]);
    hi = make_uint2(h01, h23);
    lo = make_uint2((unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16),
                    (unsigned)__builtin_bit_cast(unsigned short, l2) | ((unsigned)__builtin_bit_cast(unsigned short, l3) << 16));
}

#ifdef DIGAT_CF_TIMERS
// experiment builds only (tools/exp/cf_lab.py): cycles of wave 0 of every workgroup between the stamps below; [15] = workgroups
__device__ unsigned long long g_cf_timers[16];
#define CF_T(k) do { if (tid == 0) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); atomicAdd(&g_cf_timers[k], t__ - cf_last); cf_last = t__; } } while (0)
#else
#define CF_T(k) do {} while (0)
#endif
__global__ void __launch_bounds__(448) user_ctx_fused_kernel(const CtxFusedArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cf_smem[];
    constexpr int R = CF_R, STEPS = CF_STEPS;
    const int H = g.H, hs = H | 1, C1 = g.C1, d = g.d;
    const int KT = cf_kt(d), KGP = cf_kgp(d);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int nw = (int)(blockDim.x >> 6);
    // ---- LDS ----
    uint4* const Th = reinterpret_cast<uint4*>(cf_smem);                       // [R*16 + 16][KGP]: rows R*16 .. : the overflow tile
    uint4* const Tl = Th + (size_t)(R * 16 + 16) * KGP;
    float* const part = reinterpret_cast<float*>(Tl + (size_t)(R * 16 + 16) * KGP);   // [2][7][64] partial scores: rows alternate between the two
    float2* const aslot = reinterpret_cast<float2*>(part + 2 * 7 * 64);        // [R][64]: (alpha_t, slot of t as a float; -1: none) of history row t
    int* const sidx = reinterpret_cast<int*>(aslot + R * 64);                  // [R][64] category of history slot t (-1: none)
    int* const slive = sidx + R * 64;                                          // [R][64]
    int* const scat = slive + R * 64;                                          // [R][24] slot -> category
    int* const rinfo = scat + R * 24;                                          // [R][32]: [c] = slot of bucket c (-1: none) .. [24] = slots, [25] = mask bits
    float* const part3 = reinterpret_cast<float*>(rinfo + R * 32);             // [7][R][24]: [slot 0..19] scores, [20] = relu(b) . kq
    float* const alpha3 = part3 + 7 * R * 24;                                  // [R][24]: [slot] weights, [20] = weight of the buckets without a slot

#ifdef DIGAT_CF_TIMERS
    unsigned long long cf_last = __builtin_amdgcn_s_memtime();
#endif
    const int b0 = blockIdx.x * R;
    const int ch = wave * 64 + 4 * lr;
    const bool ch_ok = ch < d;
    const int nsteps = (H + 3) >> 2;
    float amax = 0.f;

    // the padding pieces of the tiles' rows (K tiles reach past d; the weights there are zero, the activations must be finite)
    for (int i = tid; i < (R * 16 + 16) * (KGP - d / 8); i += blockDim.x) {
        const int row = i / (KGP - d / 8), kg = d / 8 + i % (KGP - d / 8);
        Th[(size_t)row * KGP + kg] = make_uint4(0, 0, 0, 0);
        Tl[(size_t)row * KGP + kg] = make_uint4(0, 0, 0, 0);
    }

    v4f Treg[R][4];                       // T of the rows' tiles: [row][channel tile s][slot 4 lq + r]
    bool any_ov = false;                  // some row of this workgroup has more than 16 slots (wave-uniform)

    // ---- 1. topic pooling, one row at a time; the history of the next row is in flight while the current one is pooled ----
    auto row_of = [&](int r) { return min(b0 + r, g.B - 1); };
    auto load_row = [&](int r, float4 (&xq)[STEPS], float4& k4) {
        const int b = row_of(r);
        const float* Xb = g.Xu + (long)(g.group ? g.group[b] : b) * g.ld_b;
        const int nl = (g.live && g.hlast) ? min(g.hlast[b], H) : H;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int j = s * 4 + lq;
            const int jr = min(j, nl > 0 ? nl - 1 : 0);       // rows past the last live one: redirected (dropped by the flag select)
            xq[s] = (s < nsteps && j < H && ch_ok) ? *reinterpret_cast<const float4*>(Xb + (long)jr * d + ch) : f4_zero();
        }
        k4 = ch_ok ? *reinterpret_cast<const float4*>(g.kq_topic + (long)b * d + ch) : f4_zero();
    };
    // per row: live-flag select + partial scores -> barrier -> (every wave sums the partial scores for itself) segment softmax of the
    // wave's slots -> barrier -> T = M @ X on the fp32 matrix cores, M[slot][t] built on the fly from (alpha_t, slot of t).  `part`
    // alternates between two buffers: two barriers per row.
    auto pool_row = [&](auto rc, float4 (&xq)[STEPS], const float4 k4) {
        constexpr int r = decltype(rc)::value;           // compile-time: Treg[r] must stay in registers
        const int b = row_of(r);
        float* const pr = part + (r & 1) * 7 * 64;
        if (g.live) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) xq[s] = slive[r * 64 + min(s * 4 + lq, 63)] ? xq[s] : f4_zero();       // a select, never a multiply
        }
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            float p = fmaf(xq[s].w, k4.w, fmaf(xq[s].z, k4.z, fmaf(xq[s].y, k4.y, xq[s].x * k4.x)));
            p = cf_row16_sum(p);
            if (lr == 0) pr[wave * 64 + s * 4 + lq] = p;
        }
        CF_T(9);
        __syncthreads();
        CF_T(10);
        const int nslots = rinfo[r * 32 + 24];
        {
            float a = 0.f;
            for (int w = 0; w < nw; ++w) a += pr[w * 64 + lane];
            const float v = lane < H ? a / g.sqrt_d : 0.f;
            const int my = lane < H ? sidx[r * 64 + lane] : -2;
            for (int sl = wave; sl < nslots; sl += nw) {
                const bool in = my == scat[r * 24 + sl];
                const float m = wave_max(in ? v : -INFINITY);
                const float e = in ? expf(v - m) : 0.f;
                const float den = wave_sum(e);
                if (in) aslot[r * 64 + lane] = make_float2(e / den, (float)sl);
            }
        }
        CF_T(11);
        __syncthreads();
        CF_T(12);
        const int nl = (g.live && g.hlast) ? min(g.hlast[b], H) : H;
        v4f acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (s * 4 < nl) {                    // wave-uniform
                const float2 as = aslot[r * 64 + min(s * 4 + lq, 63)];
                const float av = as.y == (float)lr ? as.x : 0.f;
                const float4 xc = xq[s];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, acc[3], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) Treg[r][s] = acc[s];
        CF_T(13);
        const int kg = 8 * wave + (lr >> 1), half = lr & 1;       // this lane's four channels are half of piece 8 w + lr / 2
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            uint2 hi, lo;
            cf_split4(acc[0][rr], acc[1][rr], acc[2][rr], acc[3][rr], hi, lo, amax);
            if (ch_ok) {
                const size_t at = (size_t)(r * 16 + 4 * lq + rr) * KGP + kg;
                reinterpret_cast<uint2*>(Th + at)[half] = hi;
                reinterpret_cast<uint2*>(Tl + at)[half] = lo;
            }
        }
        if (any_ov) {                            // wave-uniform, rare: slots 16 .. 19 of the rows -> rows 4 r .. 4 r + 3 of the overflow tile
            v4f ov[4];                           // (a row without such slots stores zeros: every row of the tile is defined)
#pragma unroll
            for (int s = 0; s < 4; ++s) ov[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                if (s * 4 < nl) {
                    const float2 as = aslot[r * 64 + min(s * 4 + lq, 63)];
                    const float av = as.y == (float)(16 + lr) ? as.x : 0.f;
                    const float4 xc = xq[s];
                    ov[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, ov[0], 0, 0, 0);
                    ov[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, ov[1], 0, 0, 0);
                    ov[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, ov[2], 0, 0, 0);
                    ov[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, ov[3], 0, 0, 0);
                }
            }
            if (lq == 0 && ch_ok) {              // output rows 0 .. 3 (slots 16 .. 19) sit in the lanes of row 0
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    uint2 hi, lo;
                    cf_split4(ov[0][rr], ov[1][rr], ov[2][rr], ov[3][rr], hi, lo, amax);
                    const size_t at = (size_t)(R * 16 + 4 * r + rr) * KGP + kg;
                    reinterpret_cast<uint2*>(Th + at)[half] = hi;
                    reinterpret_cast<uint2*>(Tl + at)[half] = lo;
                }
            }
        }
    };
    {
        float4 xa[STEPS], xb[STEPS], xc[STEPS], ka, kb, kc;     // three histories in flight (the workgroup is alone on its CU: nothing else hides HBM)
        load_row(0, xa, ka);
        load_row(1, xb, kb);
        load_row(2, xc, kc);
        // while the first rows are in flight: wave r numbers the slots of row r (the categories that occur and can carry weight)
        if (wave < R) {
            const int r = wave, b = row_of(r);
            long v = -1;
            if (lane < H) v = g.idx[(long)b * H + lane];
            const int lv = (g.live && lane < H) ? (int)g.live[(long)b * g.live_ld + lane] : 1;
            const bool mk = lane < C1 && g.cat_mask[(long)b * C1 + lane] != 0;
            const int cat = (v >= 0 && v < C1) ? (int)v : -1;
            sidx[r * 64 + lane] = cat;
            slive[r * 64 + lane] = lv;
            aslot[r * 64 + lane] = make_float2(0.f, -1.f);
            unsigned present = 0u;
            for (int c = 0; c < C1; ++c) present |= __ballot(cat == c) ? (1u << c) : 0u;
            const unsigned maskbits = (unsigned)__ballot(mk);
            const unsigned needed = maskbits ? maskbits : ((1u << C1) - 1u);      // no unmasked category: every bucket weighs 1 / (C + 1)
            const unsigned slotmask = present & needed;
            const bool has = lane < C1 && ((slotmask >> lane) & 1u);
            const int slot = __popc(slotmask & ((1u << lane) - 1u));
            if (has) scat[r * 24 + slot] = lane;
            if (lane < 24) rinfo[r * 32 + lane] = has ? slot : -1;
            if (lane == 0) { rinfo[r * 32 + 24] = __popc(slotmask); rinfo[r * 32 + 25] = (int)maskbits; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) any_ov = any_ov || rinfo[r * 32 + 24] > 16;
        CF_T(0);
        pool_row(std::integral_constant<int, 0>{}, xa, ka);
        CF_T(1);
        load_row(3, xa, ka);
        pool_row(std::integral_constant<int, 1>{}, xb, kb);
        CF_T(2);
        pool_row(std::integral_constant<int, 2>{}, xc, kc);
        CF_T(3);
        pool_row(std::integral_constant<int, 3>{}, xa, ka);
        CF_T(4);
        __syncthreads();                         // the tiles are complete
        CF_T(5);
    }

    // ---- 2. featureAffine: D[slot][channel] = sum_k T[slot][k] Fa[channel][k], three fp16 products per K tile ----
    const uint4* const wim = g.wimg + (size_t)wave * 4 * KT * 128 + lane;       // + ((s KT + kt) 2 + plane) 64
    const int la = lane & 15, kq = lane >> 4;
    auto load_b = [&](int kt, uint4 (&bh)[4], uint4 (&bl)[4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bh[s] = wim[(size_t)((s * KT + kt) * 2) * 64];
            bl[s] = wim[(size_t)((s * KT + kt) * 2 + 1) * 64];
        }
    };
    auto mma = [&](const uint4 a, const uint4 b, const v4f c) -> v4f {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
    };
    constexpr float unscale = 1.f / (F16_WEIGHT_SCALE * F16_ACT_SCALE);
    const float4 bias = ch_ok ? *reinterpret_cast<const float4*>(g.bFa + ch) : f4_zero();
    v4f T2[R][4];
    // two passes over K, channel tiles {0, 1} then {2, 3}: half the accumulators and half the weight fragments of a K tile in
    // registers, so that the weights of THREE K tiles are in flight (with two the loop waited for them: 40 k cycles for 10 k of MFMA
    // issue per wave); the A fragments are read from LDS in both passes
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
        v4f acc[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r) { acc[r][0] = (v4f){0.f, 0.f, 0.f, 0.f}; acc[r][1] = (v4f){0.f, 0.f, 0.f, 0.f}; }
        auto load_b2 = [&](int kt, uint4 (&bh)[2], uint4 (&bl)[2]) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                bh[q] = wim[(size_t)(((2 * hp + q) * KT + kt) * 2) * 64];
                bl[q] = wim[(size_t)(((2 * hp + q) * KT + kt) * 2 + 1) * 64];
            }
        };
        auto step2 = [&](int kt, const uint4 (&bh)[2], const uint4 (&bl)[2]) {
            uint4 ah[R], al[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ah[r] = Th[(size_t)(r * 16 + la) * KGP + 4 * kt + kq];
                al[r] = Tl[(size_t)(r * 16 + la) * KGP + 4 * kt + kq];
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] = mma(al[r], bh[q], acc[r][q]);     // x lo . w hi
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] = mma(ah[r], bl[q], acc[r][q]);     // x hi . w lo
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][q] = mma(ah[r], bh[q], acc[r][q]);     // x hi . w hi
            }
        };
        const int KTX = KT;
        uint4 bh0[2], bl0[2], bh1[2], bl1[2], bh2[2], bl2[2];
        load_b2(0, bh0, bl0);
        if (1 < KTX) load_b2(1, bh1, bl1);
#pragma nounroll
        for (int kt = 0; kt < KTX; kt += 3) {
            if (kt + 2 < KTX) load_b2(kt + 2, bh2, bl2);
            __builtin_amdgcn_sched_barrier(0);
            step2(kt, bh0, bl0);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 1 < KTX) {
                if (kt + 3 < KTX) load_b2(kt + 3, bh0, bl0);
                __builtin_amdgcn_sched_barrier(0);
                step2(kt + 1, bh1, bl1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kt + 2 < KTX) {
                if (kt + 4 < KTX) load_b2(kt + 4, bh1, bl1);
                __builtin_amdgcn_sched_barrier(0);
                step2(kt + 2, bh2, bl2);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the GEMM's epilogue: x u, + b, relu, + T
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int s = 2 * hp + q;
                const float bs = s == 0 ? bias.x : (s == 1 ? bias.y : (s == 2 ? bias.z : bias.w));
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) T2[r][s][rr] = fmaxf(acc[r][q][rr] * unscale + bs, 0.f) + Treg[r][s][rr];
            }
    }
    CF_T(6);
    v4f T2ov[4];                          // the overflow tile: lane row lq = row lq of the workgroup, r = its slot 16 + r
#pragma unroll
    for (int s = 0; s < 4; ++s) T2ov[s] = (v4f){0.f, 0.f, 0.f, 0.f};
    if (any_ov) {                         // wave-uniform, rare: a second pass over the weights for the fifth tile
        v4f acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma nounroll
        for (int kt = 0; kt < KT; ++kt) {
            uint4 bh[4], bl[4];
            load_b(kt, bh, bl);
            const uint4 ah = Th[(size_t)(R * 16 + la) * KGP + 4 * kt + kq], al = Tl[(size_t)(R * 16 + la) * KGP + 4 * kt + kq];
#pragma unroll
            for (int s = 0; s < 4; ++s) { acc[s] = mma(al, bh[s], acc[s]); acc[s] = mma(ah, bl[s], acc[s]); acc[s] = mma(ah, bh[s], acc[s]); }
        }
        // the residual from the two fp16 pieces (22 bits of T): this lane's channels 4 lr .. + 3 of tile rows 4 lq .. + 3
        const int kg = 8 * wave + (lr >> 1), half = lr & 1;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const size_t at = (size_t)(R * 16 + 4 * lq + rr) * KGP + kg;
            const uint2 hi = ch_ok ? reinterpret_cast<const uint2*>(Th + at)[half] : make_uint2(0, 0);
            const uint2 lo = ch_ok ? reinterpret_cast<const uint2*>(Tl + at)[half] : make_uint2(0, 0);
            const unsigned hw[2] = {hi.x, hi.y}, lw[2] = {lo.x, lo.y};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const fp16x2 hp = __builtin_bit_cast(fp16x2, hw[s >> 1]), lp = __builtin_bit_cast(fp16x2, lw[s >> 1]);
                const float t = ((float)hp[s & 1] + (float)lp[s & 1]) * (1.f / F16_ACT_SCALE);
                const float bs = s == 0 ? bias.x : (s == 1 ? bias.y : (s == 2 ? bias.z : bias.w));
                T2ov[s][rr] = fmaxf(acc[s][rr] * unscale + bs, 0.f) + t;
            }
        }
    }

    // ---- 3. SDPA pooling over the buckets (layers.py:199-206): scores, masked softmax, weighted sum of T' ----
    {
        const float4 rb = make_float4(fmaxf(bias.x, 0.f), fmaxf(bias.y, 0.f), fmaxf(bias.z, 0.f), fmaxf(bias.w, 0.f));    // T' of a bucket without rows
        float4 kqv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) kqv[r] = ch_ok ? *reinterpret_cast<const float4*>(g.kq_user + (long)row_of(r) * d + ch) : f4_zero();
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float p = fmaf(T2[r][3][rr], kqv[r].w, fmaf(T2[r][2][rr], kqv[r].z, fmaf(T2[r][1][rr], kqv[r].y, T2[r][0][rr] * kqv[r].x)));
                p = cf_row16_sum(p);
                if (lr == 0) part3[(wave * R + r) * 24 + 4 * lq + rr] = p;
            }
            float pe = fmaf(rb.w, kqv[r].w, fmaf(rb.z, kqv[r].z, fmaf(rb.y, kqv[r].y, rb.x * kqv[r].x)));
            pe = cf_row16_sum(pe);
            if (lane == 0) part3[(wave * R + r) * 24 + 20] = pe;
        }
        if (any_ov) {
            // overflow tile: lane row lq holds workgroup row lq: its query is kqv[lq] (a select over the four registers)
            const float4 kqo = lq == 0 ? kqv[0] : (lq == 1 ? kqv[1] : (lq == 2 ? kqv[2] : kqv[3]));
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float p = fmaf(T2ov[3][rr], kqo.w, fmaf(T2ov[2][rr], kqo.z, fmaf(T2ov[1][rr], kqo.y, T2ov[0][rr] * kqo.x)));
                p = cf_row16_sum(p);
                if (lr == 0) part3[(wave * R + lq) * 24 + 16 + rr] = p;
            }
        }
        __syncthreads();
        CF_T(8);
        // the softmax of row r by wave r (lanes = buckets)
        if (wave < R) {
            const int r = wave;
            const int c = lane;
            const unsigned maskbits = (unsigned)rinfo[r * 32 + 25];
            const int slot = c < C1 ? rinfo[r * 32 + c] : -1;
            float sc = 0.f;
            if (c < C1) {
                const int src = slot >= 0 ? slot : 20;
                for (int w = 0; w < nw; ++w) sc += part3[(w * R + r) * 24 + src];
                sc /= g.sqrt_d;
            }
            const bool unmasked = c < C1 && ((maskbits >> c) & 1u);
            const float v = c < C1 ? (unmasked ? sc : -1e9f) : -INFINITY;
            const float m = wave_max(v);
            const float e = c < C1 ? expf(v - m) : 0.f;
            const float den = wave_sum(e);
            const float al = e / den;
            if (lane < 24) alpha3[r * 24 + lane] = 0.f;
            const float rest = wave_sum((c < C1 && slot < 0) ? al : 0.f);       // the buckets without a slot share relu(b)
            __builtin_amdgcn_wave_barrier();
            if (c < C1 && slot >= 0) alpha3[r * 24 + slot] = al;
            if (lane == 0) alpha3[r * 24 + 20] = rest;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float o[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) o[s] = 0.f;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float al = alpha3[r * 24 + 4 * lq + rr];
#pragma unroll
                for (int s = 0; s < 4; ++s) o[s] = fmaf(al, T2[r][s][rr], o[s]);
            }
            if (any_ov && lq == r) {             // this lane row's overflow slots belong to row r
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float al = alpha3[r * 24 + 16 + rr];
#pragma unroll
                    for (int s = 0; s < 4; ++s) o[s] = fmaf(al, T2ov[s][rr], o[s]);
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) o[s] = cf_rows_sum(o[s]);
            const float rest = alpha3[r * 24 + 20];
            float4 ov = make_float4(fmaf(rest, rb.x, o[0]), fmaf(rest, rb.y, o[1]), fmaf(rest, rb.z, o[2]), fmaf(rest, rb.w, o[3]));
            const int b = b0 + r;
            if (lq == 0 && ch_ok && b < g.B) {
                if (g.addend) ov = f4_add(*reinterpret_cast<const float4*>(g.addend + (long)b * d + ch), ov);
                *reinterpret_cast<float4*>(g.out + (long)b * d + ch) = ov;
            }
        }
    }
    if (g.range_flag && __builtin_amdgcn_ballot_w64(!(amax < 65504.f)) != 0 && lane == 0) atomicOr(g.range_flag, 1u);
    CF_T(9);
#ifdef DIGAT_CF_TIMERS
    if (tid == 0) atomicAdd(&g_cf_timers[15], 1ull);
#endif
}

static bool ctxfused_ok(int H, int C1, int d) {
    return H >= 1 && H <= 4 * CF_STEPS && C1 <= CF_MAXC && d % 8 == 0 && d > 192 && d <= 448;      // >= 4 waves (a wave per row runs the softmax)
}
static int launch_user_ctx_fused(const CtxFusedArgs& g, hipStream_t st) {
    if (g.B == 0) return DIGAT_OK;
    const size_t lds = ctxfused_lds_bytes(g.d, g.H);
    static std::atomic<int> raised{0};
    if (!raised.load()) {
        if (hipFuncSetAttribute((const void*)user_ctx_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
        raised.store(1);
    }
    const int groups = (g.d + 63) / 64;
    ProfScope prof(DIGAT_KERNEL_TOPIC, (double)g.B * ((double)g.H * g.d * 4 + 3.0 * g.d * 4 + g.H * 8.0 + g.C1), st);
    hipLaunchKernelGGL(user_ctx_fused_kernel, dim3((g.B + CF_R - 1) / CF_R), dim3(64 * groups), lds, st, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
