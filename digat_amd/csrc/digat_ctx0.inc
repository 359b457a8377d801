// digat_ctx0.inc — the INITIAL user context in one launch behind a small GEMM (round 8).
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950), after digat_context.inc.
//
// compute_user_graph_context pools the history nodes per category (T), sends the pooled rows through featureAffine
// (T2 = relu(T W^T + b) + T) and pools T2 over the categories.  featureAffine is linear and the weights of a present category
// sum to one, so W (sum_t alpha_t x_t) = sum_t alpha_t (W x_t): at the first call of a pass the history nodes x_t are the INPUT
// rows ue, F x = ue W^T is a GEMM over a few thousand rows (per impression in the grouped entry), and everything behind it is
// local to a row of the batch — T [B, C+1, d] and T2 never leave the chip (three launches and ~590 MB of HBM traffic at
// B = 4096, C + 1 = 18, d = 400 become a GEMM over the groups' rows and the kernel below).
struct Ctx0Args {
    const float* x; const float* fx; long ld_b;     // row b's H history rows: x + g ld_b and F x = fx + g ld_b, g = group ? group[b] : b
    const int* group;
    const float *kq_topic, *kq_user;                // [B,d] each: the two folded queries of the news context
    const int64_t* idx; const uint8_t* mask;        // [B,H] category of every history slot (outside [0,C1): none), [B,C1] bucket mask
    const float *bias, *addend; float* out;         // featureAffine's bias [d]; optional [B,d] added to the result; [B,d]
    int B, H, C1, d; float sqrt_d;
};

// One workgroup per row, one wave per 64 channels (7 waves at d = 400), the structure of topic_pool_resident_kernel:
//  1. the wave's slice of every history row x_t in registers (MFMA operand layout), scores a_t = x_t . kq_topic / sqrt(d) and
//     the segment softmax per present category, exactly as in topic_pool_resident_kernel (same code, same bits) -> M [slots, H]
//     in LDS, the present categories numbered densely (slot = rank among the present ones); a category whose bucket is
//     masked does not count as present (unless every bucket is masked): nothing pooled into it can reach the result (6.);
//  2. T_c = sum_t alpha_t x_t on the fp32 matrix cores (the k-ordered fma chain in ascending t) -> LDS [slots, d];
//  3. the SAME registers are reloaded with the rows F x_t (the 13 float4 cannot be held twice) — step by step under the MFMA
//     chain of the last category tile of 2., as each step's registers fall free — and pooled with the same M:
//     G_c = sum_t alpha_t F x_t, same chain, same order;
//  4. a category with at least one slot: T2_c = relu(G_c + b) + T_c, written over T_c by the lane that made both (no barrier);
//     a category with no slot: T2_c = relu(b) — featureAffine of the zero row the pooling left there;
//  5. bucket scores s_c = T2_c . kq_user / sqrt(d): per wave the partial sum of its 64 channels (16 lanes by DPP), the waves'
//     partial sums added in ascending wave order; a masked bucket scores -1e9; softmax over the C1 buckets in every wave for
//     itself (lane c = bucket c), so an all-masked row gets uniform weights over all C1 buckets, relu(b) buckets included;
//  6. out = (addend +) sum_c w_c T2_c over the buckets in ASCENDING CATEGORY order c = 0 .. C1 - 1, one fma chain per channel;
//     a weight of exactly 0 (a masked bucket: exp(-1e9 - max)) contributes nothing — attn_pool_resident_kernel's rule.
// LDS: M + the score scratch + [C1, d] floats (28.8 KB of 39 KB at the bench shape).  96 registers at 13 steps (the bound asks
// for five waves per SIMD): three workgroups of seven waves per CU, as topic_pool_resident_kernel<13> runs; no scratch.
template <int CTX0_STEPS>
__global__ void __launch_bounds__(CTX0_STEPS > 13 ? 512 : 1024, CTX0_STEPS > 13 ? 1 : 5) user_ctx0_kernel(const Ctx0Args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = g.H, hs = H | 1, C1 = g.C1, d = g.d;
    const int ct = (C1 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = blockDim.x, nw = nthreads >> 6;
    float* M = reinterpret_cast<float*>(smem);               // [ct*16][hs]
    float* part = M + ct * 16 * hs;                          // [nw][64] partial history scores; later partial bucket scores per slot
    float* sa = part + nw * 64;                              // [64]
    int* sidx = reinterpret_cast<int*>(sa + 64);             // [64]
    int* cslot = sidx + 64;                                  // [64] category -> slot (-1: no history slot has it)
    int* scat = cslot + 64;                                  // [68] slot -> category; [64] = number of slots, [65] = 1 + last used history row
    float* pe = reinterpret_cast<float*>(scat + 68);         // [16] per wave: partial score of a bucket no history slot has
    float* Tl = pe + 16;                                     // [C1][d] T_c, then T2_c, by slot (ctx0_lds_bytes: the same sum)
    const int b = blockIdx.x;
    const long gb = (long)(g.group ? g.group[b] : b) * g.ld_b;
    const float* Xb = g.x + gb;
    const float* Fb = g.fx + gb;
    const int lr = lane & 15, lq = lane >> 4;
    const int ch = wave * 64 + 4 * lr;
    const bool ch_ok = ch < d;               // no early exit: the MFMAs need every lane's operand rows
    const int nsteps = (H + 3) >> 2;

    float4 xq[CTX0_STEPS];
#pragma unroll
    for (int s = 0; s < CTX0_STEPS; ++s) {
        const int j = s * 4 + lq;
        xq[s] = (s < nsteps && j < H && ch_ok) ? *reinterpret_cast<const float4*>(Xb + (long)j * d + ch) : f4_zero();
    }
    const float4 k4 = ch_ok ? *reinterpret_cast<const float4*>(g.kq_topic + (long)b * d + ch) : f4_zero();
    if (tid < 64) {
        long v = -1;
        if (tid < H) v = g.idx[(long)b * H + tid];
        // A masked bucket weighs exactly 0 in 6. unless EVERY bucket is masked (uniform weights then), so whatever is pooled into
        // it is never read: its history slots count as slots without a category — no tile row, no MFMA step, no second fetch.
        // On MIND-shaped users that is the right-padding of the history (the padding category's bucket is masked): ~60 % of the rows.
        const unsigned long long mb = __ballot(tid < C1 && g.mask[(long)b * C1 + min(tid, C1 - 1)] != 0);
        const int cat = (v >= 0 && v < C1 && (mb == 0ull || ((mb >> v) & 1ull))) ? (int)v : -1;
        sidx[tid] = cat;
        unsigned long long present = 0ull;                   // wave 0: which categories occur (C1 <= 64 ballots, scalar)
        for (int c = 0; c < C1; ++c) present |= __ballot(cat == c) ? (1ull << c) : 0ull;
        const bool has = tid < C1 && ((present >> tid) & 1ull);
        const int slot = __popcll(present & ((1ull << tid) - 1ull));
        cslot[tid] = has ? slot : -1;
        if (has) scat[slot] = tid;
        const unsigned long long used = __ballot(cat >= 0);  // history rows that reach the result
        if (tid == 0) { scat[64] = __popcll(present); scat[65] = used ? 64 - __clzll(used) : 0; }
    }
    for (int i = tid; i < ct * 16 * hs; i += nthreads) M[i] = 0.f;

    // partial scores of this wave's 64 channels (topic_pool_resident_kernel's expression and order)
#pragma unroll
    for (int s = 0; s < CTX0_STEPS; ++s) {
        float p = fmaf(xq[s].w, k4.w, fmaf(xq[s].z, k4.z, fmaf(xq[s].y, k4.y, xq[s].x * k4.x)));
        p += dpp_mov<0xB1>(p); p += dpp_mov<0x4E>(p); p += dpp_mov<0x141>(p); p += dpp_mov<0x140>(p);
        if (lr == 0) part[wave * 64 + s * 4 + lq] = p;
    }
    __syncthreads();
    if (tid < 64) {
        float a = 0.f;
        for (int w = 0; w < nw; ++w) a += part[w * 64 + tid];
        sa[tid] = a / g.sqrt_d;
    }
    __syncthreads();
    // segment softmax: wave w takes the slots w, w + nw, ...; lane t is history row t
    {
        const int my = lane < H ? sidx[lane] : -2;
        const float v = lane < H ? sa[lane] : 0.f;
        const int nslots = scat[64];
        for (int sl = wave; sl < nslots; sl += nw) {
            const int c = scat[sl];
            const bool in = my == c;
            const float m = wave_max(in ? v : -INFINITY);
            const float e = in ? expf(v - m) : 0.f;
            const float den = wave_sum(e);
            if (in) M[sl * hs + lane] = e / den;
        }
    }
    __syncthreads();

    const int nslots = scat[64];
    const int ct_eff = __builtin_amdgcn_readfirstlane((nslots + 15) >> 4);       // tiles that hold a present category
    const int nl = __builtin_amdgcn_readfirstlane(scat[65]);                     // 1 + the last history row that reaches the result
    // ---- 2. T_c of the present categories, one category tile at a time; 3. in the LAST tile every step's registers are
    // reloaded with the rows F x_t as soon as its four MFMAs are issued, so that the second fetch runs under the first chain
    // (a row without a present category has no tile: its registers are never read again)
    for (int it = 0; it < ct_eff; ++it) {
        const bool last = it == ct_eff - 1;      // wave-uniform
        v4f acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CTX0_STEPS; ++s) {
            if (s * 4 < nl) {                    // wave-uniform; the steps behind hold rows of weight 0 only: fma(0, x, acc) = acc
                const int j = s * 4 + lq;
                const float4 xc = xq[s];
                const float av = j < H ? M[(it * 16 + lr) * hs + j] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, acc[3], 0, 0, 0);
                if (last) xq[s] = (j < H && ch_ok) ? *reinterpret_cast<const float4*>(Fb + (long)j * d + ch) : f4_zero();
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sl = it * 16 + 4 * lq + r;
            if (sl < nslots && ch_ok)
                *reinterpret_cast<float4*>(Tl + (long)sl * d + ch) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        }
    }
    const float4 b4 = ch_ok ? *reinterpret_cast<const float4*>(g.bias + ch) : f4_zero();
    const float4 ku4 = ch_ok ? *reinterpret_cast<const float4*>(g.kq_user + (long)b * d + ch) : f4_zero();
    for (int it = 0; it < ct_eff; ++it) {
        v4f acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CTX0_STEPS; ++s) {
            if (s * 4 < nl) {
                const int j = s * 4 + lq;
                const float4 xc = xq[s];
                const float av = j < H ? M[(it * 16 + lr) * hs + j] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, acc[3], 0, 0, 0);
            }
        }
        // ---- 4. T2_c = relu(G_c + b) + T_c in place, and 5. the wave's share of the bucket's score
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sl = it * 16 + 4 * lq + r;
            float p = 0.f;
            if (sl < nslots && ch_ok) {
                float4* tp = reinterpret_cast<float4*>(Tl + (long)sl * d + ch);
                const float4 t = *tp;
                const float4 v = make_float4(fmaxf(acc[0][r] + b4.x, 0.f) + t.x, fmaxf(acc[1][r] + b4.y, 0.f) + t.y,
                                             fmaxf(acc[2][r] + b4.z, 0.f) + t.z, fmaxf(acc[3][r] + b4.w, 0.f) + t.w);
                *tp = v;
                p = fmaf(v.w, ku4.w, fmaf(v.z, ku4.z, fmaf(v.y, ku4.y, v.x * ku4.x)));
            }
            p += dpp_mov<0xB1>(p); p += dpp_mov<0x4E>(p); p += dpp_mov<0x141>(p); p += dpp_mov<0x140>(p);
            if (lr == 0 && sl < nslots) part[wave * 64 + sl] = p;
        }
    }
    // a category no history slot has: relu(b) (zero in the channels past d: b4 is)
    const float4 e4 = make_float4(fmaxf(b4.x, 0.f), fmaxf(b4.y, 0.f), fmaxf(b4.z, 0.f), fmaxf(b4.w, 0.f));
    {
        float p = fmaf(e4.w, ku4.w, fmaf(e4.z, ku4.z, fmaf(e4.y, ku4.y, e4.x * ku4.x)));
        p += dpp_mov<0xB1>(p); p += dpp_mov<0x4E>(p); p += dpp_mov<0x141>(p); p += dpp_mov<0x140>(p);
        if (lane == 0) pe[wave] = p;
    }
    __syncthreads();
    // ---- 5. every wave runs the softmax over the buckets for itself (C1 <= 64: lane c is bucket c): same bits in every wave
    float v = -INFINITY;
    if (lane < C1) {
        const int sl = cslot[lane];
        float a = 0.f;
        for (int w = 0; w < nw; ++w) a += sl >= 0 ? part[w * 64 + sl] : pe[w];
        v = g.mask[(long)b * C1 + lane] == 0 ? -1e9f : a / g.sqrt_d;
    }
    const float m = wave_max(v);
    const float e = lane < C1 ? expf(v - m) : 0.f;
    const float den = wave_sum(e);
    const float al = e / den;
    // ---- 6. the weighted sum in ascending category order (the four lq groups of a wave compute the same sum; lq = 0 stores it)
    float4 o = f4_zero();
    for (int c = 0; c < C1; ++c) {
        const float a = lane_bcast(al, c);
        if (a == 0.f) continue;                    // wave-uniform: a masked bucket adds nothing
        const int sl = cslot[c];
        const float4 t2 = sl < 0 ? e4 : (ch_ok ? *reinterpret_cast<const float4*>(Tl + (long)sl * d + ch) : f4_zero());
        o.x = fmaf(a, t2.x, o.x); o.y = fmaf(a, t2.y, o.y); o.z = fmaf(a, t2.z, o.z); o.w = fmaf(a, t2.w, o.w);
    }
    if (lq == 0 && ch_ok) {
        if (g.addend) o = f4_add(*reinterpret_cast<const float4*>(g.addend + (long)b * d + ch), o);
        *reinterpret_cast<float4*>(g.out + (long)b * d + ch) = o;
    }
}

// F x = ue W^T (no bias, no epilogue) and the kernel, on one stream.  `rows`: the graphs ue holds (the groups, or B); `fx`:
// rows * H * d floats of scratch.  The GEMM's kernel is pinned (m_dispatch, and the workgroup count behind the 64- / 128-row tile
// choice is taken at m_dispatch too when ragged tiles are asked for — so they always are): a row of F x has the same bits
// whether it is computed among 500 rows or 200 000, which keeps the grouped and the per-row entries bit-identical; the
// K-splitting [B,d] kernels are never chosen.
static int launch_user_ctx0(const float* ue, long rows, const int* group, const float* kq_topic, const float* kq_user,
                            const int64_t* idx, const uint8_t* mask, const float* Fa, const float* bFa, const void* wsplit, int format,
                            unsigned* range_flag, int ragged, const float* addend, float* out, float* fx, int B, int H, int C1, int d,
                            hipStream_t st) {
    if (!ctx0_fits(H, C1, d) || rows <= 0 || rows * H > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    GemmArgs gf = gemm_plain(ue, d, Fa, nullptr, fx, d, (int)(rows * H), d, d, 0);
    gf.wsplit = (const unsigned short*)wsplit; gf.format = format; gf.range_flag = range_flag;
    gf.m_dispatch = 1 << 30;
    gf.ragged = ragged ? ragged : DIGAT_GEMM_RAGGED;
    int rc = launch_gemm(gf, st);
    if (rc) return rc;
    const Ctx0Args g{ue, fx, (long)H * d, group, kq_topic, kq_user, idx, mask, bFa, addend, out, B, H, C1, d, sqrtf((float)d)};
    ProfScope prof(DIGAT_KERNEL_TOPIC, (double)rows * H * d * 8.0 + (double)B * (3.0 * d * 4 + H * 8.0 + C1), st);
    const int groups = (d + 63) / 64;
    const size_t lds = ctx0_lds_bytes(H, C1, d);
    if (H <= 52) hipLaunchKernelGGL(user_ctx0_kernel<13>, dim3(B), dim3(64 * groups), lds, st, g);
    else hipLaunchKernelGGL(user_ctx0_kernel<16>, dim3(B), dim3(64 * groups), lds, st, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
