// digat_context.inc — context kernels: ScaledDotProductAttention pooling and the torch_scatter topic pooling
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

// =================================================================================================
// 3. ScaledDotProductAttention pooling (a6) with the key projection folded into the query:
//    (K x_j).q = x_j.(K^T q)  ->  one [B,d] vector kq, then a_j = x_j.kq / sqrt(d)
// =================================================================================================
struct PoolArgs {
    const float* feat; long ld_b;        // feat[b] = feat + b*ld_b, nodes are d floats apart
    const float* kq; const uint8_t* mask; const float* addend; float* out;
    int B, n, d; float sqrt_d;
    float* alpha_out;                    // optional [B,n]: the attention weights (training)
    long ld_out;                         // attn_pool_kernel only: row stride of out (0: d)
    float* node0; long ld_node0;         // attn_pool_kernel only, optional: node 0 of every row is copied to node0 + b ld_node0
};

__global__ void __launch_bounds__(256) attn_pool_kernel(const PoolArgs g) {
    __shared__ float sc[DIGAT_MAX_NODES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d4 = g.d >> 2, n = g.n;
    const float4* F4 = reinterpret_cast<const float4*>(g.feat + (long)b * g.ld_b);
    const float4* K4 = reinterpret_cast<const float4*>(g.kq + (long)b * g.d);
    for (int j = wave; j < n; j += 4) {
        float part = 0.f;
        for (int c4 = lane; c4 < d4; c4 += 64) {
            const float4 x = F4[(long)j * d4 + c4], k = K4[c4];
            part = fmaf(x.w, k.w, fmaf(x.z, k.z, fmaf(x.y, k.y, fmaf(x.x, k.x, part))));
        }
        part = wave_sum(part);
        if (lane == 0) sc[j] = g.mask[(long)b * n + j] == 0 ? -1e9f : part / g.sqrt_d;
    }
    __syncthreads();
    if (wave == 0) {
        const float v0 = lane < n ? sc[lane] : -INFINITY;
        const float v1 = lane + 64 < n ? sc[lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(v0, v1));
        const float e0 = lane < n ? expf(v0 - m) : 0.f;
        const float e1 = lane + 64 < n ? expf(v1 - m) : 0.f;
        const float s = wave_sum(e0 + e1);
        if (lane < n) sc[lane] = e0 / s;
        if (lane + 64 < n) sc[lane + 64] = e1 / s;
        if (g.alpha_out) {
            if (lane < n) g.alpha_out[(long)b * n + lane] = e0 / s;
            if (lane + 64 < n) g.alpha_out[(long)b * n + lane + 64] = e1 / s;
        }
    }
    __syncthreads();
    for (int c4 = tid; c4 < d4; c4 += 256) {
        float4 o = f4_zero();
        for (int j = 0; j < n; ++j) {
            const float al = sc[j];
            // a weight of exactly zero (a masked node) adds nothing and its row is not read: dead nodes of a larger news graph are
            // never written (news_live_flags_kernel), and 0 x NaN would be NaN — the same rule as attn_pool_resident_kernel's
            if (al == 0.f) continue;               // the same for every thread of the workgroup
            const float4 x = F4[(long)j * d4 + c4];
            o.x = fmaf(al, x.x, o.x); o.y = fmaf(al, x.y, o.y); o.z = fmaf(al, x.z, o.z); o.w = fmaf(al, x.w, o.w);
        }
        if (g.addend) o = f4_add(reinterpret_cast<const float4*>(g.addend + (long)b * g.d)[c4], o);
        reinterpret_cast<float4*>(g.out + (long)b * (g.ld_out ? g.ld_out : (long)g.d))[c4] = o;
        if (g.node0) reinterpret_cast<float4*>(g.node0 + (long)b * g.ld_node0)[c4] = F4[c4];
    }
}

// The same pooling with every node read ONCE: wave w keeps its nodes (w, w + 4, ...: at most NPW of them) in registers, scores them,
// and after the softmax adds its own weighted rows; the four partial sums meet in LDS.  (The kernel above reads the rows a second
// time for the weighted sum, with 100 of 256 threads active at d = 400.)  Scores and weights are bit-identical to it; the
// weighted sum adds the nodes in the order (w = 0: j = 0, 4, 8, ...), (w = 1: ...), ... instead of j = 0, 1, 2, ...
template <int NPW, int U>      // n <= 4 NPW; float4 pieces per lane: d <= 256 U
__global__ void __launch_bounds__(256) attn_pool_resident_kernel(const PoolArgs g) {
    __shared__ float sc[DIGAT_MAX_NODES];
    __shared__ float4 part[4][64 * U];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d4 = g.d >> 2, n = g.n;
    const float4* F4 = reinterpret_cast<const float4*>(g.feat + (long)b * g.ld_b);
    const float4* K4 = reinterpret_cast<const float4*>(g.kq + (long)b * g.d);
    float4 x[NPW][U], k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        const float4 kv = K4[c4];
        k[u] = lane + 64 * u < d4 ? kv : f4_zero();           // padding lanes re-read the last piece and weigh it with zero
    }
    // Round 6: a MASKED node weighs exactly 0 (exp(-1e9 - max)) unless every node is masked (uniform weights then) and its row is
    // never touched below — so it is not fetched either: the user attention masks 8 of a MIND user's 18 buckets (118 -> ~66 MB per
    // 4 096-row launch), and the rows of masked buckets were never written by featureAffine anyway.  One byte per lane, two ballots.
    const unsigned long long mb0 = __ballot(lane < n && g.mask[(long)b * n + min(lane, n - 1)] != 0);
    const unsigned long long mb1 = __ballot(lane + 64 < n && g.mask[(long)b * n + min(lane + 64, n - 1)] != 0);
    const bool none = (mb0 | mb1) == 0ull;
#pragma unroll
    for (int t = 0; t < NPW; ++t) {
        const int j = min(wave + 4 * t, n - 1);                // slots past n: a repeated row, weight 0 below
        const bool want = none || (((j < 64 ? mb0 : mb1) >> (j & 63)) & 1ull);      // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u) x[t][u] = want ? F4[(long)j * d4 + min(lane + 64 * u, d4 - 1)] : f4_zero();
    }
#pragma unroll
    for (int t = 0; t < NPW; ++t) {
        const int j = wave + 4 * t;
        float p = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) p = fmaf(x[t][u].w, k[u].w, fmaf(x[t][u].z, k[u].z, fmaf(x[t][u].y, k[u].y, fmaf(x[t][u].x, k[u].x, p))));
        p = wave_sum(p);
        if (lane == 0 && j < n) sc[j] = g.mask[(long)b * n + j] == 0 ? -1e9f : p / g.sqrt_d;
    }
    __syncthreads();
    {   // every wave runs the softmax for itself (n <= 128: two values per lane): no second barrier, same bits in every wave
        const float v0 = lane < n ? sc[lane] : -INFINITY;
        const float v1 = lane + 64 < n ? sc[lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(v0, v1));
        const float e0 = lane < n ? expf(v0 - m) : 0.f;
        const float e1 = lane + 64 < n ? expf(v1 - m) : 0.f;
        const float s = wave_sum(e0 + e1);
        const float a0 = e0 / s, a1 = e1 / s;
        if (wave == 0 && g.alpha_out) {
            if (lane < n) g.alpha_out[(long)b * n + lane] = a0;
            if (lane + 64 < n) g.alpha_out[(long)b * n + lane + 64] = a1;
        }
        float4 o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) o[u] = f4_zero();
#pragma unroll
        for (int t = 0; t < NPW; ++t) {
            const int j = wave + 4 * t;
            const float al = j < n ? (j < 64 ? lane_bcast(a0, j & 63) : lane_bcast(a1, j & 63)) : 0.f;
            // a weight of exactly zero — a masked node: exp(-1e9 - max) = 0 — adds nothing, and its row may never have been written (the
            // dead nodes of a larger news graph, news_live_flags_kernel): it is not touched at all (wave-uniform; 0 x NaN would be NaN)
            if (al != 0.f) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    o[u].x = fmaf(al, x[t][u].x, o[u].x); o[u].y = fmaf(al, x[t][u].y, o[u].y);
                    o[u].z = fmaf(al, x[t][u].z, o[u].z); o[u].w = fmaf(al, x[t][u].w, o[u].w);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) part[wave][lane + 64 * u] = o[u];
    }
    __syncthreads();
    for (int c4 = tid; c4 < d4; c4 += 256) {
        float4 o = f4_add(f4_add(part[0][c4], part[1][c4]), f4_add(part[2][c4], part[3][c4]));
        if (g.addend) o = f4_add(reinterpret_cast<const float4*>(g.addend + (long)b * g.d)[c4], o);
        reinterpret_cast<float4*>(g.out + (long)b * g.d)[c4] = o;
    }
}

static int launch_pool(const float* feat, long ld_b, const float* kq, const uint8_t* mask, const float* addend,
                       float* out, int B, int n, int d, hipStream_t st) {
    if (n > DIGAT_MAX_NODES || d % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    PoolArgs g{feat, ld_b, kq, mask, addend, out, B, n, d, sqrtf((float)d), nullptr};
    ProfScope prof(DIGAT_KERNEL_POOL, (double)B * ((double)n * d * 4 + 2.0 * d * 4 + n), st);
    const int d4 = d / 4;
    if (d4 <= 128 && n <= 68) {              // every node read once (registers); inference and training alike
        if (d4 <= 64) {
            if (n <= 12) hipLaunchKernelGGL((attn_pool_resident_kernel<3, 1>), dim3(B), dim3(256), 0, st, g);
            else if (n <= 20) hipLaunchKernelGGL((attn_pool_resident_kernel<5, 1>), dim3(B), dim3(256), 0, st, g);
            else if (n <= 28) hipLaunchKernelGGL((attn_pool_resident_kernel<7, 1>), dim3(B), dim3(256), 0, st, g);
            else hipLaunchKernelGGL((attn_pool_resident_kernel<17, 1>), dim3(B), dim3(256), 0, st, g);
        } else {
            // (n <= 28: the 26-node news graphs of the MIND-large configuration — in the 17-slot form a wave requested ten rows it did
            // not have, repeats of its last one, and held 136 registers of rows: 60 us per 4 096 graphs)
            if (n <= 12) hipLaunchKernelGGL((attn_pool_resident_kernel<3, 2>), dim3(B), dim3(256), 0, st, g);
            else if (n <= 20) hipLaunchKernelGGL((attn_pool_resident_kernel<5, 2>), dim3(B), dim3(256), 0, st, g);
            else if (n <= 28) hipLaunchKernelGGL((attn_pool_resident_kernel<7, 2>), dim3(B), dim3(256), 0, st, g);
            else hipLaunchKernelGGL((attn_pool_resident_kernel<17, 2>), dim3(B), dim3(256), 0, st, g);
        }
        DIGAT_CHECK_LAUNCH();
        return DIGAT_OK;
    }
    hipLaunchKernelGGL(attn_pool_kernel, dim3(B), dim3(256), 0, st, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// =================================================================================================
// 4. topic pooling: scatter_softmax over history positions grouped by category + scatter_sum
// =================================================================================================
struct TopicArgs {
    const float* Xu; long ld_b; const float* kq; const int64_t* idx; float* out;
    int B, H, C1, d; float sqrt_d;
    float* alpha_out;                    // optional [B,H]: the segment-softmax weights (training)
    const int* group;                    // optional [B]: row b's nodes live at Xu + group[b] * ld_b (rows of one impression share them)
    const uint8_t* live; int live_ld;    // optional [B, live_ld] bytes: history rows t with live[b * live_ld + t] == 0 hold nothing
                                         // (dead nodes are never written by the encoder's layers): they are taken as 0 — by a
                                         // select, never a multiply, so that whatever bits the row holds cannot reach the result
    const int* hlast;                    // optional [B], with live: history rows t >= hlast[b] are all dead and are not even read
                                         // (right-padded histories: on MIND-shaped users ~60 % of the rows)
};
constexpr int TOPIC_MAX_H = 256;
constexpr int TOPIC_MAX_CT = 4;          // 16-row category tiles: category_num + 1 <= 64

// One workgroup per row, one wave per 64 channels (7 waves at d = 400).
//  1. scores a_t = x_t . kq / sqrt(d): a wave takes four history rows at a time (all their loads in flight),
//     lanes span the channels, one wave reduction per row;
//  2. segment softmax over the rows of equal category (H threads, O(H^2) LDS reads) -> the [C1, H] matrix
//     M[c][t] = alpha_t if idx_t == c else 0 in LDS;
//  3. out = M @ X on the fp32 matrix cores: v_mfma_f32_16x16x4_f32 is an exact k-ordered fma chain and
//     fma(0, x, acc) = acc, so out[c] is the sum over the rows of category c in ascending t — the CPU
//     scatter_add order — while X streams through once, coalesced, prefetched (the scalar version of this
//     phase walked H dependent, branchy loads per output).  Lane layout as in xattn_agg_kernel: MFMA column
//     l&15 of channel tile s is channel c0 + 4*(l&15) + s, so X loads and output stores are float4.
__global__ void __launch_bounds__(1024) topic_pool_kernel(const TopicArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = g.H, hs = H | 1;
    const int ct = (g.C1 + 15) >> 4;
    float* M = reinterpret_cast<float*>(smem);               // [ct*16][hs]
    float* sa = M + ct * 16 * hs;                            // [H]
    int* sidx = reinterpret_cast<int*>(sa + H);              // [H]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = blockDim.x, nw = nthreads >> 6;
    const int d4 = g.d >> 2;
    const float* Xb = g.Xu + (long)(g.group ? g.group[b] : b) * g.ld_b;
    const float4* F4 = reinterpret_cast<const float4*>(Xb);
    const float4* K4 = reinterpret_cast<const float4*>(g.kq + (long)b * g.d);
    unsigned char* slive = reinterpret_cast<unsigned char*>(sidx + H);   // [H]
    for (int t = tid; t < H; t += nthreads) {
        const long v = g.idx[(long)b * H + t];
        sidx[t] = (v >= 0 && v < g.C1) ? (int)v : -1;
        slive[t] = g.live ? g.live[(long)b * g.live_ld + t] : 1;
    }
    for (int i = tid; i < ct * 16 * hs; i += nthreads) M[i] = 0.f;
    __syncthreads();
    for (int t0 = wave; t0 < H; t0 += 4 * nw) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c4 = lane; c4 < d4; c4 += 64) {
            const float4 k = K4[c4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + r * nw;
                if (t < H && slive[t]) {
                    const float4 x = F4[(long)t * d4 + c4];
                    part[r] = fmaf(x.w, k.w, fmaf(x.z, k.z, fmaf(x.y, k.y, fmaf(x.x, k.x, part[r]))));
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + r * nw;
            const float s = wave_sum(part[r]);
            if (lane == 0 && t < H) sa[t] = s / g.sqrt_d;
        }
    }
    __syncthreads();
    for (int t = tid; t < H; t += nthreads) {
        const int s = sidx[t];
        float m = -INFINITY;
        for (int u = 0; u < H; ++u) if (sidx[u] == s) m = fmaxf(m, sa[u]);
        float den = 0.f;
        for (int u = 0; u < H; ++u) if (sidx[u] == s) den += expf(sa[u] - m);
        const float al = s >= 0 ? expf(sa[t] - m) / den : 0.f;
        if (s >= 0) M[s * hs + t] = al;
        if (g.alpha_out) g.alpha_out[(long)b * H + t] = al;
    }
    __syncthreads();

    const int lr = lane & 15, lq = lane >> 4;
    const int ch = wave * 64 + 4 * lr;
    const bool ch_ok = ch < g.d;             // no early exit: the MFMAs need every lane's operand rows
    const int nsteps = (H + 3) >> 2;
    auto load_x = [&](int step) -> float4 {
        const int j = step * 4 + lq;
        return (j < H && ch_ok && slive[j]) ? *reinterpret_cast<const float4*>(Xb + (long)j * g.d + ch) : f4_zero();
    };
    constexpr int PF = 4;
    v4f acc[TOPIC_MAX_CT][4];
#pragma unroll
    for (int it = 0; it < TOPIC_MAX_CT; ++it)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[it][s] = (v4f){0.f, 0.f, 0.f, 0.f};
    float4 xq[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) xq[u] = load_x(u);
    for (int step = 0; step < nsteps; step += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int st = step + u;
            if (st < nsteps) {
                const float4 xc = xq[u];
                xq[u] = load_x(st + PF);
                const int j = st * 4 + lq;
#pragma unroll
                for (int it = 0; it < TOPIC_MAX_CT; ++it) {
                    if (it < ct) {
                        const float av = j < H ? M[(it * 16 + lr) * hs + j] : 0.f;
                        acc[it][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, acc[it][0], 0, 0, 0);
                        acc[it][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, acc[it][1], 0, 0, 0);
                        acc[it][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, acc[it][2], 0, 0, 0);
                        acc[it][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, acc[it][3], 0, 0, 0);
                    }
                }
            }
        }
    }
    float* Ob = g.out + (long)b * g.C1 * g.d;
#pragma unroll
    for (int it = 0; it < TOPIC_MAX_CT; ++it) {
        if (it < ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = it * 16 + 4 * lq + r;
                if (c < g.C1 && ch_ok)
                    *reinterpret_cast<float4*>(Ob + (long)c * g.d + ch) =
                        make_float4(acc[it][0][r], acc[it][1][r], acc[it][2][r], acc[it][3][r]);
            }
        }
    }
}

// H <= 64 (the reference's max_history_num is 50): the history rows are read ONCE.  A wave owns 64 channels and
// keeps its slice of every history row in registers, in the MFMA operand layout of phase 3 (lane (lr, lq) holds
// channels c0+4lr..+3 of rows 4*step+lq): all 16 loads of a lane are in flight together, the scores are
// partial dot products over the wave's channels (reduced over the 16 lr lanes, then over the waves through LDS),
// the segment softmax is one masked wave reduction per category, and the MFMAs take X straight from the
// registers.  Same results as the kernel above up to the summation order of the scores.

// STEPS: 4-row steps held in registers (H <= 4 * STEPS).  With 16 steps hipcc spilled two registers at the 128 it may use
// (16 waves per CU keep two workgroups of 7 waves resident: a 512-thread bound without spills ran at 3 waves per SIMD and
// 20 % slower); the reference's H = 50 needs 13 steps and fits.
// The 16-step instantiation (H = 53 .. 64) is bounded to 512 threads (d <= 512): at 1024 it has 128 registers and spills two
// dozen of them; wider rows with such histories take topic_pool_kernel.
template <int TOPIC_RES_STEPS>
__global__ void __launch_bounds__(TOPIC_RES_STEPS > 13 ? 512 : 1024) topic_pool_resident_kernel(const TopicArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = g.H, hs = H | 1;
    const int ct = (g.C1 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = blockDim.x, nw = nthreads >> 6;
    float* M = reinterpret_cast<float*>(smem);               // [ct*16][hs]
    float* part = M + ct * 16 * hs;                          // [nw][64] partial scores
    float* sa = part + nw * 64;                              // [64]
    int* sidx = reinterpret_cast<int*>(sa + 64);             // [64]
    int* slive = sidx + 64;                                  // [64] live flags of the history rows (1 without a list)
    // Round 5: the categories that OCCUR among the row's history slots are numbered densely (slot = rank of the category among the
    // present ones) and only ceil(slots / 16) category tiles go through the matrix cores: a MIND user's 50 slots fall into 13 of the
    // 18 categories on average, one tile instead of two — half of this kernel's fp32 MFMAs (44 of its 97 us of SIMD time per 4096-row
    // launch, issued beside the projection GEMMs').  Per category the products and their order are unchanged: same bits.
    int* cslot = slive + 64;                                 // [64] category -> slot (-1: no history slot has it)
    int* scat = cslot + 64;                                  // [64] slot -> category; scat[63 - k] is not used: [64] = number of slots
    const int b = blockIdx.x;
    const float* Xb = g.Xu + (long)(g.group ? g.group[b] : b) * g.ld_b;
    const int lr = lane & 15, lq = lane >> 4;
    const int ch = wave * 64 + 4 * lr;
    const bool ch_ok = ch < g.d;             // no early exit: the MFMAs need every lane's operand rows
    const int nsteps = (H + 3) >> 2;
    // rows past the last live history slot are not requested at all: one scalar load ahead of the row requests (the count is
    // wave-uniform, so the predicate costs nothing per lane; a per-row flag load in front of every request measured slower)
    const int nl = (g.live && g.hlast) ? min(g.hlast[b], H) : H;

    float4 xq[TOPIC_RES_STEPS];
#pragma unroll
    for (int s = 0; s < TOPIC_RES_STEPS; ++s) {
        const int j = s * 4 + lq;
        // rows past the last live one: the request is redirected to that last row (a cache hit; dropped by the flag select below)
        // rather than predicated off — a per-lane "j < nl" in front of the 13 loads cost six spilled registers
        const int jr = min(j, nl > 0 ? nl - 1 : 0);
        xq[s] = (s < nsteps && j < H && ch_ok) ? *reinterpret_cast<const float4*>(Xb + (long)jr * g.d + ch) : f4_zero();
    }
    const float4 k4 = ch_ok ? *reinterpret_cast<const float4*>(g.kq + (long)b * g.d + ch) : f4_zero();
    if (tid < 64) {
        long v = -1;
        if (tid < H) v = g.idx[(long)b * H + tid];
        const int cat = (v >= 0 && v < g.C1) ? (int)v : -1;
        sidx[tid] = cat;
        slive[tid] = (g.live && tid < H) ? (int)g.live[(long)b * g.live_ld + tid] : 1;
        unsigned long long present = 0ull;                   // wave 0: which categories occur (C1 <= 64 ballots, scalar)
        for (int c = 0; c < g.C1; ++c) present |= __ballot(cat == c) ? (1ull << c) : 0ull;
        const bool has = tid < g.C1 && ((present >> tid) & 1ull);
        const int slot = __popcll(present & ((1ull << tid) - 1ull));
        cslot[tid] = has ? slot : -1;
        if (has) scat[slot] = tid;
        if (tid == 0) scat[64] = __popcll(present);
    }
    for (int i = tid; i < ct * 16 * hs; i += nthreads) M[i] = 0.f;
    if (g.live) {
        // The flags travel through LDS while the rows are in flight (no dependent round trip: the rows of dead nodes are
        // fetched and dropped — skipping their loads behind a flag load measured 38 -> 45 us).  A select, not a multiply.
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TOPIC_RES_STEPS; ++s) xq[s] = slive[min(s * 4 + lq, 63)] ? xq[s] : f4_zero();
    }

    // partial scores of this wave's 64 channels
#pragma unroll
    for (int s = 0; s < TOPIC_RES_STEPS; ++s) {
        float p = fmaf(xq[s].w, k4.w, fmaf(xq[s].z, k4.z, fmaf(xq[s].y, k4.y, xq[s].x * k4.x)));
        // sum over the 16 lanes of a row by DPP (VALU modifiers; __shfl_xor is a ds_bpermute round trip through the LDS crossbar:
        // 52 of them per lane sat on this kernel's critical path)
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
    // segment softmax: wave w takes the categories c = w, w + nw, ...; lane t is history row t
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
            if (in) {
                const float al = e / den;
                M[sl * hs + lane] = al;
                if (g.alpha_out) g.alpha_out[(long)b * H + lane] = al;
            }
        }
        if (wave == 0 && g.alpha_out && lane < H && my < 0) g.alpha_out[(long)b * H + lane] = 0.f;
    }
    __syncthreads();

    const int ct_eff = __builtin_amdgcn_readfirstlane((scat[64] + 15) >> 4);       // tiles that hold a present category
    const int nslots_all = scat[64];
    float* Ob = g.out + (long)b * g.C1 * g.d;
    // one category tile at a time (the rows stay in registers: nothing is re-read): 16 accumulator registers instead of 64 for the
    // four tiles a row may have, so that three workgroups of seven waves fit a CU instead of two
    for (int it = 0; it < ct_eff; ++it) {
        v4f acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < TOPIC_RES_STEPS; ++s) {
            if (s * 4 < nl) {                    // wave-uniform; the steps past the last live row hold zeros only: fma(alpha, 0, acc) = acc
                const int j = s * 4 + lq;
                const float4 xc = xq[s];
                const float av = j < H ? M[(it * 16 + lr) * hs + j] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xc.w, acc[3], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sl = it * 16 + 4 * lq + r;
            if (sl < nslots_all && ch_ok)
                *reinterpret_cast<float4*>(Ob + (long)scat[sl] * g.d + ch) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        }
    }
    // the categories no history slot has: zero rows (what the empty sums of the full tiles were)
    for (int c = lq; c < g.C1; c += 4)
        if (cslot[c] < 0 && ch_ok) *reinterpret_cast<float4*>(Ob + (long)c * g.d + ch) = f4_zero();
}

static int launch_topic_args(TopicArgs g, hipStream_t st) {
    const int groups = (g.d + 63) / 64;
    const int ct = (g.C1 + 15) / 16;
    if (g.H > TOPIC_MAX_H || g.d % 4 || groups > 16 || ct > TOPIC_MAX_CT) return DIGAT_ERR_SHAPE;
    const size_t lds = ((size_t)ct * 16 * (g.H | 1) + 2 * (size_t)g.H) * 4 + align_up((size_t)g.H, 16);
    if (lds > 64 * 1024) {
        static int raised = 0;
        if (!raised) {
            if (hipFuncSetAttribute((const void*)topic_pool_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
            raised = 1;
        }
    }
    if (g.H <= 64 && (g.H <= 52 || groups <= 8)) {
        const size_t ldsr = ((size_t)ct * 16 * (g.H | 1) + (size_t)groups * 64 + 192 + 64 + 68) * 4;
        if (g.H <= 52) hipLaunchKernelGGL(topic_pool_resident_kernel<13>, dim3(g.B), dim3(64 * groups), ldsr, st, g);
        else hipLaunchKernelGGL(topic_pool_resident_kernel<16>, dim3(g.B), dim3(64 * groups), ldsr, st, g);
    } else {
        hipLaunchKernelGGL(topic_pool_kernel, dim3(g.B), dim3(64 * groups), lds, st, g);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

static int launch_topic(const float* Xu, long ld_b, const float* kq, const int64_t* idx, float* out,
                        int B, int H, int C1, int d, hipStream_t st, const int* group = nullptr,
                        const uint8_t* live = nullptr, int live_ld = 0, const int* hlast = nullptr) {
    if (B == 0) return DIGAT_OK;
    TopicArgs g{Xu, ld_b, kq, idx, out, B, H, C1, d, sqrtf((float)d), nullptr, group, live, live_ld, hlast};
    ProfScope prof(DIGAT_KERNEL_TOPIC, (double)B * ((double)H * d * 4 + d * 4.0 + H * 8.0 + (double)C1 * d * 4), st);
    return launch_topic_args(g, st);
}

