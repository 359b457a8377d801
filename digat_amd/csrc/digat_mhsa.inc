// digat_mhsa.inc — key-masked multi-head self-attention encoder: the NRMS / NRMS-SA baselines of the reference's second experiment
// (Appendix-B/layers.py:79-95 MultiHeadAttention.forward with a mask, newsEncoders.py:46-58, userEncoders.py:44-47).
//   X = table[ids] (or dense rows);  Xd = dropout_{p_in}(X);  [Q|K|V] = Xd [W_Q|W_K|W_V]^T + [b_Q|0|b_V];  per sequence and head
//   S = Q K^T / sqrt(d_k), -1e9 over masked KEYS for every query row, alpha = softmax_j(S), c = dropout_{p_ctx}(alpha V)  (no ReLU);
//   out = additive tanh pooling of c (news_pool_fwd: masked with the same mask, or unmasked — the user encoder).
// Stages A and C are the MSA encoder's (digat_news.inc, digat_news_train.inc); the middle stage, forward and backward, is here.
// Two consequences of masked_fill(-1e9) are kept as they are: a sequence without a live key attends uniformly over all L positions
// (every score is -1e9), and no gradient reaches a masked score — in that sequence none at all, although alpha != 0 there.
// Included by digat_kernels.hip after digat_news_train.inc.

struct MhsaAttnArgs { const float* qkv; const uint8_t* mask; float* h; int T, L, heads, dk; unsigned thr, seed; float dscale; };
struct MhsaAttnBwdArgs { const float* qkv; const uint8_t* mask; const float* dh; float* dqkv; int T, L, heads, dk; unsigned thr, seed; float dscale; };
constexpr int MHSA_ST = 36;            // LDS row stride of the Q / K / V / dO images: both read patterns below are two-way at most
constexpr int MHSA_MFMA_DK = 32;       // the matrix-core kernels' head dim limit
constexpr int MHSA_MAX_DK = 128;       // the plain kernels'
constexpr int MHSA_MAX_L = 64;

// score of key j as the softmax sees it: tile padding (j >= L) is no key at all, a masked key reads -1e9 (masked_fill after the scale)
__device__ __forceinline__ float mhsa_score(float s, float scale, bool in_seq, bool live) {
    return in_seq ? (live ? s * scale : -1e9f) : -INFINITY;
}

// ---- forward on the fp32 matrix cores (L <= 16 NT, d_k <= 32): msa_attention_mfma_kernel's scheme, up to NT x NT score tiles ----------
//   S^T = K Q^T: tile (tj, ti), lane (lr, lq) ends with S[i = 16 ti + lr][j = 16 tj + 4 lq + r]; the softmax over j is in-lane plus two
//   xor-shuffles; alpha is the A operand of alpha V as it stands.  A wave holds one head at a time (Q, K, V images in LDS) and walks
//   its query tiles ti one after the other: NT score tiles and two output tiles live at a time.  Query and key tiles past L are skipped.
//   NT = 4: two waves a workgroup, NT = 2: four — 54 KB of LDS either way.
template <int NT>
__global__ void __launch_bounds__(NT == 4 ? 128 : 256) mhsa_attention_mfma_kernel(const MhsaAttnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = 16 * NT, IMG = R * MHSA_ST;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int L = g.L, dk = g.dk, hd = g.heads * g.dk;
    const int t = blockIdx.x;
    float* Qs = reinterpret_cast<float*>(smem) + (size_t)wave * 3 * IMG;
    float* Ks = Qs + IMG;
    float* Vs = Ks + IMG;
    const float* base = g.qkv + (long)t * L * 3 * hd;
    const float scale = 1.f / sqrtf((float)dk);
    const int ks_n = (dk + 3) >> 2, nct = dk > 16 ? 2 : 1, nt = (L + 15) >> 4;      // k steps, channel tiles, sequence tiles in use
    unsigned live = 0;                                   // bit 4 tj + r: key 16 tj + 4 lq + r is live
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = tj * 16 + 4 * lq + r;
            if (j < L && g.mask[(long)t * L + j]) live |= 1u << (4 * tj + r);
        }
    for (int head = blockIdx.y * nwaves + wave; head < g.heads; head += nwaves * gridDim.y) {
#pragma unroll 4
        for (int e = lane; e < nt * 16 * 32; e += 64) {
            const int j = e >> 5, c = e & 31;
            const bool ok = j < L && c < dk;
            const long off = (long)min(j, L - 1) * 3 * hd + head * dk + min(c, dk - 1);
            const float q = base[off], k = base[off + hd], v = base[off + 2 * hd];
            Qs[j * MHSA_ST + c] = ok ? q : 0.f; Ks[j * MHSA_ST + c] = ok ? k : 0.f; Vs[j * MHSA_ST + c] = ok ? v : 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int ti = 0; ti < nt; ++ti) {
            v4f s[NT];                             // [tj]
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) s[tj] = (v4f){0.f, 0.f, 0.f, 0.f};
            for (int ks = 0; ks < ks_n; ++ks) {
                const int k = ks * 4 + lq;
                const float qq = Qs[(16 * ti + lr) * MHSA_ST + k];
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
                    if (tj < nt) s[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(16 * tj + lr) * MHSA_ST + k], qq, s[tj], 0, 0, 0);
            }
            float m = -INFINITY;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = mhsa_score(s[tj][r], scale, tj * 16 + 4 * lq + r < L, (live >> (4 * tj + r)) & 1u);
                    s[tj][r] = x;
                    m = fmaxf(m, x);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float den = 0.f;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = expf(s[tj][r] - m);            // 0 on the tile padding, and on masked keys next to a live one
                    s[tj][r] = e;
                    den += e;
                }
            den += __shfl_xor(den, 16, 64);
            den += __shfl_xor(den, 32, 64);
            const float inv = 1.f / den;
            v4f o[2] = {(v4f){0.f, 0.f, 0.f, 0.f}, (v4f){0.f, 0.f, 0.f, 0.f}};      // [ct]
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
                if (tj < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = tj * 16 + 4 * lq + r;
                        const float al = s[tj][r] * inv;
                        o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(al, Vs[j * MHSA_ST + lr], o[0], 0, 0, 0);
                        if (nct > 1) o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(al, Vs[j * MHSA_ST + 16 + lr], o[1], 0, 0, 0);
                    }
                }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * 16 + 4 * lq + r, c = ct * 16 + lr;
                    if (i < L && c < dk) {
                        const long e = ((long)t * L + i) * hd + head * dk + c;
                        float v = o[ct][r];
                        if (g.thr) v = drop_keep(g.seed, e, g.thr) ? v * g.dscale : 0.f;      // site 2
                        g.h[e] = v;
                    }
                }
        }
        __builtin_amdgcn_wave_barrier();           // the next head overwrites Q / K / V
    }
}

// ---- backward on the fp32 matrix cores (same limits): one wave per head at a time, S and alpha recomputed -------------------------
// With dO = dropout-backward(dh) (keep bits regenerated), s = 1/sqrt(d_k):
//   dalpha = dO V^T;  delta_i = sum_j alpha_ij dalpha_ij;  dS = live_j ? s alpha (dalpha - delta) : 0;  dQ = dS K;  dK = dS^T Q;  dV = alpha^T dO.
// Pass 1, per query tile ti, holds the transposed tiles (lane: i = 16 ti + lr, j = 16 tj + 4 lq + r): softmax and delta in-lane plus two
// shuffles, dS the A operand of dQ = dS K as it stands; it leaves max, 1 / denominator and delta per query row in LDS (3 x 64 floats).
// Pass 2, again per query tile, forms S and dalpha once more in the other orientation (lane: j = 16 tj + lr, i = 16 ti + 4 lq + r) from
// the same images — 2 NT^2 d_k/4 more matrix instructions, nothing of size L^2 through LDS — and there alpha and dS are the A operands
// of dV and dK as they stand; dK and dV accumulate over the query tiles.
template <int NT>
__global__ void __launch_bounds__(NT == 4 ? 64 : 128) mhsa_attention_bwd_mfma_kernel(const MhsaAttnBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = 16 * NT, IMG = R * MHSA_ST, PER_WAVE = 4 * IMG + 3 * R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int L = g.L, dk = g.dk, hd = g.heads * g.dk;
    const int t = blockIdx.x;
    float* Qs = reinterpret_cast<float*>(smem) + (size_t)wave * PER_WAVE;
    float* Ks = Qs + IMG;
    float* Vs = Ks + IMG;
    float* Os = Vs + IMG;                // dO
    float* Ms = Os + IMG;                // per query row: max, 1 / denominator, delta
    float* Is = Ms + R;
    float* Dl = Is + R;
    const float* base = g.qkv + (long)t * L * 3 * hd;
    const float* dhb = g.dh + (long)t * L * hd;
    float* dbase = g.dqkv + (long)t * L * 3 * hd;
    const float scale = 1.f / sqrtf((float)dk);
    const int ks_n = (dk + 3) >> 2, nct = dk > 16 ? 2 : 1, nt = (L + 15) >> 4;
    unsigned live1 = 0, live2 = 0;       // pass 1: bit 4 tj + r = key 16 tj + 4 lq + r;  pass 2: bit tj = key 16 tj + lr
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = tj * 16 + 4 * lq + r;
            if (j < L && g.mask[(long)t * L + j]) live1 |= 1u << (4 * tj + r);
        }
        const int j2 = tj * 16 + lr;
        if (j2 < L && g.mask[(long)t * L + j2]) live2 |= 1u << tj;
    }
    for (int head = blockIdx.y * nwaves + wave; head < g.heads; head += nwaves * gridDim.y) {
#pragma unroll 4
        for (int e = lane; e < nt * 16 * 32; e += 64) {
            const int j = e >> 5, c = e & 31;
            const bool ok = j < L && c < dk;
            const int jc = min(j, L - 1), cc = min(c, dk - 1);
            const long off = (long)jc * 3 * hd + head * dk + cc, ho = (long)jc * hd + head * dk + cc;
            const float q = base[off], k = base[off + hd], v = base[off + 2 * hd];
            float d = dhb[ho];
            if (g.thr) d = drop_keep(g.seed, (long)t * L * hd + ho, g.thr) ? d * g.dscale : 0.f;      // site 2, backward
            Qs[j * MHSA_ST + c] = ok ? q : 0.f; Ks[j * MHSA_ST + c] = ok ? k : 0.f; Vs[j * MHSA_ST + c] = ok ? v : 0.f;
            Os[j * MHSA_ST + c] = ok ? d : 0.f;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        // ---- pass 1: dQ and the row statistics
#pragma unroll 1
        for (int ti = 0; ti < nt; ++ti) {
            v4f s[NT], da[NT];                     // [tj]: S^T -> alpha; dalpha -> dS
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) { s[tj] = (v4f){0.f, 0.f, 0.f, 0.f}; da[tj] = (v4f){0.f, 0.f, 0.f, 0.f}; }
            for (int ks = 0; ks < ks_n; ++ks) {
                const int k = ks * 4 + lq;
                const float qq = Qs[(16 * ti + lr) * MHSA_ST + k], oo = Os[(16 * ti + lr) * MHSA_ST + k];
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
                    if (tj < nt) {
                        s[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(16 * tj + lr) * MHSA_ST + k], qq, s[tj], 0, 0, 0);
                        da[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(Vs[(16 * tj + lr) * MHSA_ST + k], oo, da[tj], 0, 0, 0);
                    }
            }
            float m = -INFINITY;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = mhsa_score(s[tj][r], scale, tj * 16 + 4 * lq + r < L, (live1 >> (4 * tj + r)) & 1u);
                    s[tj][r] = x;
                    m = fmaxf(m, x);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float den = 0.f;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = expf(s[tj][r] - m);
                    s[tj][r] = e;
                    den += e;
                }
            den += __shfl_xor(den, 16, 64);
            den += __shfl_xor(den, 32, 64);
            const float inv = 1.f / den;
            float delta = 0.f;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[tj][r] *= inv;
                    delta = fmaf(s[tj][r], da[tj][r], delta);
                }
            delta += __shfl_xor(delta, 16, 64);
            delta += __shfl_xor(delta, 32, 64);
            if (lq == 0) { Ms[16 * ti + lr] = m; Is[16 * ti + lr] = inv; Dl[16 * ti + lr] = delta; }
            v4f o[2] = {(v4f){0.f, 0.f, 0.f, 0.f}, (v4f){0.f, 0.f, 0.f, 0.f}};      // dQ: [ct]
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
                if (tj < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = tj * 16 + 4 * lq + r;
                        const float ds = ((live1 >> (4 * tj + r)) & 1u) ? scale * s[tj][r] * (da[tj][r] - delta) : 0.f;
                        o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, Ks[j * MHSA_ST + lr], o[0], 0, 0, 0);
                        if (nct > 1) o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, Ks[j * MHSA_ST + 16 + lr], o[1], 0, 0, 0);
                    }
                }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = ti * 16 + 4 * lq + r, c = ct * 16 + lr;
                    if (row < L && c < dk) dbase[(long)row * 3 * hd + head * dk + c] = o[ct][r];
                }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);        // the row statistics are in LDS
        __builtin_amdgcn_wave_barrier();
        // ---- pass 2: dK and dV
        v4f pk[NT][2], pv[NT][2];                  // [tj][ct], rows j = 16 tj + 4 lq + r, channel 16 ct + lr
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) { pk[tj][ct] = (v4f){0.f, 0.f, 0.f, 0.f}; pv[tj][ct] = (v4f){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
        for (int ti = 0; ti < nt; ++ti) {
            v4f s[NT], da[NT];                     // [tj]: lane holds [i = 16 ti + 4 lq + r][j = 16 tj + lr]
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) { s[tj] = (v4f){0.f, 0.f, 0.f, 0.f}; da[tj] = (v4f){0.f, 0.f, 0.f, 0.f}; }
            for (int ks = 0; ks < ks_n; ++ks) {
                const int k = ks * 4 + lq;
                const float qq = Qs[(16 * ti + lr) * MHSA_ST + k], oo = Os[(16 * ti + lr) * MHSA_ST + k];
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
                    if (tj < nt) {
                        s[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq, Ks[(16 * tj + lr) * MHSA_ST + k], s[tj], 0, 0, 0);
                        da[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(oo, Vs[(16 * tj + lr) * MHSA_ST + k], da[tj], 0, 0, 0);
                    }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 16 + 4 * lq + r;
                const float m = Ms[i], inv = Is[i], delta = Dl[i];
                const float q0 = Qs[i * MHSA_ST + lr], g0 = Os[i * MHSA_ST + lr];
                const float q1 = Qs[i * MHSA_ST + 16 + lr], g1 = Os[i * MHSA_ST + 16 + lr];
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
                    if (tj < nt) {
                        const bool lv = (live2 >> tj) & 1u;
                        const float al = expf(mhsa_score(s[tj][r], scale, tj * 16 + lr < L, lv) - m) * inv;
                        const float ds = lv ? scale * al * (da[tj][r] - delta) : 0.f;
                        pk[tj][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, q0, pk[tj][0], 0, 0, 0);
                        pv[tj][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(al, g0, pv[tj][0], 0, 0, 0);
                        if (nct > 1) {
                            pk[tj][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds, q1, pk[tj][1], 0, 0, 0);
                            pv[tj][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(al, g1, pv[tj][1], 0, 0, 0);
                        }
                    }
            }
        }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tj * 16 + 4 * lq + r, c = ct * 16 + lr;
                    if (row < L && c < dk) {
                        dbase[(long)row * 3 * hd + hd + head * dk + c] = pk[tj][ct][r];
                        dbase[(long)row * 3 * hd + 2 * hd + head * dk + c] = pv[tj][ct][r];
                    }
                }
        __builtin_amdgcn_wave_barrier();           // the next head overwrites the images
    }
}

// ---- plain fp32 kernels of the same semantics (d_k > 32): one wave per (sequence, head), lane i owns query row i (then key row i);
// alpha and dS rows in LDS (row stride L + 1), Q / K / V rows from global memory (L2-resident: 64 rows of one head) ------------------
__global__ void __launch_bounds__(64) mhsa_attention_plain_kernel(const MhsaAttnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Ss = reinterpret_cast<float*>(smem);
    const int i = threadIdx.x, L = g.L, dk = g.dk, hd = g.heads * g.dk, t = blockIdx.x, head = blockIdx.y, st = L + 1;
    const float* base = g.qkv + (long)t * L * 3 * hd + head * dk;
    const float scale = 1.f / sqrtf((float)dk);
    if (i >= L) return;                            // no workgroup barrier below: every lane works on its own row of Ss
    const float* q = base + (long)i * 3 * hd;
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) {
        const float* k = base + (long)j * 3 * hd + hd;
        float s = 0.f;
        for (int c = 0; c < dk; ++c) s = fmaf(q[c], k[c], s);
        s = mhsa_score(s, scale, true, g.mask[(long)t * L + j] != 0);
        Ss[i * st + j] = s;
        m = fmaxf(m, s);
    }
    float den = 0.f;
    for (int j = 0; j < L; ++j) { const float e = expf(Ss[i * st + j] - m); Ss[i * st + j] = e; den += e; }
    const float inv = 1.f / den;
    for (int c = 0; c < dk; ++c) {
        float o = 0.f;
        for (int j = 0; j < L; ++j) o = fmaf(Ss[i * st + j] * inv, base[(long)j * 3 * hd + 2 * hd + c], o);
        const long e = ((long)t * L + i) * hd + head * dk + c;
        if (g.thr) o = drop_keep(g.seed, e, g.thr) ? o * g.dscale : 0.f;
        g.h[e] = o;
    }
}

__global__ void __launch_bounds__(64) mhsa_attention_bwd_plain_kernel(const MhsaAttnBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int i = threadIdx.x, L = g.L, dk = g.dk, hd = g.heads * g.dk, t = blockIdx.x, head = blockIdx.y, st = L + 1;
    float* As = reinterpret_cast<float*>(smem);    // alpha [i][j]
    float* Ds = As + L * st;                       // dS [i][j]
    const float* base = g.qkv + (long)t * L * 3 * hd + head * dk;
    const float* dhb = g.dh + (long)t * L * hd + head * dk;
    float* dbase = g.dqkv + (long)t * L * 3 * hd + head * dk;
    const float scale = 1.f / sqrtf((float)dk);
    auto dO = [&](int row, int c) {
        const long e = ((long)t * L + row) * hd + head * dk + c;
        const float d = dhb[(long)row * hd + c];
        return g.thr ? (drop_keep(g.seed, e, g.thr) ? d * g.dscale : 0.f) : d;
    };
    if (i < L) {
        const float* q = base + (long)i * 3 * hd;
        float m = -INFINITY;
        for (int j = 0; j < L; ++j) {
            const float* k = base + (long)j * 3 * hd + hd;
            float s = 0.f;
            for (int c = 0; c < dk; ++c) s = fmaf(q[c], k[c], s);
            s = mhsa_score(s, scale, true, g.mask[(long)t * L + j] != 0);
            As[i * st + j] = s;
            m = fmaxf(m, s);
        }
        float den = 0.f;
        for (int j = 0; j < L; ++j) { const float e = expf(As[i * st + j] - m); As[i * st + j] = e; den += e; }
        const float inv = 1.f / den;
        float delta = 0.f;
        for (int j = 0; j < L; ++j) {
            const float* v = base + (long)j * 3 * hd + 2 * hd;
            float da = 0.f;
            for (int c = 0; c < dk; ++c) da = fmaf(dO(i, c), v[c], da);
            const float al = As[i * st + j] * inv;
            As[i * st + j] = al;
            Ds[i * st + j] = da;
            delta = fmaf(al, da, delta);
        }
        for (int j = 0; j < L; ++j)
            Ds[i * st + j] = g.mask[(long)t * L + j] ? scale * As[i * st + j] * (Ds[i * st + j] - delta) : 0.f;
        for (int c = 0; c < dk; ++c) {
            float o = 0.f;
            for (int j = 0; j < L; ++j) o = fmaf(Ds[i * st + j], base[(long)j * 3 * hd + hd + c], o);
            dbase[(long)i * 3 * hd + c] = o;
        }
    }
    __syncthreads();                               // one wave: the rows of alpha and dS are read across lanes below
    if (i < L) {
        for (int c = 0; c < dk; ++c) {
            float a = 0.f, b = 0.f;
            for (int r = 0; r < L; ++r) {
                a = fmaf(Ds[r * st + i], base[(long)r * 3 * hd + c], a);
                b = fmaf(As[r * st + i], dO(r, c), b);
            }
            dbase[(long)i * 3 * hd + hd + c] = a;
            dbase[(long)i * 3 * hd + 2 * hd + c] = b;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static int launch_mhsa_attention(const float* qkv, const uint8_t* mask, float* h, float p_ctx, uint32_t seed, int T, int L, int heads, int dk,
                                 hipStream_t st) {
    MhsaAttnArgs a{qkv, mask, h, T, L, heads, dk, p_ctx > 0.f ? drop_threshold(p_ctx) : 0u, seed, 1.f / (1.f - p_ctx)};
    if (dk <= MHSA_MFMA_DK) {
        const size_t lds = (size_t)4 * 3 * 32 * MHSA_ST * 4;          // four waves x 32 rows = two waves x 64 rows
        // few sequences (a training step's 64 histories): the heads of one are spread over up to four workgroups, as in the backward
        if (L <= 32) hipLaunchKernelGGL(mhsa_attention_mfma_kernel<2>, dim3(T, T >= 1024 ? 1 : min(4, (heads + 3) / 4)), dim3(256), lds, st, a);
        else hipLaunchKernelGGL(mhsa_attention_mfma_kernel<4>, dim3(T, T >= 1024 ? 1 : min(4, (heads + 1) / 2)), dim3(128), lds, st, a);
    } else {
        hipLaunchKernelGGL(mhsa_attention_plain_kernel, dim3(T, heads), dim3(64), (size_t)L * (L + 1) * 4, st, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
static int launch_mhsa_attention_bwd(const float* qkv, const uint8_t* mask, const float* dh, float* dqkv, float p_ctx, uint32_t seed, int T, int L,
                                     int heads, int dk, hipStream_t st) {
    MhsaAttnBwdArgs a{qkv, mask, dh, dqkv, T, L, heads, dk, p_ctx > 0.f ? drop_threshold(p_ctx) : 0u, seed, 1.f / (1.f - p_ctx)};
    if (dk <= MHSA_MFMA_DK) {
        // few sequences: the heads of one are spread over up to four workgroups
        if (L <= 32) {
            const int gy = T >= 1024 ? 1 : min(4, (heads + 1) / 2);
            hipLaunchKernelGGL(mhsa_attention_bwd_mfma_kernel<2>, dim3(T, gy), dim3(128), (size_t)2 * (4 * 32 * MHSA_ST + 3 * 32) * 4, st, a);
        } else {
            const int gy = T >= 1024 ? 1 : min(4, heads);
            hipLaunchKernelGGL(mhsa_attention_bwd_mfma_kernel<4>, dim3(T, gy), dim3(64), (size_t)(4 * 64 * MHSA_ST + 3 * 64) * 4, st, a);
        }
    } else {
        hipLaunchKernelGGL(mhsa_attention_bwd_plain_kernel, dim3(T, heads), dim3(64), (size_t)2 * L * (L + 1) * 4, st, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// inference: the MSA encoder's regions and the all-ones pooling mask of the "pooling unmasked" flag
struct MhsaFwdWs { MsaFwdWs m; uint8_t* ones; };
static size_t mhsa_fwd_carve(Arena& w, int T, int L, int dm, int hd, int att, MhsaFwdWs* o) {
    msa_fwd_carve(w, T, L, dm, hd, att, &o->m);
    o->ones = w.take<uint8_t>((size_t)T * L);
    return w.used;
}
struct MhsaTrainWs { MsaTrainWs m; uint8_t* ones; };
static size_t mhsa_train_carve(Arena& w, int T, int L, int dm, int hd, int att, MhsaTrainWs* o) {
    msa_train_carve(w, T, L, dm, hd, att, &o->m);
    o->ones = w.take<uint8_t>((size_t)T * L);
    return w.used;
}
static int mhsa_shape_ok(const digat_mhsa_params* p, int L, bool training) {
    const int dm = p->in_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    return dm > 0 && dm % 4 == 0 && heads > 0 && dk > 0 && dk <= MHSA_MAX_DK && att > 0 && (!training || att % 4 == 0) && (heads * dk) % 4 == 0 &&
           L <= MHSA_MAX_L;
}
// the pooling mask: the key mask, or all ones
static int mhsa_pool_mask(const digat_mhsa_params* p, const uint8_t* mask, uint8_t* ones, long M, hipStream_t st, const uint8_t** out) {
    *out = mask;
    if (p->flags & DIGAT_MHSA_POOL_UNMASKED) {
        if (hipMemsetAsync(ones, 1, (size_t)M, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
        *out = ones;
    }
    return DIGAT_OK;
}

extern "C" {

int digat_mhsa_attention_fwd(const float* qkv, const uint8_t* mask, float* h, float p_ctx, uint32_t seed, int T, int L, int heads, int dk,
                             void* stream) {
    if (!qkv || !mask || !h || T < 0 || L <= 0 || heads <= 0 || dk <= 0 || p_ctx < 0.f || p_ctx >= 1.f) return DIGAT_ERR_ARG;
    if (L > MHSA_MAX_L || dk > MHSA_MAX_DK) return DIGAT_ERR_SHAPE;
    if (T == 0) return DIGAT_OK;
    return launch_mhsa_attention(qkv, mask, h, p_ctx, seed, T, L, heads, dk, (hipStream_t)stream);
}
int digat_mhsa_attention_bwd(const float* qkv, const uint8_t* mask, const float* dh, float* dqkv, float p_ctx, uint32_t seed, int T, int L,
                             int heads, int dk, void* stream) {
    if (!qkv || !mask || !dh || !dqkv || T < 0 || L <= 0 || heads <= 0 || dk <= 0 || p_ctx < 0.f || p_ctx >= 1.f) return DIGAT_ERR_ARG;
    if (L > MHSA_MAX_L || dk > MHSA_MAX_DK) return DIGAT_ERR_SHAPE;
    if (T == 0) return DIGAT_OK;
    return launch_mhsa_attention_bwd(qkv, mask, dh, dqkv, p_ctx, seed, T, L, heads, dk, (hipStream_t)stream);
}

size_t digat_mhsa_workspace_bytes(int T, int L, int in_dim, int heads, int dk, int att) {
    Arena measure;
    MhsaFwdWs o;
    return mhsa_fwd_carve(measure, T, L, in_dim, heads * dk, att, &o);
}

int digat_mhsa_fwd(const digat_mhsa_params* p, const int32_t* ids, const uint8_t* mask, float* out, int T, int L, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!p || !p->table || !mask || !out || !workspace || T < 0 || L <= 0) return DIGAT_ERR_ARG;
    if (!mhsa_shape_ok(p, L, false)) return DIGAT_ERR_SHAPE;
    const int dm = p->in_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim, hd = heads * dk;
    Arena w(workspace, workspace_bytes);
    MhsaFwdWs o;
    mhsa_fwd_carve(w, T, L, dm, hd, att, &o);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    if (T == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)T * L;
    // A. [Q|K|V]: the ids are the GEMM's row list where its kernel takes one; else the rows are gathered first and the launch is the
    //    dense input's.  Unlike digat_msa_fwd, which drops the split image on its gather fallback and runs fp32 there, both keep
    //    `wsplit`: below 2 048 rows the dispatch then takes the skinny kernel on the same bf16x6 image (fp32-grade as well), and the
    //    gathered and the dense call stay one launch, bit for bit.
    GemmArgs g = gemm_plain(p->table, dm, p->W_Q, p->b_Q, o.m.qkv, 3 * hd, (int)M, hd, dm, 0);
    g.w[1] = p->W_K; g.bias[1] = nullptr; g.y[1] = o.m.qkv + hd;
    g.w[2] = p->W_V; g.bias[2] = p->b_V; g.y[2] = o.m.qkv + 2 * hd;
    g.nsegs = 3;
    g.wsplit = (const unsigned short*)p->qkv_wsplit;
    if (ids) {
        g.rowidx = ids; g.gather_only = 1;
        if (!gemm_takes_row_list(g)) {
            T_TRY(launch_gather_embedding(p->table, ids, o.m.emb, M, dm, st));
            g.a0 = o.m.emb; g.rowidx = nullptr; g.gather_only = 0;
        }
    }
    T_TRY(launch_gemm(g, st, DIGAT_KERNEL_LINEAR));
    // B. key-masked attention, no ReLU
    T_TRY(launch_mhsa_attention(o.m.qkv, mask, o.m.h, 0.f, 0u, T, L, heads, dk, st));
    // C. pooling
    const uint8_t* pmask;
    T_TRY(mhsa_pool_mask(p, mask, o.ones, M, st, &pmask));
    return news_pool_fwd(o.m.h, hd, p->A1, p->a1_wsplit, p->b1, p->a2, o.m.pre, pmask, out, nullptr, T, L, att, false, st);
}

size_t digat_mhsa_train_save_bytes(int T, int L, int in_dim, int heads, int dk, int att) {
    Arena measure;
    MsaSave s;
    return msa_save_carve(measure, T, L, in_dim, heads * dk, att, &s);
}
size_t digat_mhsa_train_workspace_bytes(int T, int L, int in_dim, int heads, int dk, int att) {
    Arena measure;
    MhsaTrainWs o;
    return mhsa_train_carve(measure, T, L, in_dim, heads * dk, att, &o);
}

// p_in: dropout on the input rows (site 1: the counter hash of `seed` over the [T L, in_dim] elements); p_ctx: on the attention's output
// (site 2: `seed + 1` over [T L, hd], applied in the attention kernel's epilogue).  The *_wsplit fields of params are not used (the
// weights change every optimiser step: they are split here, into the workspace).
int digat_mhsa_fwd_train(const digat_mhsa_params* p, const int32_t* ids, const uint8_t* mask, float* out, float p_in, float p_ctx, uint32_t seed,
                         int T, int L, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !p->table || !mask || !out || !save || !workspace || T < 0 || L <= 0 || p_in < 0.f || p_in >= 1.f || p_ctx < 0.f || p_ctx >= 1.f)
        return DIGAT_ERR_ARG;
    if (!mhsa_shape_ok(p, L, true)) return DIGAT_ERR_SHAPE;
    const int dm = p->in_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim, hd = heads * dk;
    if (T == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    MsaSave s;
    MhsaTrainWs o;
    msa_save_carve(sa, T, L, dm, hd, att, &s);
    mhsa_train_carve(w, T, L, dm, hd, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)T * L;
    // Xd = dropout(table[ids]) in `save`; dense rows without dropout are read where they are
    const float* Xd = s.Ed;
    if (ids) {
        T_TRY(launch_gather_embedding(p->table, ids, s.Ed, M, dm, st));
        if (p_in > 0.f) T_TRY(digat_dropout_fwd(s.Ed, s.Ed, s.dmask, M * dm, p_in, seed, stream));
    } else if (p_in > 0.f) {
        T_TRY(digat_dropout_fwd(p->table, s.Ed, s.dmask, M * dm, p_in, seed, stream));
    } else {
        Xd = p->table;
    }
    GemmArgs g = gemm_plain(Xd, dm, p->W_Q, p->b_Q, s.qkv, 3 * hd, (int)M, hd, dm, 0);
    g.w[1] = p->W_K; g.bias[1] = nullptr; g.y[1] = s.qkv + hd;
    g.w[2] = p->W_V; g.bias[2] = p->b_V; g.y[2] = s.qkv + 2 * hd;
    g.nsegs = 3;
    if (hd % 80 == 0 && dm >= 32 && M >= 2048) {
        T_TRY(launch_split(p->W_Q, p->W_K, p->W_V, hd, 3, dm, o.m.qkv_img, st));
        g.wsplit = (const unsigned short*)o.m.qkv_img;
        if (g_train_bf16) g.x1_segs = 7;
    }
    T_TRY(launch_gemm(g, st, DIGAT_KERNEL_LINEAR));
    T_TRY(launch_mhsa_attention(s.qkv, mask, s.h, p_ctx, seed + 1u, T, L, heads, dk, st));
    const void* a1_img = nullptr;
    if (M >= 2048 && hd >= 32) {
        T_TRY(launch_split(p->A1, p->A1, p->A1, att, 1, hd, o.m.a1_img, st));
        a1_img = o.m.a1_img;
    }
    const uint8_t* pmask;
    T_TRY(mhsa_pool_mask(p, mask, o.ones, M, st, &pmask));
    return news_pool_fwd(s.h, hd, p->A1, a1_img, p->b1, p->a2, s.pre, pmask, out, s.alpha, T, L, att, true, st);
}

// dout [T, hd].  p_in, p_ctx and seed are the forward's.  Written (not accumulated): row_grad [T L, in_dim], rows ld_row_grad floats apart
// (in_dim, or digat_msa_row_grad_ld(T, L, in_dim)) — the gradient at the gathered rows before the dropout (feed it to
// digat_embedding_bwd), which for dense input is dX — and the weight gradients as digat_msa_bwd writes them.
int digat_mhsa_bwd(const digat_mhsa_params* p, const int32_t* ids, const uint8_t* mask, const float* dout, float p_in, float p_ctx, uint32_t seed,
                   const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW_Q, float* db_Q, float* dW_K, float* dW_V,
                   float* db_V, float* dA1, float* db1, float* da2, int T, int L, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !p->table || !mask || !dout || !save || !row_grad || !dW_Q || !db_Q || !dW_K || !dW_V || !db_V || !dA1 || !db1 || !da2 || !workspace ||
        T < 0 || L <= 0 || p_in < 0.f || p_in >= 1.f || p_ctx < 0.f || p_ctx >= 1.f) return DIGAT_ERR_ARG;
    if (!mhsa_shape_ok(p, L, true)) return DIGAT_ERR_SHAPE;
    const int dm = p->in_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    const int hd = heads * dk, dmp = (int)msa_attp(dm);
    if (ld_row_grad != dm && ld_row_grad != dmp) return DIGAT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t wn = (size_t)hd * dm, hn = hd, an = att;
    if (T == 0) return zero_floats(st, {{dW_Q, wn}, {dW_K, wn}, {dW_V, wn}, {db_Q, hn}, {db_V, hn}, {dA1, an * hn}, {db1, an}, {da2, an}});
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    MsaSave s;
    MhsaTrainWs o;
    msa_save_carve(sa, T, L, dm, hd, att, &s);
    mhsa_train_carve(w, T, L, dm, hd, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    const long M = (long)T * L;
    const float* Xd = (ids || p_in > 0.f) ? s.Ed : p->table;
    const uint8_t* pmask;
    T_TRY(mhsa_pool_mask(p, mask, o.ones, M, st, &pmask));
    T_TRY(news_pool_bwd(dout, s.h, hd, s.pre, s.alpha, pmask, p->A1, p->b1, p->a2, o.m.pool, o.m.wg, o.m.wgb, dA1, db1, da2, T, L, att, st));
    // site 2's backward + attention
    T_TRY(launch_mhsa_attention_bwd(s.qkv, mask, o.m.pool.dh, o.m.dqkv, p_ctx, seed + 1u, T, L, heads, dk, st));
    // projections: dXd = dQ W_Q + dK W_K + dV W_V with site 1's backward, dW_* = d*^T Xd, db_Q, db_V = column sums: digat_msa_bwd's
    T_TRY(qkv_input_grad(p->W_Q, p->W_K, p->W_V, o.m, s.dmask, p_in, row_grad, ld_row_grad, M, dm, hd, st));
    return qkv_weight_grad(o.m, Xd, dW_Q, db_Q, dW_K, dW_V, db_V, M, dm, hd, st);
}

}  // extern "C"
