// digat_news.inc — MSA news encoder, inference (SURVEY §8f-2; reference: newsEncoders.py:58-82, layers.py:50-115).
// Upstream of the graph encoder: it produces the [news_num, 400] representations util.py:24-33 caches.  Three stages:
//   A. [Q|K|V] = embedding[tokens] [W_Q|W_K|W_V]^T (+ b_Q, -, b_V): the strip-mined bf16x6 GEMM with the embedding
//      lookup folded into its operand DMA (the token ids are the row list of A; "gather only");
//   B. per title and head: softmax(Q K^T / sqrt(d_k)) V, no padding mask (layers.py:84-87), ReLU (newsEncoders.py:78);
//   C. additive attention pooling: a_t = affine2 . tanh(affine1 h_t + b), -1e9 on padding, softmax over the title,
//      sum_t alpha_t h_t (layers.py:108-114); the affine1 product is one more bf16x6 GEMM (its rows zero-padded to a
//      multiple of 80), the rest one small kernel per title.  This stage is the CNN encoder's too (digat_cnn.inc): news_pool_fwd
//      below is the one place it is launched from, for both encoders, inference and training.
// Included at the end of digat_kernels.hip.

// embeddings of the listed tokens as a dense matrix (fallback when the GEMM cannot take the row list)
__global__ void __launch_bounds__(256) gather_embedding_kernel(const float4* table, const int* tokens, float4* out, long M, int d4) {
    const long total = M * d4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / d4;
        out[i] = table[(long)tokens[r] * d4 + (i - r * d4)];
    }
}

// Stage B.  One workgroup per title, wave w takes heads w, w+4, ...  Lane i owns query row i: its scores over the
// keys live in LDS (row stride Lw+1), K and V rows are LDS broadcasts, the softmax is in-lane.
struct MsaAttnArgs { const float* qkv; float* h; int T, Lw, heads, dk; };
constexpr int MSA_MAX_DK = 32;

__global__ void __launch_bounds__(256) msa_attention_kernel(const MsaAttnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Lw = g.Lw, dk = g.dk, hd = g.heads * g.dk;
    const int t = blockIdx.x;
    float* Ks = reinterpret_cast<float*>(smem) + (size_t)wave * (2 * Lw * dk + Lw * (Lw + 1));   // per-wave: K, V, scores
    float* Vs = Ks + Lw * dk;
    float* Ss = Vs + Lw * dk;
    const float* base = g.qkv + (long)t * Lw * 3 * hd;
    const float scale = 1.f / sqrtf((float)dk);
    for (int head = wave; head < g.heads; head += 4) {
        // K_h, V_h of the title -> LDS (this wave's region; only this wave reads it)
        for (int e = lane; e < Lw * dk; e += 64) {
            const int j = e / dk, c = e - j * dk;
            Ks[e] = base[(long)j * 3 * hd + hd + head * dk + c];
            Vs[e] = base[(long)j * 3 * hd + 2 * hd + head * dk + c];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): the stores above are in LDS before this wave reads them
        __builtin_amdgcn_wave_barrier();
        for (int i0 = 0; i0 < Lw; i0 += 64) {
            const int i = i0 + lane;
            if (i < Lw) {
                float q[MSA_MAX_DK];
#pragma unroll
                for (int c = 0; c < MSA_MAX_DK; ++c) q[c] = c < dk ? base[(long)i * 3 * hd + head * dk + c] : 0.f;
                float m = -INFINITY;
                for (int j = 0; j < Lw; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < MSA_MAX_DK; ++c)
                        if (c < dk) s = fmaf(q[c], Ks[j * dk + c], s);
                    s *= scale;
                    Ss[i * (Lw + 1) + j] = s;
                    m = fmaxf(m, s);
                }
                float den = 0.f;
                for (int j = 0; j < Lw; ++j) {
                    const float e = expf(Ss[i * (Lw + 1) + j] - m);
                    Ss[i * (Lw + 1) + j] = e;
                    den += e;
                }
                float o[MSA_MAX_DK];
#pragma unroll
                for (int c = 0; c < MSA_MAX_DK; ++c) o[c] = 0.f;
                for (int j = 0; j < Lw; ++j) {
                    const float al = Ss[i * (Lw + 1) + j] / den;
#pragma unroll
                    for (int c = 0; c < MSA_MAX_DK; ++c)
                        if (c < dk) o[c] = fmaf(al, Vs[j * dk + c], o[c]);
                }
                float* out = g.h + ((long)t * Lw + i) * hd + head * dk;
#pragma unroll
                for (int c = 0; c < MSA_MAX_DK; ++c)
                    if (c < dk) out[c] = fmaxf(o[c], 0.f);          // ReLU (newsEncoders.py:78)
            }
        }
        __builtin_amdgcn_wave_barrier();           // the next head overwrites K / V
    }
}

// Stage B on the matrix cores (Lw <= 32, d_k <= 32): per head two tiny products, v_mfma_f32_16x16x4_f32 (exact fp32).
//   S^T = K Q^T : tile (tj, ti), lane (lr, lq) ends with S[i = 16 ti + lr][j = 16 tj + 4 lq + r], r = 0..3
//   softmax over j for every i: in-lane over (tj, r), then over the four lq lane groups (two xor-shuffles)
//   out = alpha V: the k-step (tj, r) of the second product sums over j = 16 tj + 4 lq' + r, lq' = 0..3 — lane lq holds
//   exactly alpha[i][16 tj + 4 lq + r] in its accumulator, so alpha is the A operand as it stands (no transposition
//   through LDS); V rows are read in the matching order.
// Q, K, V of a head sit in LDS per wave (rows padded: 28-float k for Q/K... generally 4*ceil(dk/4); V 32 columns).
template <int KS>      // k steps of the first product: padded head dim kp = 4 KS >= d_k
__global__ void __launch_bounds__(256) msa_attention_mfma_kernel(const MsaAttnArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int Lw = g.Lw, dk = g.dk, hd = g.heads * g.dk;
    constexpr int ks_n = KS, kp = KS * 4;
    const int t = blockIdx.x;
    float* Qs = reinterpret_cast<float*>(smem) + (size_t)wave * (2 * 32 * kp + 32 * 33);
    float* Ks = Qs + 32 * kp;
    float* Vs = Ks + 32 * kp;                                 // [32][33]
    const float* base = g.qkv + (long)t * Lw * 3 * hd;
    const float scale = 1.f / sqrtf((float)dk);
    // A head's Q, K, V are requested while the previous head is computed: the registers are free once their values are in LDS.
    // Straight-line clamped loads (compile-time trip counts: all in flight together); tile padding is zeroed at the LDS store.
    constexpr int QK_IT = (32 * kp + 63) / 64;
    float rq[QK_IT], rk[QK_IT], rv[16];
    auto request = [&](int head) {
#pragma unroll
        for (int u = 0; u < QK_IT; ++u) {
            const int e = lane + 64 * u;
            const int j = min(e / kp, Lw - 1), c = min(e - (e / kp) * kp, dk - 1);
            rq[u] = base[(long)j * 3 * hd + head * dk + c];
            rk[u] = base[(long)j * 3 * hd + hd + head * dk + c];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = lane + 64 * u;
            const int j = min(e >> 5, Lw - 1), c = min(e & 31, dk - 1);
            rv[u] = base[(long)j * 3 * hd + 2 * hd + head * dk + c];
        }
    };
    if (wave < g.heads) request(wave);
    for (int head = wave; head < g.heads; head += 4) {
#pragma unroll
        for (int u = 0; u < QK_IT; ++u) {
            const int e = lane + 64 * u;
            const int j = e / kp, c = e - j * kp;
            const bool ok = j < Lw && c < dk;
            if (e < 32 * kp) { Qs[e] = ok ? rq[u] : 0.f; Ks[e] = ok ? rk[u] : 0.f; }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = lane + 64 * u;
            Vs[(e >> 5) * 33 + (e & 31)] = ((e >> 5) < Lw && (e & 31) < dk) ? rv[u] : 0.f;
        }
        if (head + 4 < g.heads) request(head + 4);
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        v4f s[2][2];                               // [tj][ti]
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) s[tj][ti] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < ks_n; ++ks) {
            const int k = ks * 4 + lq;
            const float k0 = Ks[lr * kp + k], k1 = Ks[(16 + lr) * kp + k];
            const float q0 = Qs[lr * kp + k], q1 = Qs[(16 + lr) * kp + k];
            s[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, q0, s[0][0], 0, 0, 0);
            s[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, q1, s[0][1], 0, 0, 0);
            s[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, q0, s[1][0], 0, 0, 0);
            s[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, q1, s[1][1], 0, 0, 0);
        }
        // softmax over j (keys) for i = 16 ti + lr; keys j >= Lw are padding of the tile, not of the title: excluded
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            float m = -INFINITY;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = tj * 16 + 4 * lq + r;
                    const float x = j < Lw ? s[tj][ti][r] * scale : -INFINITY;
                    s[tj][ti][r] = x;
                    m = fmaxf(m, x);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float den = 0.f;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = expf(s[tj][ti][r] - m);        // exp(-inf) = 0 on the tile padding
                    s[tj][ti][r] = e;
                    den += e;
                }
            den += __shfl_xor(den, 16, 64);
            den += __shfl_xor(den, 32, 64);
            const float inv = 1.f / den;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[tj][ti][r] *= inv;
        }
        v4f o[2][2];                               // [ti][ct]
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) o[ti][ct] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = tj * 16 + 4 * lq + r;
                const float v0 = Vs[j * 33 + lr], v1 = Vs[j * 33 + 16 + lr];
                o[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[tj][0][r], v0, o[0][0], 0, 0, 0);
                o[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[tj][0][r], v1, o[0][1], 0, 0, 0);
                o[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[tj][1][r], v0, o[1][0], 0, 0, 0);
                o[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[tj][1][r], v1, o[1][1], 0, 0, 0);
            }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * 16 + 4 * lq + r, c = ct * 16 + lr;
                    if (i < Lw && c < dk) g.h[((long)t * Lw + i) * hd + head * dk + c] = fmaxf(o[ti][ct][r], 0.f);   // ReLU
                }
        __builtin_amdgcn_wave_barrier();           // the next head overwrites Q / K / V
    }
}

// Stage C after the affine1 GEMM: one workgroup per title.
struct MsaPoolArgs { const float* pre; int ldp; const float* b1; const float* a2; const float* h; const uint8_t* mask; float* out; int T, Lw, att, hd;
                     float* alpha_out; };     // optional [T, Lw]: the pooling weights, kept for the backward (digat_msa_fwd_train)

__global__ void __launch_bounds__(256) msa_pool_kernel(const MsaPoolArgs g) {
    __shared__ float al[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x, Lw = g.Lw;
    for (int j = wave; j < Lw; j += 4) {
        const float* row = g.pre + ((long)t * Lw + j) * g.ldp;
        float part = 0.f;
        for (int c = lane; c < g.att; c += 64) part = fmaf(g.a2[c], tanhf(row[c] + g.b1[c]), part);
        part = wave_sum(part);
        if (lane == 0) al[j] = g.mask[(long)t * Lw + j] ? part : -1e9f;       // masked_fill(mask == 0, -1e9)
    }
    __syncthreads();
    if (wave == 0) {
        const float v = lane < Lw ? al[lane] : -INFINITY;
        const float m = wave_max(v);
        const float e = lane < Lw ? expf(v - m) : 0.f;
        const float den = wave_sum(e);
        if (lane < Lw) al[lane] = e / den;
        if (g.alpha_out && lane < Lw) g.alpha_out[(long)t * Lw + lane] = e / den;
    }
    __syncthreads();
    const float* hb = g.h + (long)t * Lw * g.hd;
    for (int c = threadIdx.x; c < g.hd; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < Lw; ++j) acc = fmaf(al[j], hb[(long)j * g.hd + c], acc);
        g.out[(long)t * g.hd + c] = acc;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// attention_dim (or any column count) rounded up to the 80-column strips of the bf16x6 GEMM
static size_t msa_attp(int att) { return ((size_t)att + 79) / 80 * 80; }

// out [M, dm] = table[tokens]
static int launch_gather_embedding(const float* table, const int32_t* tokens, float* out, long M, int dm, hipStream_t st) {
    hipLaunchKernelGGL(gather_embedding_kernel, dim3(grid_for(M * (dm / 4))), dim3(256), 0, st, (const float4*)table, tokens, (float4*)out, M,
                       dm / 4);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// Stage B: the matrix-core kernel up to 32 words a title, the LDS-broadcast one above
static int launch_msa_attention(const float* qkv, float* h, int T, int Lw, int heads, int dk, hipStream_t st) {
    MsaAttnArgs a{qkv, h, T, Lw, heads, dk};
    if (Lw <= 32) {
        const int ks = (dk + 3) / 4, kp = ks * 4;
        const size_t lds = (size_t)4 * (2 * 32 * kp + 32 * 33) * 4;
        switch (ks) {
            case 1: hipLaunchKernelGGL(msa_attention_mfma_kernel<1>, dim3(T), dim3(256), lds, st, a); break;
            case 2: hipLaunchKernelGGL(msa_attention_mfma_kernel<2>, dim3(T), dim3(256), lds, st, a); break;
            case 3: hipLaunchKernelGGL(msa_attention_mfma_kernel<3>, dim3(T), dim3(256), lds, st, a); break;
            case 4: hipLaunchKernelGGL(msa_attention_mfma_kernel<4>, dim3(T), dim3(256), lds, st, a); break;
            case 5: hipLaunchKernelGGL(msa_attention_mfma_kernel<5>, dim3(T), dim3(256), lds, st, a); break;
            case 6: hipLaunchKernelGGL(msa_attention_mfma_kernel<6>, dim3(T), dim3(256), lds, st, a); break;
            case 7: hipLaunchKernelGGL(msa_attention_mfma_kernel<7>, dim3(T), dim3(256), lds, st, a); break;
            default: hipLaunchKernelGGL(msa_attention_mfma_kernel<8>, dim3(T), dim3(256), lds, st, a); break;
        }
    } else {
        // up to 132 096 B (Lw = 64, d_k = 32) of the CU's 160 KiB: above 64 KiB a launch has to opt in (as cnn_launch_conv does)
        const size_t lds = (size_t)4 * (2 * Lw * dk + Lw * (Lw + 1)) * 4;
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)msa_attention_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess) return DIGAT_ERR_LAUNCH;
        hipLaunchKernelGGL(msa_attention_kernel, dim3(T), dim3(256), lds, st, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// Stage C of BOTH news encoders, inference and training (h [T Lw, hd]: hd = heads * d_k, or the CNN's kernel_num): pre = h A1^T
// without the bias (the pooling kernel adds it), then msa_pool_kernel; `alpha` (optional [T, Lw]) keeps the pooling weights for the
// backward.  `a1_image`: a ready split image of A1, or NULL — whether one exists is the caller's decision; with it the product runs
// over attp = att rounded up to 80 columns (the image holds zero rows there; those columns of `pre` are never read).  `bf16_ok`:
// under digat_set_train_precision(1) the image's product may run on the bf16 single-product segments.
static int news_pool_fwd(const float* h, int hd, const float* A1, const void* a1_image, const float* b1, const float* a2, float* pre,
                         const uint8_t* mask, float* out, float* alpha, int T, int Lw, int att, bool bf16_ok, hipStream_t st) {
    const long M = (long)T * Lw;
    const int attp = (int)msa_attp(att);
    GemmArgs ga = gemm_plain(h, hd, A1, nullptr, pre, attp, (int)M, att, hd, 0);
    if (a1_image) {
        GemmArgs gx = ga;
        gx.nseg = attp; gx.wsplit = (const unsigned short*)a1_image;
        if (bf16_ok && g_train_bf16) gx.x1_segs = 7;
        if (gemm_takes_row_list(gx)) ga = gx;
    }
    T_TRY(launch_gemm(ga, st, DIGAT_KERNEL_LINEAR));
    MsaPoolArgs pa{pre, attp, b1, a2, h, mask, out, T, Lw, att, hd, alpha};
    hipLaunchKernelGGL(msa_pool_kernel, dim3(T), dim3(256), 0, st, pa);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// the inference workspace: qkv, h, the affine1 product, and the embedded tokens for shapes whose GEMM cannot take the row list
struct MsaFwdWs { float *qkv, *h, *pre, *emb; };
static size_t msa_fwd_carve(Arena& w, int T, int Lw, int dm, int hd, int att, MsaFwdWs* o) {
    const size_t M = (size_t)T * Lw;
    o->qkv = w.take<float>(M * 3 * hd); o->h = w.take<float>(M * hd); o->pre = w.take<float>(M * msa_attp(att)); o->emb = w.take<float>(M * dm);
    return w.used;
}

extern "C" {

size_t digat_msa_split_bytes(int word_embedding_dim, int head_num, int head_dim) {
    return digat_split_weights_bytes(3 * head_num * head_dim, word_embedding_dim);
}
int digat_split_msa_weights(const float* W_Q, const float* W_K, const float* W_V, int word_embedding_dim, int hd,
                            void* wsplit, void* stream) {
    if (!W_Q || !W_K || !W_V || !wsplit || word_embedding_dim <= 0 || hd <= 0) return DIGAT_ERR_ARG;
    return launch_split(W_Q, W_K, W_V, hd, 3, word_embedding_dim, wsplit, (hipStream_t)stream, 0, DIGAT_GEMM_BF16X6);
}

size_t digat_msa_workspace_bytes(int T, int Lw, int dm, int heads, int dk, int att) {
    Arena measure;
    MsaFwdWs o;
    return msa_fwd_carve(measure, T, Lw, dm, heads * dk, att, &o);
}

int digat_msa_fwd(const digat_msa_params* p, const int32_t* title_text, const uint8_t* title_mask, float* out,
                  int T, int Lw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !title_text || !title_mask || !out || !workspace || T < 0 || Lw <= 0) return DIGAT_ERR_ARG;
    const int dm = p->word_embedding_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    const int hd = heads * dk;
    if (dm <= 0 || dm % 4 || heads <= 0 || dk <= 0 || dk > MSA_MAX_DK || att <= 0 || hd % 4 || Lw > 64) return DIGAT_ERR_SHAPE;
    Arena w(workspace, workspace_bytes);
    MsaFwdWs o;
    msa_fwd_carve(w, T, Lw, dm, hd, att, &o);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    if (T == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)T * Lw;

    // A. [Q|K|V]
    GemmArgs g = gemm_plain(p->word_embedding, dm, p->W_Q, p->b_Q, o.qkv, 3 * hd, (int)M, hd, dm, 0);
    g.w[1] = p->W_K; g.bias[1] = nullptr; g.y[1] = o.qkv + hd;
    g.w[2] = p->W_V; g.bias[2] = p->b_V; g.y[2] = o.qkv + 2 * hd;
    g.nsegs = 3;
    g.wsplit = (const unsigned short*)p->qkv_wsplit;
    g.rowidx = title_text; g.gather_only = 1;
    if (!gemm_takes_row_list(g)) {                 // small / odd shapes: materialise the embeddings, then the generic dispatch
        T_TRY(launch_gather_embedding(p->word_embedding, title_text, o.emb, M, dm, st));
        g.a0 = o.emb; g.rowidx = nullptr; g.gather_only = 0; g.wsplit = nullptr;
    }
    T_TRY(launch_gemm(g, st, DIGAT_KERNEL_LINEAR));
    // B. attention + ReLU
    T_TRY(launch_msa_attention(o.qkv, o.h, T, Lw, heads, dk, st));
    // C. pooling (inference: fp32-grade whatever the training precision)
    return news_pool_fwd(o.h, hd, p->A1, p->a1_wsplit, p->b1, p->a2, o.pre, title_mask, out, nullptr, T, Lw, att, false, st);
}

}  // extern "C"
