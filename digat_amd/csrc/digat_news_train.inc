// digat_news_train.inc — MSA news encoder, training forward and backward (SURVEY §8f-2; reference: newsEncoders.py:70-82,
// layers.py:75-88 MultiHeadAttention.forward, layers.py:107-115 Attention.forward).  One C-ABI call per direction, like the
// graph encoder's pairs (digat_train_abi.inc): what the backward needs travels in a caller-owned `save` buffer.
//   forward:  Ed = dropout_p(embedding[tokens]);  [Q|K|V] = Ed [W_Q|W_K|W_V]^T + [b_Q|0|b_V];  per title and head
//             O = softmax(Q K^T / sqrt(d_k)) V;  h = relu(O);  pre = h A1^T;  a_t = a2 . tanh(pre_t + b1), -1e9 on padding;
//             alpha = softmax_t(a);  out = sum_t alpha_t h_t
//   backward: the pooling (alpha, tanh), affine1 (two GEMMs), ReLU, the attention (S and alpha RECOMPUTED from Q, K: nothing
//             of size Lw^2 is saved), the three projections (input and weight gradients), dropout, and the embedding rows
//             summed per token in a fixed order (bit-reproducible, no atomics).
// The pooling stage's backward (news_pool_bwd) also serves the CNN encoder (digat_cnn.inc).
// Included by digat_kernels.hip after digat_news.inc.

// ---- embedding rows of the listed tokens (float4) ---------------------------------------------------------------
// (gather_embedding_kernel of digat_news.inc; the dropout is digat_dropout_fwd in place)

// ---- pooling backward: one workgroup per title ---------------------------------------------------------------
//   dal_j = dout . h_j;  da_j = mask_j ? alpha_j (dal_j - sum_s alpha_s dal_s) : 0   (masked_fill: no gradient to a masked score)
//   dh[j] = alpha_j dout  (the affine1 path is added by the GEMM that follows);  th = tanh(pre + b1):
//   dpre[j][c] = da_j a2_c (1 - th^2)  (columns att..ldp-1, the GEMM's padding, = 0);  da2 partial[t][c] = sum_j da_j th_jc
struct MsaPoolBwdArgs {
    const float* dout; const float* h; const float* pre; int ldp; const float* b1; const float* a2; const float* alpha; const uint8_t* mask;
    float* dh; float* dpre; float* da2_part; int T, Lw, att, hd;
};
__global__ void __launch_bounds__(256) msa_pool_bwd_kernel(const MsaPoolBwdArgs g) {
    __shared__ float dal[64], da[64], al[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int t = blockIdx.x, Lw = g.Lw, hd = g.hd;
    const float* hb = g.h + (long)t * Lw * hd;
    const float* dob = g.dout + (long)t * hd;
    for (int j = wave; j < Lw; j += 4) {
        float part = 0.f;
        for (int c = lane; c < hd; c += 64) part = fmaf(dob[c], hb[(long)j * hd + c], part);
        part = wave_sum(part);
        if (lane == 0) dal[j] = part;
    }
    if (tid < Lw) al[tid] = g.alpha[(long)t * Lw + tid];
    __syncthreads();
    if (wave == 0) {
        const float a = lane < Lw ? al[lane] : 0.f, x = lane < Lw ? dal[lane] : 0.f;
        const float dot = wave_sum(a * x);
        if (lane < Lw) da[lane] = g.mask[(long)t * Lw + lane] ? a * (x - dot) : 0.f;
    }
    __syncthreads();
    float* dhb = g.dh + (long)t * Lw * hd;
    for (int e = tid; e < Lw * hd; e += 256) {
        const int j = e / hd, c = e - j * hd;
        dhb[e] = al[j] * dob[c];
    }
    const float* pb = g.pre + (long)t * Lw * g.ldp;
    float* dpb = g.dpre + (long)t * Lw * g.ldp;
    for (int c = tid; c < g.ldp; c += 256) {
        if (c < g.att) {
            const float a2c = g.a2[c], b = g.b1[c];
            float s = 0.f;
            for (int j = 0; j < Lw; ++j) {
                const float th = tanhf(pb[(long)j * g.ldp + c] + b);
                dpb[(long)j * g.ldp + c] = da[j] * a2c * (1.f - th * th);
                s = fmaf(da[j], th, s);
            }
            g.da2_part[(long)t * g.att + c] = s;
        } else {
            for (int j = 0; j < Lw; ++j) dpb[(long)j * g.ldp + c] = 0.f;
        }
    }
}

// ---- attention backward on the fp32 matrix cores: one workgroup (two waves) per title, wave w takes heads w, w+2, ... ----------
// With dO = dh . [h > 0] (ReLU), s = 1/sqrt(d_k):  S = s Q K^T, alpha = softmax_j(S) (recomputed as in msa_attention_mfma_kernel),
//   dalpha = dO V^T;  delta_i = sum_j alpha_ij dalpha_ij;  dS = s alpha (dalpha - delta);
//   dQ = dS K;  dK = dS^T Q;  dV = alpha^T dO.
// v_mfma_f32_16x16x4_f32 tiles, Lw <= 32, d_k <= 32.  The transposed score tile (lane (lr, lq) holds [i = 16 ti + lr]
// [j = 16 tj + 4 lq + r]) makes the softmax and delta in-lane + two xor-shuffles, and is the A operand of dQ = dS K as it stands;
// dK and dV need the other orientation: alpha and dS go through LDS once.  Q, K, V, dO: [32][33] images per wave.
struct MsaAttnBwdArgs { const float* qkv; const float* h; const float* dh; float* dqkv; int T, Lw, heads, dk; };
constexpr int MSA_BWD_IMG = 32 * 33;

__global__ void __launch_bounds__(128) msa_attention_bwd_kernel(const MsaAttnBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int Lw = g.Lw, dk = g.dk, hd = g.heads * g.dk;
    const int t = blockIdx.x;
    float* Qs = reinterpret_cast<float*>(smem) + (size_t)wave * 5 * MSA_BWD_IMG;
    float* Ks = Qs + MSA_BWD_IMG;
    float* Vs = Ks + MSA_BWD_IMG;        // V, then alpha
    float* Os = Vs + MSA_BWD_IMG;        // dO
    float* Ds = Os + MSA_BWD_IMG;        // dS
    const float* base = g.qkv + (long)t * Lw * 3 * hd;
    const float* hb = g.h + (long)t * Lw * hd;
    const float* dhb = g.dh + (long)t * Lw * hd;
    float* dbase = g.dqkv + (long)t * Lw * 3 * hd;
    const float scale = 1.f / sqrtf((float)dk);
    const int ks_n = (dk + 3) >> 2;
    // a head's operands are requested while the previous head is computed: the registers are free once they are in LDS
    float rq[16], rk[16], rv[16], rh[16], rd[16];
    auto request = [&](int head) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = lane + 64 * u;
            const int j = min(e >> 5, Lw - 1), c = min(e & 31, dk - 1);      // clamped, straight-line loads; padding is zeroed at the store
            const long qo = (long)j * 3 * hd + head * dk + c, ho = (long)j * hd + head * dk + c;
            rq[u] = base[qo];
            rk[u] = base[qo + hd];
            rv[u] = base[qo + 2 * hd];
            rh[u] = hb[ho];
            rd[u] = dhb[ho];
        }
    };
    if (wave < g.heads) request(wave);
    for (int head = wave; head < g.heads; head += 2) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = lane + 64 * u;
            const bool ok = (e >> 5) < Lw && (e & 31) < dk;
            const int o = (e >> 5) * 33 + (e & 31);
            Qs[o] = ok ? rq[u] : 0.f; Ks[o] = ok ? rk[u] : 0.f; Vs[o] = ok ? rv[u] : 0.f;
            Os[o] = (ok && rh[u] > 0.f) ? rd[u] : 0.f;                       // ReLU (newsEncoders.py:79)
        }
        if (head + 2 < g.heads) request(head + 2);
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        v4f s[2][2], da[2][2];                     // [tj][ti]: S^T -> alpha; dalpha -> dS
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) { s[tj][ti] = (v4f){0.f, 0.f, 0.f, 0.f}; da[tj][ti] = (v4f){0.f, 0.f, 0.f, 0.f}; }
        for (int ks = 0; ks < ks_n; ++ks) {
            const int k = ks * 4 + lq;
            const float k0 = Ks[lr * 33 + k], k1 = Ks[(16 + lr) * 33 + k];
            const float q0 = Qs[lr * 33 + k], q1 = Qs[(16 + lr) * 33 + k];
            const float v0 = Vs[lr * 33 + k], v1 = Vs[(16 + lr) * 33 + k];
            const float o0 = Os[lr * 33 + k], o1 = Os[(16 + lr) * 33 + k];
            s[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, q0, s[0][0], 0, 0, 0);
            s[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(k0, q1, s[0][1], 0, 0, 0);
            s[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, q0, s[1][0], 0, 0, 0);
            s[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(k1, q1, s[1][1], 0, 0, 0);
            da[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, o0, da[0][0], 0, 0, 0);
            da[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, o1, da[0][1], 0, 0, 0);
            da[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, o0, da[1][0], 0, 0, 0);
            da[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, o1, da[1][1], 0, 0, 0);
        }
        // softmax over the keys j for i = 16 ti + lr (as the forward kernel: keys j >= Lw are tile padding), then dS
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
                    const float e = expf(s[tj][ti][r] - m);
                    s[tj][ti][r] = e;
                    den += e;
                }
            den += __shfl_xor(den, 16, 64);
            den += __shfl_xor(den, 32, 64);
            const float inv = 1.f / den;
            float delta = 0.f;
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[tj][ti][r] *= inv;
                    delta = fmaf(s[tj][ti][r], da[tj][ti][r], delta);
                }
            delta += __shfl_xor(delta, 16, 64);
            delta += __shfl_xor(delta, 32, 64);
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) da[tj][ti][r] = scale * s[tj][ti][r] * (da[tj][ti][r] - delta);
        }
        // alpha (over V: every read of V precedes these writes in the wave's LDS queue) and dS to LDS as [i][j]
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = (16 * ti + lr) * 33 + 16 * tj + 4 * lq + r;
                    Vs[o] = s[tj][ti][r];
                    Ds[o] = da[tj][ti][r];
                }
        // dQ = dS K: dS is the A operand as it stands (lane lq holds k = j = 16 tj + 4 lq + r of k-step (tj, r))
        v4f o[2][2];                               // [row tile][channel tile]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) o[a][ct] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = tj * 16 + 4 * lq + r;
                const float b0 = Ks[j * 33 + lr], b1 = Ks[j * 33 + 16 + lr];
                o[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[tj][0][r], b0, o[0][0], 0, 0, 0);
                o[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[tj][0][r], b1, o[0][1], 0, 0, 0);
                o[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[tj][1][r], b0, o[1][0], 0, 0, 0);
                o[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[tj][1][r], b1, o[1][1], 0, 0, 0);
            }
        auto store = [&](int seg) {                // o[row tile][channel tile]: rows 16 a + 4 lq + r, channel 16 ct + lr
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = a * 16 + 4 * lq + r, c = ct * 16 + lr;
                        if (row < Lw && c < dk) dbase[(long)row * 3 * hd + seg * hd + head * dk + c] = o[a][ct][r];
                    }
        };
        store(0);
        __builtin_amdgcn_s_waitcnt(0xc07f);        // alpha and dS are in LDS
        __builtin_amdgcn_wave_barrier();
        // dK = dS^T Q and dV = alpha^T dO: A[m = j][k = i] read from the LDS images, k-step st covers i = 4 st + lq
        v4f p[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) { o[a][ct] = (v4f){0.f, 0.f, 0.f, 0.f}; p[a][ct] = (v4f){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const int i = 4 * st + lq;
            const float d0 = Ds[i * 33 + lr], d1 = Ds[i * 33 + 16 + lr];
            const float a0 = Vs[i * 33 + lr], a1 = Vs[i * 33 + 16 + lr];
            const float q0 = Qs[i * 33 + lr], q1 = Qs[i * 33 + 16 + lr];
            const float g0 = Os[i * 33 + lr], g1 = Os[i * 33 + 16 + lr];
            o[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, q0, o[0][0], 0, 0, 0);
            o[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(d0, q1, o[0][1], 0, 0, 0);
            o[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, q0, o[1][0], 0, 0, 0);
            o[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(d1, q1, o[1][1], 0, 0, 0);
            p[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, g0, p[0][0], 0, 0, 0);
            p[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, g1, p[0][1], 0, 0, 0);
            p[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, g0, p[1][0], 0, 0, 0);
            p[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, g1, p[1][1], 0, 0, 0);
        }
        store(1);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) o[a][ct] = p[a][ct];
        store(2);
        __builtin_amdgcn_wave_barrier();           // the next head overwrites the images
    }
}

// ---- embedding gradient: rows summed per token in a fixed order ---------------------------------------------------------
// `order` lists the row indices sorted by token (stable: ascending row within a token), `stok` the tokens in that order.  A
// workgroup owns EMB_CHUNK consecutive sorted positions and walks them in order; a run of equal tokens that begins and ends
// inside the chunk is complete and goes to table_grad[token]; the first / last run when it continues across the chunk border is
// a partial: part[2k] / part[2k+1] (+ its token, -1 = none; empty slots only ever lie between DIFFERENT tokens).  The partials,
// in chunk order, are again rows sorted by token: the same kernel reduces them (order = NULL: identity) until one chunk is left,
// where every run is complete.
constexpr int EMB_CHUNK = 64;
struct EmbBwdArgs { const float* rows; long ld; const int* order; const int* stok; long n; int dm; float* table_grad; float* part; int* part_tok; };
__global__ void __launch_bounds__(256) embedding_bwd_kernel(const EmbBwdArgs g) {
    __shared__ int tok[EMB_CHUNK + 2], src[EMB_CHUNK];
    const long p0 = (long)blockIdx.x * EMB_CHUNK;
    const int cnt = (int)(g.n - p0 < EMB_CHUNK ? g.n - p0 : EMB_CHUNK);
    const int tid = threadIdx.x;
    if (tid < cnt) { tok[tid + 1] = g.stok[p0 + tid]; src[tid] = g.order ? g.order[p0 + tid] : (int)(p0 + tid); }
    if (tid == 0) tok[0] = p0 > 0 ? g.stok[p0 - 1] : -2;                      // -2: no neighbour (never a token; -1 = empty entry)
    if (tid == 1) tok[cnt + 1] = p0 + cnt < g.n ? g.stok[p0 + cnt] : -2;
    __syncthreads();
    const bool head_open = tok[1] == tok[0] && tok[1] >= 0, tail_open = tok[cnt] == tok[cnt + 1] && tok[cnt] >= 0;
    if (tid < 2) g.part_tok[2 * (long)blockIdx.x + tid] = -1;
    __syncthreads();
    for (int c = tid; c < g.dm; c += 256) {
        float acc = 0.f;
        int run_start = 0;
        for (int q = 0; q < cnt; ++q) {
            const int tk = tok[q + 1];
            if (tk >= 0) acc += g.rows[(long)src[q] * g.ld + c];
            if (q + 1 == cnt || tok[q + 2] != tk) {                            // the run ends here
                if (tk >= 0) {
                    const bool open_h = run_start == 0 && head_open, open_t = q + 1 == cnt && tail_open;
                    if (open_h || open_t) {
                        const long slot = 2 * (long)blockIdx.x + (open_h ? 0 : 1);
                        g.part[slot * g.dm + c] = acc;
                        if (c == 0) g.part_tok[slot] = tk;
                        if (open_h && open_t) {          // one run across the whole chunk: the second slot carries the token with a zero
                            g.part[(slot + 1) * g.dm + c] = 0.f;      // row, so that a token's partials stay ADJACENT in the next level
                            if (c == 0) g.part_tok[slot + 1] = tk;
                        }
                    } else {
                        g.table_grad[(long)tk * g.dm + c] = acc;
                    }
                }
                acc = 0.f;
                run_start = q + 1;
            }
        }
    }
}

// ---- the same sum without a sorted order: a few thousand looked-up rows of a WIDE table (the news-embedding rows of a training
// step: 2 x 3 200 ids into 65 k rows of 400 floats) in two launches, where torch's embedding backward sorts, scans and scatters
// (18 launches per lookup at these sizes).  A wave per position p, twice:
//   1. inside p's chunk of 64 positions: the FIRST position of an id in the chunk adds the gradient rows of the chunk's positions
//      with that id, ascending, into part[p] and flags itself (a padding id fills whole chunks: 64 rows per wave, not thousands);
//   2. over all chunks: the first position of an id overall adds the flagged partial rows of its id in ascending chunk order
//      (at most M / 64 of them) and writes table_grad[id] once.  Who is first overall and how many partial rows an id has come from
//      an integer atomicMin / count per id in launch 1 (order-independent results): most ids occur in one chunk and need no scan.
// Fixed summation order, no floating-point atomics; ids come as two lists (the second list's positions follow the first's: the candidate graphs' nodes and
// the histories are looked up in one table); an id outside [0, V) receives nothing.
struct EmbScanArgs { const int64_t* ids0; const float* g0; long ld0; int M0; const int64_t* ids1; const float* g1; long ld1; int M1;
                     int dm; long V; float* table_grad; float* part; int* key;      // key[p] = p's id if p is the first of its chunk with it, else -1
                     unsigned* head; unsigned* left; };   // per id: the smallest such p (atomicMin), 0xFFFFFFFF - their count (both start as 0xFF bytes)
// acc (+)= the rows `row_of(t)` of the set bits t of `hits`, ascending, eight rows in flight (the sums are chains of dependent
// round trips: ~2 us each when taken one at a time)
template <int U, class RowOf>
__device__ __forceinline__ void emb_add_rows(unsigned long long hits, float4 (&acc)[U], int d4, int lane, RowOf row_of) {
    while (hits) {
        const float4* r[8];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (hits) { r[k] = row_of(__builtin_ctzll(hits)); hits &= hits - 1; cnt = k + 1; } else r[k] = r[0];
        }
        float4 v[8][U];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u) v[k][u] = r[k][min(lane + 64 * u, d4 - 1)];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < cnt) {                       // wave-uniform
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = f4_add(acc[u], v[k][u]);
            }
    }
}
template <int U>      // float4 pieces per lane: dm <= 256 U
__global__ void __launch_bounds__(256) embedding_bwd_chunk_kernel(const EmbScanArgs g) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), M = g.M0 + g.M1;
    if (p >= M) return;
    auto id_at = [&](int q) -> long { return q < g.M0 ? (long)g.ids0[q] : (long)g.ids1[q - g.M0]; };
    const int p0 = p & ~63, q = p0 + lane;
    const long theirs = id_at(min(q, M - 1));
    const long mine = __shfl(theirs, p - p0);                     // wave-uniform
    const unsigned long long hits = __ballot(q < M && theirs == mine);
    const bool first = mine >= 0 && mine < g.V && __builtin_ctzll(hits) == p - p0;
    if (lane == 0) {
        g.key[p] = first ? (int)mine : -1;
        if (first) {                              // integer min / count: the same result in any order of arrival
            atomicMin(g.head + mine, (unsigned)p);
            atomicSub(g.left + mine, 1u);
        }
    }
    if (!first) return;
    const int d4 = g.dm >> 2;
    float4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f4_zero();
    emb_add_rows<U>(hits, acc, d4, lane, [&](int t) {
        const int src = p0 + t;
        return reinterpret_cast<const float4*>(src < g.M0 ? g.g0 + (long)src * g.ld0 : g.g1 + (long)(src - g.M0) * g.ld1);
    });
    float4* out = reinterpret_cast<float4*>(g.part + (long)p * g.dm);
#pragma unroll
    for (int u = 0; u < U; ++u) if (lane + 64 * u < d4) out[lane + 64 * u] = acc[u];
}
template <int U>
__global__ void __launch_bounds__(256) embedding_bwd_merge_kernel(const EmbScanArgs g) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), M = g.M0 + g.M1;
    if (p >= M) return;
    const int mine = g.key[p];                                    // wave-uniform
    if (mine < 0 || g.head[mine] != (unsigned)p) return;          // the first position overall owns the row
    int todo = (int)(0xFFFFFFFFu - g.left[mine]);                 // chunk partials of this id: 1 for most ids (no scan then)
    const int d4 = g.dm >> 2;
    float4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f4_zero();
    // the key list is scanned eight chunks per step, all eight loads in flight, until every partial row has been found
    const bool single = todo == 1;                                // only p's own chunk holds the id: one key load, one row
    for (int q0 = p & ~63; q0 < M && todo > 0; q0 += 512) {
        int k[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) k[t] = !single || t == 0 ? g.key[min(q0 + 64 * t + lane, M - 1)] : -1;
        // a chunk holds at most ONE partial row of an id (its first position there): the rows of the eight chunks are requested
        // together and added in chunk order (taken chunk by chunk, a heavy id — a padding id fills every chunk — is a chain of M / 64
        // dependent round trips: 74 us of this launch at 6 400 positions)
        float4 v[8][U];
        bool has[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int qb = q0 + 64 * t;
            const unsigned long long hits = __ballot(qb + lane < M && k[t] == mine);
            has[t] = hits != 0ull;                                 // wave-uniform
            const float4* row = reinterpret_cast<const float4*>(g.part + (long)(has[t] ? qb + __builtin_ctzll(hits) : p) * g.dm);
#pragma unroll
            for (int u = 0; u < U; ++u) v[t][u] = row[min(lane + 64 * u, d4 - 1)];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (has[t]) {
                --todo;
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] = f4_add(acc[u], v[t][u]);
            }
    }
    float4* out = reinterpret_cast<float4*>(g.table_grad + (long)mine * g.dm);
#pragma unroll
    for (int u = 0; u < U; ++u) if (lane + 64 * u < d4) out[lane + 64 * u] = acc[u];
}

struct MsaRowDropArgs { float* x; long ld; const uint8_t* mask; long M; int dm; float scale; };
__global__ void __launch_bounds__(256) msa_row_dropout_bwd_kernel(const MsaRowDropArgs g) {      // in place, rows ld apart, mask dense [M, dm]
    const long n = g.M * g.dm;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long r = e / g.dm;
        float* v = g.x + r * g.ld + (e - r * g.dm);
        *v = g.mask[e] ? *v * g.scale : 0.f;
    }
}

extern "C" {

// table_grad [V, dm] must be zero-filled by the caller (rows of tokens that do not occur stay zero).
size_t digat_embedding_bwd_workspace_bytes(int64_t M, int dm) {
    size_t total = 0;
    long n = M;
    while (n > EMB_CHUNK) {
        const long chunks = (n + EMB_CHUNK - 1) / EMB_CHUNK;
        total += align_up((size_t)2 * chunks * dm * 4, 256) + align_up((size_t)2 * chunks * 4, 256);
        n = 2 * chunks;
    }
    total += align_up((size_t)2 * dm * 4, 256) + 256;       // the last level's (unused) partial slots
    return total;
}
int digat_embedding_bwd(const float* row_grad, int64_t ld_row_grad, const int32_t* order, const int32_t* sorted_tokens, int64_t M, int dm,
                        float* table_grad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!row_grad || !order || !sorted_tokens || !table_grad || !workspace || M < 0 || dm <= 0 || ld_row_grad < dm) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_embedding_bwd_workspace_bytes(M, dm)) return DIGAT_ERR_WORKSPACE;
    if (M == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    Arena w(workspace, workspace_bytes);
    const float* rows = row_grad; const int* ord = order; const int* stok = sorted_tokens;
    long n = M, ld = ld_row_grad;
    for (;;) {
        const long chunks = (n + EMB_CHUNK - 1) / EMB_CHUNK;
        float* part = w.take<float>((size_t)2 * chunks * dm);
        int* ptok = w.take<int>((size_t)2 * chunks);
        if (!w.ok) return DIGAT_ERR_WORKSPACE;
        EmbBwdArgs a{rows, ld, ord, stok, n, dm, table_grad, part, ptok};
        hipLaunchKernelGGL(embedding_bwd_kernel, dim3((unsigned)chunks), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
        if (chunks == 1) break;
        rows = part; ld = dm; ord = nullptr; stok = ptok; n = 2 * chunks;
    }
    return DIGAT_OK;
}

// table_grad [V, dm] zero-filled by the caller; ids0 [M0] / ids1 [M1] int64 (ids1 may be NULL with M1 = 0), row gradients g0 / g1 with
// row strides ld0 / ld1; ids outside [0, V) receive nothing.  dm % 4 == 0, dm <= 1024.
static size_t emb_unsorted_ws(int64_t M, int dm, int64_t V) {
    return align_up((size_t)M * dm * 4, 256) + align_up((size_t)M * 4, 256) + align_up((size_t)V * 8, 256);
}
size_t digat_embedding_bwd_unsorted_workspace_bytes(int64_t M, int dm, int64_t V) { return emb_unsorted_ws(M, dm, V); }
int digat_embedding_bwd_unsorted(const int64_t* ids0, const float* g0, int64_t ld0, int64_t M0, const int64_t* ids1, const float* g1, int64_t ld1,
                                 int64_t M1, int dm, int64_t V, float* table_grad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table_grad || M0 < 0 || M1 < 0 || (M0 > 0 && (!ids0 || !g0)) || (M1 > 0 && (!ids1 || !g1)) || dm <= 0 || V <= 0) return DIGAT_ERR_ARG;
    if (dm % 4 || dm > 1024 || ld0 % 4 || ld1 % 4 || M0 + M1 > (1 << 24)) return DIGAT_ERR_SHAPE;
    const long M = M0 + M1;
    if (M == 0) return DIGAT_OK;
    if (V > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (!workspace || workspace_bytes < emb_unsorted_ws(M, dm, V)) return DIGAT_ERR_WORKSPACE;
    Arena w(workspace, workspace_bytes);
    float* part = w.take<float>((size_t)M * dm);
    int* key = w.take<int>((size_t)M);
    unsigned* head = w.take<unsigned>(2 * (size_t)V);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    EmbScanArgs a{ids0, g0, (long)ld0, (int)M0, ids1, g1, (long)ld1, (int)M1, dm, (long)V, table_grad, part, key, head, head + V};
    const dim3 grid((unsigned)((M + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(head, 0xFF, 2 * (size_t)V * 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    if (dm <= 256) {
        hipLaunchKernelGGL(embedding_bwd_chunk_kernel<1>, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(embedding_bwd_merge_kernel<1>, grid, dim3(256), 0, st, a);
    } else if (dm <= 512) {
        hipLaunchKernelGGL(embedding_bwd_chunk_kernel<2>, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(embedding_bwd_merge_kernel<2>, grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(embedding_bwd_chunk_kernel<4>, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(embedding_bwd_merge_kernel<4>, grid, dim3(256), 0, st, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// ---- the pooling stage's backward, shared with the CNN encoder (digat_cnn.inc) ---------------------------------------------
// the regions it works in; each encoder's training carve places them in its own layout
struct PoolBwdWs { void* a1t_img; float *dh, *dpre, *da2p, *da2g; };
// h [T Lw, hd], pre, alpha: what news_pool_fwd left in `save`.  Written: w.dh = alpha_j dout + dpre A1 (the gradient at h), dA1 [att, hd],
// db1, da2 [att].  wg / wgb: the encoder's weight-gradient scratch, at least digat_linear_bwd_weight_workspace(T Lw, att, hd) bytes.
static int news_pool_bwd(const float* dout, const float* h, int hd, const float* pre, const float* alpha, const uint8_t* mask, const float* A1,
                         const float* b1, const float* a2, const PoolBwdWs& w, void* wg, size_t wgb, float* dA1, float* db1, float* da2, int T, int Lw,
                         int att, hipStream_t st) {
    const long M = (long)T * Lw;
    const int attp = (int)msa_attp(att);
    MsaPoolBwdArgs pb{dout, h, pre, attp, b1, a2, alpha, mask, w.dh, w.dpre, w.da2p, T, Lw, att, hd};
    hipLaunchKernelGGL(msa_pool_bwd_kernel, dim3(T), dim3(256), 0, st, pb);
    DIGAT_CHECK_LAUNCH();
    const int per = 64, G = (T + per - 1) / per;       // da2 = the column sums of the per-title partials, in two levels
    hipLaunchKernelGGL(colsum_groups_kernel, dim3((att + 63) / 64, G), dim3(256), 0, st, (const float*)w.da2p, (long)att, w.da2g, T, att, per, (const int*)nullptr, 0);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_kernel, dim3((att + 63) / 64), dim3(256), 0, st, (const float*)w.da2g, (long)att, da2, G, att, 0, (const int*)nullptr, 0);
    DIGAT_CHECK_LAUNCH();
    // affine1: dh += dpre A1; dA1 = dpre^T h; db1 = colsum(dpre)
    if (x3_ok(M, hd, att)) T_TRY(digat_linear_bwd_input_x3(w.dpre, attp, A1, w.dh, hd, (int)M, att, hd, 1, w.a1t_img, st));
    else T_TRY(digat_linear_bwd_input(w.dpre, attp, A1, w.dh, hd, (int)M, att, hd, 1, st));
    return digat_linear_bwd_weight(w.dpre, attp, h, hd, dA1, db1, (int)M, att, hd, 0, wg, wgb, st);
}

// ---- the pair ------------------------------------------------------------------------------------------------------
struct MsaSave { float* Ed; uint8_t* dmask; float *qkv, *h, *pre, *alpha; };
static size_t msa_save_carve(Arena& a, int T, int Lw, int dm, int hd, int att, MsaSave* s) {
    const size_t M = (size_t)T * Lw;
    s->Ed = a.take<float>(M * dm); s->dmask = a.take<uint8_t>(M * dm); s->qkv = a.take<float>(M * 3 * hd); s->h = a.take<float>(M * hd);
    s->pre = a.take<float>(M * msa_attp(att)); s->alpha = a.take<float>(M);
    return a.used;
}
// One layout for both directions.  Forward: the split images of [W_Q; W_K; W_V] and A1 (the weights change every optimiser step).
// Backward: A1^T's image and the pooling regions, dqkv, the image of the stacked weights' transpose (dm rounded up to 80 rows), the
// weight-gradient scratch (the larger of the two products), and the stacked dW / db for callers whose three dW are not one buffer.
struct MsaTrainWs { void *qkv_img, *a1_img; PoolBwdWs pool; float* dqkv; void *wcat_img, *wg; size_t wgb; float *wg3, *db3g; };
static size_t msa_train_carve(Arena& w, int T, int Lw, int dm, int hd, int att, MsaTrainWs* o) {
    const size_t M = (size_t)T * Lw;
    o->qkv_img = w.take<char>(digat_split_weights_bytes(3 * hd, dm));
    o->a1_img = w.take<char>(digat_split_weights_bytes(att, hd));
    o->pool.a1t_img = w.take<char>(digat_split_weights_bytes(hd, att));
    o->pool.dh = w.take<float>(M * hd);
    o->pool.dpre = w.take<float>(M * msa_attp(att));
    o->dqkv = w.take<float>(M * 3 * hd);
    o->pool.da2p = w.take<float>((size_t)T * att);
    o->pool.da2g = w.take<float>((size_t)((T + 63) / 64) * att);
    o->wcat_img = w.take<char>(digat_split_weights_bytes((int)msa_attp(dm), 3 * hd));
    o->wgb = digat_linear_bwd_weight_workspace((int)M, 3 * hd, dm);
    const size_t wgb2 = digat_linear_bwd_weight_workspace((int)M, att, hd);
    if (wgb2 > o->wgb) o->wgb = wgb2;
    o->wg = w.take<char>(o->wgb);
    o->wg3 = w.take<float>(3 * (size_t)hd * dm);
    o->db3g = w.take<float>(3 * (size_t)hd);
    return w.used;
}
// ---- the projections' backward, shared by digat_msa_bwd and digat_mhsa_bwd (digat_mhsa.inc) --------------------------------------
// row_grad = (dQ W_Q + dK W_K + dV W_V) under the input dropout's keep bytes: w.dqkv [M, 3 hd] -> row_grad [M, dm], rows ld_row_grad apart
static int qkv_input_grad(const float* W_Q, const float* W_K, const float* W_V, const MsaTrainWs& w, const uint8_t* dmask, float p_drop,
                          float* row_grad, int64_t ld_row_grad, long M, int dm, int hd, hipStream_t st) {
    const int dmp = (int)msa_attp(dm);
    // projections: dEd = dQ W_Q + dK W_K + dV W_V; dW_* = d*^T Ed; db_Q, db_V = column sums
    if (M >= 2048 && (3 * hd) % 8 == 0 && ld_row_grad == dmp) {
        // one bf16x6 product over the stacked weights [W_Q; W_K; W_V] ([3 hd, dm], used as its transpose), split from their three
        // homes; the output's 80-column strips run over dm rounded up (zero weight rows): row_grad's rows are ld_row_grad = dmp
        // floats apart
        T_TRY(launch_split(W_Q, W_K, W_V, dm, 1, 3 * hd, w.wcat_img, st, 2));
        GemmArgs gx = gemm_plain(w.dqkv, 3 * hd, W_Q, nullptr, row_grad, ld_row_grad, (int)M, dm, 3 * hd, 0);
        gx.nseg = dmp; gx.wsplit = (const unsigned short*)w.wcat_img;
        if (g_train_bf16) gx.x1_segs = 7;
        if (!gemm_takes_row_list(gx)) return DIGAT_ERR_SHAPE;
        const bool mask_here = p_drop > 0.f && dm % 4 == 0;          // the embedding dropout's backward in this product's epilogue
        if (mask_here) { gx.dmask = dmask; gx.lddm = dm; gx.dscale = 1.f / (1.f - p_drop); gx.dmask_cols = dm; }
        T_TRY(launch_gemm(gx, st, DIGAT_KERNEL_LINEAR));
        if (mask_here) p_drop = 0.f;                                  // (the launch below is not needed)
    } else {
        T_TRY(digat_linear_bwd_input(w.dqkv, 3 * hd, W_Q, row_grad, ld_row_grad, (int)M, hd, dm, 0, st));
        T_TRY(digat_linear_bwd_input(w.dqkv + hd, 3 * hd, W_K, row_grad, ld_row_grad, (int)M, hd, dm, 1, st));
        T_TRY(digat_linear_bwd_input(w.dqkv + 2 * hd, 3 * hd, W_V, row_grad, ld_row_grad, (int)M, hd, dm, 1, st));
    }
    if (p_drop > 0.f) {
        MsaRowDropArgs a{row_grad, ld_row_grad, dmask, M, dm, 1.f / (1.f - p_drop)};
        hipLaunchKernelGGL(msa_row_dropout_bwd_kernel, dim3(grid_for(M * dm)), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}
// dW_Q, dW_K, dW_V [hd, dm] and db_Q, db_V [hd] from w.dqkv and the projections' input rows Xd [M, dm]
static int qkv_weight_grad(const MsaTrainWs& w, const float* Xd, float* dW_Q, float* db_Q, float* dW_K, float* dW_V, float* db_V, long M, int dm,
                           int hd, hipStream_t st) {
    const size_t wn = (size_t)hd * dm, hn = hd;
    {   // the three weight gradients as one product dQKV^T Ed ([3 hd, dm]); db_Q / db_V are the column sums of its outer blocks
        // a caller that hands over dW_Q, dW_K, dW_V as the three blocks of ONE [3 hd, dm] buffer (newsEncoders.MsaFused does) gets the
        // product written in place
        const bool stacked = dW_K == dW_Q + wn && dW_V == dW_Q + 2 * wn;
        T_TRY(digat_linear_bwd_weight(w.dqkv, 3 * hd, Xd, dm, stacked ? dW_Q : w.wg3, w.db3g, (int)M, 3 * hd, dm, 0, w.wg, w.wgb, st));
        if (!stacked && (hipMemcpyAsync(dW_Q, w.wg3, wn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                         hipMemcpyAsync(dW_K, w.wg3 + wn, wn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                         hipMemcpyAsync(dW_V, w.wg3 + 2 * wn, wn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)) return DIGAT_ERR_LAUNCH;
        if (hipMemcpyAsync(db_Q, w.db3g, hn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(db_V, w.db3g + 2 * hd, hn * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    }
    return DIGAT_OK;
}

static int msa_shape_ok(const digat_msa_params* p, int Lw) {
    const int dm = p->word_embedding_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    return dm > 0 && dm % 4 == 0 && heads > 0 && dk > 0 && dk <= MSA_MAX_DK && att > 0 && att % 4 == 0 && (heads * dk) % 4 == 0 && Lw <= 32;
}

// the leading dimension of row_grad that lets digat_msa_bwd compute it as one matrix-core product
int64_t digat_msa_row_grad_ld(int T, int Lw, int word_embedding_dim) {
    return (long)T * Lw >= 2048 ? (int64_t)msa_attp(word_embedding_dim) : word_embedding_dim;
}
size_t digat_msa_train_save_bytes(int T, int Lw, int dm, int heads, int dk, int att) {
    Arena measure;
    MsaSave s;
    return msa_save_carve(measure, T, Lw, dm, heads * dk, att, &s);
}
size_t digat_msa_train_workspace_bytes(int T, int Lw, int dm, int heads, int dk, int att) {
    Arena measure;
    MsaTrainWs o;
    return msa_train_carve(measure, T, Lw, dm, heads * dk, att, &o);
}

// out [T, heads*dk].  p_drop: dropout on the embedded tokens (newsEncoders.py:77); params' *_wsplit fields are not used (the
// weights change every optimiser step: they are split here, into the workspace).
int digat_msa_fwd_train(const digat_msa_params* p, const int32_t* title_text, const uint8_t* title_mask, float* out, float p_drop,
                        uint32_t seed, int T, int Lw, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (!p || !title_text || !title_mask || !out || !save || !workspace || T < 0 || Lw <= 0 || p_drop < 0.f || p_drop >= 1.f)
        return DIGAT_ERR_ARG;
    if (!msa_shape_ok(p, Lw)) return DIGAT_ERR_SHAPE;
    const int dm = p->word_embedding_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    const int hd = heads * dk;
    if (T == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    MsaSave s;
    MsaTrainWs o;
    msa_save_carve(sa, T, Lw, dm, hd, att, &s);
    msa_train_carve(w, T, Lw, dm, hd, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)T * Lw;
    // Ed = dropout(embedding[tokens])
    T_TRY(launch_gather_embedding(p->word_embedding, title_text, s.Ed, M, dm, st));
    if (p_drop > 0.f) T_TRY(digat_dropout_fwd(s.Ed, s.Ed, s.dmask, M * dm, p_drop, seed, stream));
    GemmArgs g = gemm_plain(s.Ed, dm, p->W_Q, p->b_Q, s.qkv, 3 * hd, (int)M, hd, dm, 0);
    g.w[1] = p->W_K; g.bias[1] = nullptr; g.y[1] = s.qkv + hd;
    g.w[2] = p->W_V; g.bias[2] = p->b_V; g.y[2] = s.qkv + 2 * hd;
    g.nsegs = 3;
    if (hd % 80 == 0 && dm >= 32 && M >= 2048) {
        T_TRY(launch_split(p->W_Q, p->W_K, p->W_V, hd, 3, dm, o.qkv_img, st));
        g.wsplit = (const unsigned short*)o.qkv_img;
        if (g_train_bf16) g.x1_segs = 7;
    }
    T_TRY(launch_gemm(g, st, DIGAT_KERNEL_LINEAR));
    T_TRY(launch_msa_attention(s.qkv, s.h, T, Lw, heads, dk, st));          // msa_shape_ok: Lw <= 32, the matrix-core kernel
    const void* a1_img = nullptr;
    if (M >= 2048 && hd >= 32) {
        T_TRY(launch_split(p->A1, p->A1, p->A1, att, 1, hd, o.a1_img, st));
        a1_img = o.a1_img;
    }
    // bf16_ok = true: as the projections above, affine1 follows digat_set_train_precision (digat_cnn_fwd_train's does not)
    return news_pool_fwd(s.h, hd, p->A1, a1_img, p->b1, p->a2, s.pre, title_mask, out, s.alpha, T, Lw, att, true, st);
}

// dout [T, heads*dk].  Written (not accumulated): row_grad [T*Lw, dm] with rows ld_row_grad floats apart — dm, or dm rounded up
// to a multiple of 80 (digat_msa_row_grad_ld: then one bf16x6 product computes it) — the gradient at the embedded tokens, after
// the dropout's backward: feed it to digat_embedding_bwd; dW_Q dW_K dW_V [hd, dm], db_Q db_V [hd], dA1 [att, hd], db1 da2 [att].
int digat_msa_bwd(const digat_msa_params* p, const int32_t* title_text, const uint8_t* title_mask, const float* dout, float p_drop,
                  const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW_Q, float* db_Q, float* dW_K,
                  float* dW_V, float* db_V, float* dA1, float* db1, float* da2, int T, int Lw, void* workspace, size_t workspace_bytes,
                  void* stream) {
    if (!p || !title_text || !title_mask || !dout || !save || !row_grad || !dW_Q || !db_Q || !dW_K || !dW_V || !db_V || !dA1 || !db1 ||
        !da2 || !workspace || T < 0 || Lw <= 0) return DIGAT_ERR_ARG;
    if (!msa_shape_ok(p, Lw)) return DIGAT_ERR_SHAPE;
    const int dm = p->word_embedding_dim, heads = p->head_num, dk = p->head_dim, att = p->attention_dim;
    const int hd = heads * dk, dmp = (int)msa_attp(dm);
    if (ld_row_grad != dm && ld_row_grad != dmp) return DIGAT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t wn = (size_t)hd * dm, hn = hd, an = att;          // floats of one projection's weight, of a bias, of an attention vector
    if (T == 0) return zero_floats(st, {{dW_Q, wn}, {dW_K, wn}, {dW_V, wn}, {db_Q, hn}, {db_V, hn}, {dA1, an * hn}, {db1, an}, {da2, an}});
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    MsaSave s;
    MsaTrainWs o;
    msa_save_carve(sa, T, Lw, dm, hd, att, &s);
    msa_train_carve(w, T, Lw, dm, hd, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    const long M = (long)T * Lw;
    T_TRY(news_pool_bwd(dout, s.h, hd, s.pre, s.alpha, title_mask, p->A1, p->b1, p->a2, o.pool, o.wg, o.wgb, dA1, db1, da2, T, Lw, att, st));
    // ReLU + attention
    {
        MsaAttnBwdArgs a{s.qkv, s.h, o.pool.dh, o.dqkv, T, Lw, heads, dk};
        const size_t lds = (size_t)2 * 5 * MSA_BWD_IMG * 4;
        hipLaunchKernelGGL(msa_attention_bwd_kernel, dim3(T), dim3(128), lds, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    T_TRY(qkv_input_grad(p->W_Q, p->W_K, p->W_V, o, s.dmask, p_drop, row_grad, ld_row_grad, M, dm, hd, st));
    return qkv_weight_grad(o, s.Ed, dW_Q, db_Q, dW_K, dW_V, db_V, M, dm, hd, st);
}

}  // extern "C"
