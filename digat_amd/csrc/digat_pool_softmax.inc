// digat_pool_softmax.inc — retrieval training: the softmax loss of given targets over a user's whole pool and its gradients, without
// the [G, P] score matrix, its softmax or its gradient ever reaching memory (evaluate.pool_softmax, nrms.retrieval_step).  Included in
// digat_kernels.hip behind digat_dot_rank.inc, whose product, elements and target plumbing these are: DotArgs / DotShared, dot_tile
// (every score the same bits wherever it is computed), dot_skipped, rank_tile_starts, rank_user, rank_hash and dot_rank_target_kernel.
// An element of user g is a pool position whose id lies in [0, N) and is not in skip[g].  x(g, p) = fl(scale * score(g, p)).
//   lse[g]  = log sum over g's elements of exp(x(g, p))                 (-inf when g has no element)
//   loss[t] = lse[g(t)] - x(g(t), pos[t])   when pos[t] is an element of g(t);   0, with out_target_score[t] = NaN, otherwise
// Backward, given grad_loss [T] (ignored where the target is no element): c[g] = the sum of grad_loss over g's ranked targets, and
//   C(g, p) = c[g] exp(x(g, p) - lse[g]) - sum over g's ranked targets at p of grad_loss        on elements, 0 elsewhere (never stored)
//   d_users[g, :] = scale sum_p C(g, p) news[id(p), :]            d_rows[p, :] = scale sum_g C(g, p) users[g, :]     (per POOL POSITION)
//
// Forward, four launches sized by what the host knows (target_start is never read on the host):
//   psm_init_kernel         one thread per target: loss 0, score NaN, rank flag -1, key 0: every output byte is written whatever
//                           target_start holds.
//   dot_rank_target_kernel  (digat_dot_rank.inc, shared) one workgroup per tile of 64 users: the targets' own scores through dot_tile,
//                           flag 0 where the target is an element.
//   psm_chunk_kernel<SKIP>  one workgroup per (tile of 64 users, chunk of DIGAT_DOT_TOPK_CHUNK positions), dot_chunk_kernel's grid.  Per
//                           sub-tile dot_tile, then wave w owns users 16 w .. + 16, one position per lane.  The skip row is consulted
//                           only where a per-user Bloom filter of the row hits (dot_rank_count_kernel's).  Every lane keeps, per user,
//                           a running reference r — the largest ceil(y) so far, y = fl(x log2 e) — and a Kahan-compensated sum of
//                           2^(y - r): a new reference rescales the sum by a power of two, exactly; the maximum is always subtracted.
//                           At the end of the chunk the wave's largest r, the lanes' sums scaled to it (exactly) and a butterfly sum
//                           (lane l + lane l ^ 32, ^ 16, .. ^ 1) give (r, s) -> workspace [G][chunks].
//   psm_finish_kernel       one workgroup per tile, a wave per user: lane l combines chunks l, l + 64, .. in that order (references by
//                           exact power-of-two scaling), then the same butterfly; lse = r ln 2 + log s and, for the user's targets,
//                           loss = lse - fl(scale * score), both in fp64 and rounded once.
// Backward, six launches: psm_init_kernel and dot_rank_target_kernel again (which targets are elements), then
//   psm_prep_kernel         one workgroup per tile: c[g], a thread per user adding grad_loss in ascending t; per target a record — its
//                           position when it is the FIRST ranked target of its user there (with a flag when later ones share it), -1
//                           otherwise; per tile whether anything in it is non-zero (a tile where nothing is is never multiplied).
//   psm_users_kernel<NB>    one workgroup per (tile, group of chunks): at most ceil(256 / tiles) groups per tile, so the partial sums
//                           stay bounded whatever G is.  Per sub-tile dot_tile, Ss overwritten by C — c exp2((x - lse) log2 e) on
//                           elements of users with c != 0, exactly 0 elsewhere (a user with c == 0 never meets its lse); then every
//                           first-record target of the sub-tile subtracts its grad_loss and, flagged, those of the later targets at
//                           its position in ascending t: one writer per (user, position) — and the second product C x news rows on
//                           v_mfma_f32_16x16x4_f32, A from Ss, B straight from the rows, accumulated over the group's sub-tiles in
//                           position order into a 64 x d block of registers (NB column blocks of 16 per wave: d <= 64 NB, NB in 1, 2,
//                           4, 8, hence d <= 512) -> workspace [tile][group][64][d].
//   psm_users_reduce_kernel one thread per element of d_users: the groups' partial sums added in group order, times scale.
//   psm_rows_kernel<NB>     one workgroup per 64 positions, walking the user tiles in order: the same tile and C, the second product
//                           C^T x user rows, accumulated in registers over all tiles; d_rows = scale times that.
// No floating-point atomics: every sum's order is fixed by G, P, d and the targets alone, so two calls give the same bits, and a
// user's lse and loss do not depend on who else is in the call.
//
// Error of lse and loss against an exact evaluation on the same fp32 scores (u = 2^-24, n elements, S = sub-tiles of a chunk <= 32,
// C = chunks): x carries one rounding, u |x|, which moves lse by at most u max|x|; so does y = fl(x log2 e).  A term 2^(y - r): the
// subtraction rounds by u |y - r| and v_exp_f32 by 1 ulp = 2 u; weighted by the terms, the mean of |y - r| ln 2 is the entropy of the
// softmax minus log s <= log n.  The sum: Kahan per lane (2 u + O(S u^2)), 6 butterfly levels, ceil(C / 64) - 1 + 6 additions in the
// finish kernel, all rescalings exact: relative error of s <= (2 + 2 + log n + 6 + ceil(C / 64) + 5) u.  r ln 2 + log s is taken in
// fp64 and rounded once (u |lse|; the bound below keeps 4 u |lse|).  Altogether
//   |lse - exact|  <= u (15 + ceil(C / 64) + log n + 4 |lse| + 2 max|x|)
//   |loss - exact| <= that + u (|x_target| + |loss|)
// At P = 65 237, |x| <= 30: 28 u + 6 u |lse| <= 1.7e-6 + 3.6e-7 |lse| — inside the project's output tolerance (atol 2e-6, rtol 1e-5).
// evaluate.pool_softmax_bound is this formula; tests/test_hip_pool_softmax.py holds the kernels to it.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   psm_init_kernel            VGPRs 7             SGPRs 16    LDS 0 B       scratch 0   occupancy 8 waves / SIMD
//   psm_chunk_kernel<false>    VGPRs 116 + 16 acc  SGPRs 103   LDS 43008 B   scratch 0   occupancy 3 waves / SIMD (by LDS)
//   psm_chunk_kernel<true>     VGPRs 153 + 16 acc  SGPRs 106   LDS 59392 B   scratch 0   occupancy 2 waves / SIMD (by LDS: the Bloom filters)
//   psm_finish_kernel          VGPRs 66            SGPRs 40    LDS 520 B     scratch 0   occupancy 7 waves / SIMD
//   psm_prep_kernel            VGPRs 28            SGPRs 56    LDS 784 B     scratch 0   occupancy 8 waves / SIMD
//   psm_users_kernel<1|2|4|8>  VGPRs 99 | 85 | 89 | 152  + 32 | 44 | 76 | 140 acc   SGPRs 106   LDS 60936 B   scratch 0   occupancy 2 | 2 | 2 | 1
//   psm_users_reduce_kernel    VGPRs 13            SGPRs 25    LDS 0 B       scratch 0   occupancy 8 waves / SIMD
//   psm_rows_kernel<1|2|4|8>   VGPRs 103 | 89 | 89 | 141 + 32 | 44 | 76 | 140 acc   SGPRs 106   LDS 60936 B   scratch 0   occupancy 2 | 2 | 2 | 1
//   (<8>, d in (256, 512]: 128 accumulator registers of the second product + 16 of dot_tile leave one workgroup per CU — by registers,
//   292 of the 512 a lane may have; <1> .. <4> are held at two by their 60 KB of LDS.)
//
// Measured on an MI355X at G = 4 096, P = 65 237, d = 400, 50-entry skip rows: forward 3.7 ms at one target per user and 3.8 ms at five
// (torch.matmul + masked logsumexp per 1 024 users: 3.8 ms), forward + backward 27.8 / 28.1 ms (stock autograd: 12.1 ms) at a peak of
// 106 MiB of device memory beyond the inputs, gradients included, where the stock composition holds 2 803 MiB; at G = 64 — one tile —
// 0.9 ms and 2.6 ms against 0.15 and 0.66 ms (DESIGN section 8).

#define PSM_MAX_D 512                    // the backward's 64 x d block of accumulators: 8 column blocks of 16 per wave
#define PSM_LOG2E 1.44269504088896341f
#define PSM_DUP (1ll << 62)              // record flag: later ranked targets of the user share this position

struct PsmArgs {
    RankArgs r;                          // dot (users .. chunks), target_pos, target_start, T; out_rank = flag [T] (0: an element, -1: none),
                                         // out_scores = the targets' score bits [T], key [T] (dot_rank_target_kernel's, not read here)
    float scale;
    float* loss;                         // [T]   forward out
    float* lse;                          // [G]   forward out, backward in
    float2* part;                        // workspace [G][chunks]: (reference, sum of 2^(y - reference))
    const float* grad_loss;              // [T]
    float* c;                            // workspace [G]
    long long* rec;                      // workspace [T]
    int* live;                           // workspace [tiles]
    float* partial;                      // workspace [tiles][groups][64][d]
    float* d_users;                      // [G, d]
    float* d_rows;                       // [P, d]
    long groups, per_group;              // chunk groups per tile, chunks per group
};

struct PsmShared {                       // the backward's, next to DotShared
    long ts[DOT_USERS + 1];
    float c[DOT_USERS], lse[DOT_USERS];
    const float* row[DOT_USERS];         // the second product's B rows: news rows of the sub-tile's positions, or the tile's user rows
    unsigned bloom[DOT_USERS][RANK_BLOOM_WORDS];
};

// (int)(a - b) for references a <= b, held at -256 (2^-256 of anything here is 0; -inf - -inf = NaN lands there too)
__device__ __forceinline__ int psm_shift(float a, float b) { return (int)fmaxf(a - b, -256.f); }

// The tile's Bloom filters of the skip rows (dot_rank_count_kernel's).  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ void psm_bloom(const DotArgs& a, unsigned (*bloom)[RANK_BLOOM_WORDS], long u0) {
    const int tid = threadIdx.x;
    for (int x = tid; x < DOT_USERS * RANK_BLOOM_WORDS; x += 256) bloom[x / RANK_BLOOM_WORDS][x % RANK_BLOOM_WORDS] = 0u;
    __syncthreads();
    for (int x = tid; x < DOT_USERS * a.skip_len; x += 256) {
        const int u = x / a.skip_len;
        if (u0 + u < a.G) {
            const long long id = (long long)a.skip[(u0 + u) * a.skip_len + (x - u * a.skip_len)];
            const unsigned ha = rank_hash(id, RANK_HASH_A), hb = rank_hash(id, RANK_HASH_B);
            atomicOr(&bloom[u][ha >> 5], 1u << (ha & 31));
            atomicOr(&bloom[u][hb >> 5], 1u << (hb & 31));
        }
    }
    __syncthreads();
}

// One wave, user u of the tile (u0 + u < G), one position per lane: is the lane's position an element of the user?
__device__ __forceinline__ bool psm_element(const DotArgs& a, const unsigned (*bloom)[RANK_BLOOM_WORDS], int u, long u0, long long id,
                                            unsigned ha, unsigned hb, int lane) {
    bool elem = id >= 0;
    const bool maybe = elem && ((bloom[u][ha >> 5] >> (ha & 31)) & (bloom[u][hb >> 5] >> (hb & 31)) & 1u);
    const unsigned long long pass = __ballot(maybe);
    if (pass) {
        const unsigned long long out = dot_skipped(a.skip + (u0 + u) * a.skip_len, a.skip_len, id, pass, lane);
        if ((out >> lane) & 1ull) elem = false;
    }
    return elem;
}

// The sub-tile's pool ids into s.id (-1: beyond pend or outside [0, N)).  No barrier.
__device__ __forceinline__ void psm_ids(const DotArgs& a, DotShared& s, long q0, long pend) {
    const int tid = threadIdx.x;
    if (tid < DOT_SUB) {
        const long p = q0 + tid;
        long long id = -1;
        if (p < pend) {
            id = a.pool ? (long long)a.pool[p] : (long long)p;
            if (id < 0 || id >= a.N) id = -1;
        }
        s.id[tid] = id;
    }
}

__device__ __forceinline__ float psm_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ float psm_wave_sum(float v) {         // every lane ends with the same bits: a + b == b + a
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256) psm_init_kernel(const PsmArgs q) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < q.r.T) {
        q.r.out_rank[t] = -1;
        q.r.out_scores[t] = __uint_as_float(0x7fc00000u);
        q.r.key[t] = 0u;
        if (q.loss) q.loss[t] = 0.f;
    }
}

template <bool SKIP>
__global__ void __launch_bounds__(256) psm_chunk_kernel(const PsmArgs q) {
    __shared__ DotShared s;
    __shared__ unsigned bloom[SKIP ? DOT_USERS : 1][RANK_BLOOM_WORDS];
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long tile = blockIdx.x % a.tiles, chunk = blockIdx.x / a.tiles;
    const long u0 = tile * DOT_USERS, p0 = chunk * DIGAT_DOT_TOPK_CHUNK;
    const long pend = p0 + DIGAT_DOT_TOPK_CHUNK < a.P ? p0 + DIGAT_DOT_TOPK_CHUNK : a.P;
    if (SKIP) psm_bloom(a, bloom, u0);
    float ref[DOT_USERS / 4], sum[DOT_USERS / 4], comp[DOT_USERS / 4];
#pragma unroll
    for (int i = 0; i < DOT_USERS / 4; ++i) { ref[i] = -INFINITY; sum[i] = 0.f; comp[i] = 0.f; }
    for (long q0 = p0; q0 < pend; q0 += DOT_SUB) {
        psm_ids(a, s, q0, pend);
        __syncthreads();
        dot_tile(a, s, u0);
        const long long id = s.id[lane];
        const unsigned ha = rank_hash(id, RANK_HASH_A), hb = rank_hash(id, RANK_HASH_B);
#pragma unroll
        for (int i = 0; i < DOT_USERS / 4; ++i) {
            const int u = wave * (DOT_USERS / 4) + i;
            if (u0 + u >= a.G) continue;                          // wave-uniform
            const bool elem = SKIP ? psm_element(a, bloom, u, u0, id, ha, hb, lane) : id >= 0;
            const float y = (q.scale * s.Ss[u][lane]) * PSM_LOG2E;
            if (elem && y != -INFINITY) {                         // exp(-inf) adds nothing; a NaN goes through and shows
                const float rn = fmaxf(ref[i], ceilf(y));
                const int sh = psm_shift(ref[i], rn);
                const float e = __builtin_amdgcn_exp2f(y - rn) - ldexpf(comp[i], sh);
                const float so = ldexpf(sum[i], sh), sn = so + e;
                comp[i] = (sn - so) - e;
                sum[i] = sn;
                ref[i] = rn;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < DOT_USERS / 4; ++i) {
        const long g = u0 + wave * (DOT_USERS / 4) + i;
        if (g >= a.G) continue;
        const float R = psm_wave_max(ref[i]);
        const float v = psm_wave_sum(ldexpf(sum[i] - comp[i], psm_shift(ref[i], R)));
        if (lane == 0) q.part[g * a.chunks + chunk] = make_float2(R, v);
    }
}

__global__ void __launch_bounds__(256) psm_finish_kernel(const PsmArgs q) {
    __shared__ long ts[DOT_USERS + 1];
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long u0 = (long)blockIdx.x * DOT_USERS;
    rank_tile_starts(q.r, ts, u0);
    for (int i = 0; i < DOT_USERS / 4; ++i) {
        const int u = wave * (DOT_USERS / 4) + i;
        const long g = u0 + u;
        if (g >= a.G) continue;
        float ref = -INFINITY, sum = 0.f;
        for (long c = lane; c < a.chunks; c += 64) {
            const float2 p = q.part[g * a.chunks + c];
            const float rn = fmaxf(ref, p.x);
            sum = ldexpf(sum, psm_shift(ref, rn)) + ldexpf(p.y, psm_shift(p.x, rn));
            ref = rn;
        }
        const float R = psm_wave_max(ref);
        const float S = psm_wave_sum(ldexpf(sum, psm_shift(ref, R)));
        // one logarithm and one sum per user, in fp64 and rounded once: the backward's exp(x - lse) shares lse's error over the whole
        // row, so it is kept to half an ulp.  No element: -inf + -inf.
        const double l = (double)R * 0.69314718055994530942 + log((double)S);
        const float lse = (float)l;
        if (lane == 0) q.lse[g] = lse;
        for (long t = ts[u] + lane; t < ts[u + 1]; t += 64)
            q.loss[t] = q.r.out_rank[t] == 0 ? (float)(l - (double)(q.scale * q.r.out_scores[t])) : 0.f;
    }
}

__global__ void __launch_bounds__(256) psm_prep_kernel(const PsmArgs q) {
    __shared__ long ts[DOT_USERS + 1];
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x;
    const long u0 = (long)blockIdx.x * DOT_USERS;
    rank_tile_starts(q.r, ts, u0);
    const long tb = ts[0], te = ts[DOT_USERS];
    for (long t = tb + tid; t < te; t += 256) {
        long long rec = -1;
        if (q.r.out_rank[t] == 0) {
            const int u = rank_user(ts, t);
            const long pos = q.r.target_pos[t];                   // an element: inside [0, P)
            bool first = true, dup = false;
            for (long t2 = ts[u]; t2 < t && first; ++t2) first = !(q.r.out_rank[t2] == 0 && q.r.target_pos[t2] == pos);
            if (first) {
                for (long t2 = t + 1; t2 < ts[u + 1] && !dup; ++t2) dup = q.r.out_rank[t2] == 0 && q.r.target_pos[t2] == pos;
                rec = (long long)pos | (dup ? PSM_DUP : 0ll);
            }
        }
        q.rec[t] = rec;
    }
    bool some = false;
    if (tid < DOT_USERS && u0 + tid < a.G) {
        float c = 0.f;
        for (long t = ts[tid]; t < ts[tid + 1]; ++t)
            if (q.r.out_rank[t] == 0) {
                const float gl = q.grad_loss[t];
                c += gl;
                some = some || gl != 0.f;
            }
        q.c[u0 + tid] = c;
        some = some || c != 0.f;
    }
    const int live = __syncthreads_or(some ? 1 : 0);
    if (tid == 0) q.live[blockIdx.x] = live;
}

// The tile's targets, c and lse into LDS.  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ void psm_tile_users(const PsmArgs& q, PsmShared& h, long u0) {
    const int tid = threadIdx.x;
    rank_tile_starts(q.r, h.ts, u0);
    if (tid < DOT_USERS) {
        const long g = u0 + tid;
        const bool in = g < q.r.dot.G;
        h.c[tid] = in ? q.c[g] : 0.f;
        h.lse[tid] = in ? q.lse[g] : 0.f;
    }
    __syncthreads();
}

// Ss[u][j] = the score of (user u0 + u, position q0 + j) on entry, C(u, j) on return.  Whole workgroup; ends behind a barrier.
__device__ __forceinline__ void psm_coefficients(const PsmArgs& q, DotShared& s, PsmShared& h, long u0, long q0) {
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long id = s.id[lane];
    const unsigned ha = rank_hash(id, RANK_HASH_A), hb = rank_hash(id, RANK_HASH_B);
#pragma unroll 4
    for (int i = 0; i < DOT_USERS / 4; ++i) {
        const int u = wave * (DOT_USERS / 4) + i;
        const float cg = h.c[u];                                  // wave-uniform; 0 beyond G
        float v = 0.f;
        if (cg != 0.f) {
            const bool elem = a.skip ? psm_element(a, h.bloom, u, u0, id, ha, hb, lane) : id >= 0;
            if (elem) v = cg * __builtin_amdgcn_exp2f((q.scale * s.Ss[u][lane] - h.lse[u]) * PSM_LOG2E);
        }
        s.Ss[u][lane] = v;
    }
    __syncthreads();
    const long tb = h.ts[0], te = h.ts[DOT_USERS];
    for (long t = tb + tid; t < te; t += 256) {
        const long long rec = q.rec[t];
        if (rec < 0) continue;
        const long pos = (long)(rec & ~PSM_DUP);
        if (pos < q0 || pos >= q0 + DOT_SUB) continue;
        const int u = rank_user(h.ts, t);
        float v = s.Ss[u][pos - q0] - q.grad_loss[t];             // the only writer of this (user, position)
        if (rec & PSM_DUP)
            for (long t2 = t + 1; t2 < h.ts[u + 1]; ++t2)
                if (q.r.out_rank[t2] == 0 && q.r.target_pos[t2] == pos) v -= q.grad_loss[t2];
        s.Ss[u][pos - q0] = v;
    }
    __syncthreads();
}

// acc += A x B over the sub-tile's 64 k: A[m][k] = Ss[m][k] (TRANSPOSED: Ss[k][m]), B[k][:] = h.row[k][0 .. d) (nullptr: zeros).
// Wave w owns the column blocks w, w + 4, ..; acc[j][tm] is the 16 x 16 tile of rows 16 tm .., columns 16 (w + 4 j) ..
template <int NB, bool TRANSPOSED>
__device__ __forceinline__ void psm_accumulate(v4f (&acc)[NB][4], const DotShared& s, const PsmShared& h, int d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
#pragma unroll 2
    for (int ks = 0; ks < DOT_SUB / 4; ++ks) {
        const int k = 4 * ks + lq;
        const float* row = h.row[k];
        float am[4];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) am[tm] = TRANSPOSED ? s.Ss[k][16 * tm + lr] : s.Ss[16 * tm + lr][k];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int c0 = 16 * (wave + 4 * j);
            if (c0 < d) {                                         // wave-uniform
                const float b = row && c0 + lr < d ? row[c0 + lr] : 0.f;
#pragma unroll
                for (int tm = 0; tm < 4; ++tm) acc[j][tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(am[tm], b, acc[j][tm], 0, 0, 0);
            }
        }
    }
}

// D[row 16 tm + 4 lq + r][column 16 (w + 4 j) + lr] -> out[row][column] * mul for rows < rows
template <int NB>
__device__ __forceinline__ void psm_store(const v4f (&acc)[NB][4], float* out, long rows, int d, float mul) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int col = 16 * (wave + 4 * j) + lr;
        if (col >= d) continue;
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = 16 * tm + 4 * lq + r;
                if (row < rows) out[row * d + col] = acc[j][tm][r] * mul;
            }
    }
}

template <int NB>
__global__ void __launch_bounds__(256) psm_users_kernel(const PsmArgs q) {
    __shared__ DotShared s;
    __shared__ PsmShared h;
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x;
    const long tile = blockIdx.x % a.tiles, grp = blockIdx.x / a.tiles;
    const long u0 = tile * DOT_USERS;
    v4f acc[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) acc[j][tm] = (v4f){0.f, 0.f, 0.f, 0.f};
    if (q.live[tile]) {                                           // workgroup-uniform
        psm_tile_users(q, h, u0);
        if (a.skip) psm_bloom(a, h.bloom, u0);
        const long c1 = (grp + 1) * q.per_group < a.chunks ? (grp + 1) * q.per_group : a.chunks;
        const long p1 = c1 * DIGAT_DOT_TOPK_CHUNK < a.P ? c1 * DIGAT_DOT_TOPK_CHUNK : a.P;
        for (long q0 = grp * q.per_group * DIGAT_DOT_TOPK_CHUNK; q0 < p1; q0 += DOT_SUB) {
            psm_ids(a, s, q0, p1);
            __syncthreads();
            if (tid < DOT_SUB) h.row[tid] = s.id[tid] >= 0 ? a.news + s.id[tid] * a.d : nullptr;
            dot_tile(a, s, u0);
            psm_coefficients(q, s, h, u0, q0);
            psm_accumulate<NB, false>(acc, s, h, a.d);
            __syncthreads();
        }
    }
    psm_store<NB>(acc, q.partial + (tile * q.groups + grp) * DOT_USERS * a.d, DOT_USERS, a.d, 1.f);
}

__global__ void __launch_bounds__(256) psm_users_reduce_kernel(const PsmArgs q) {
    const DotArgs& a = q.r.dot;
    const long x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= a.G * a.d) return;
    const long g = x / a.d, ch = x - g * a.d, tile = g / DOT_USERS, row = g - tile * DOT_USERS;
    float v = 0.f;
    for (long grp = 0; grp < q.groups; ++grp) v += q.partial[((tile * q.groups + grp) * DOT_USERS + row) * a.d + ch];
    q.d_users[x] = q.scale * v;
}

template <int NB>
__global__ void __launch_bounds__(256) psm_rows_kernel(const PsmArgs q) {
    __shared__ DotShared s;
    __shared__ PsmShared h;
    const DotArgs& a = q.r.dot;
    const int tid = threadIdx.x;
    const long q0 = (long)blockIdx.x * DOT_SUB;
    const long pend = q0 + DOT_SUB < a.P ? q0 + DOT_SUB : a.P;
    v4f acc[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) acc[j][tm] = (v4f){0.f, 0.f, 0.f, 0.f};
    psm_ids(a, s, q0, pend);
    __syncthreads();
    for (long tile = 0; tile < a.tiles; ++tile) {
        if (!q.live[tile]) continue;                              // workgroup-uniform
        const long u0 = tile * DOT_USERS;
        psm_tile_users(q, h, u0);
        if (a.skip) psm_bloom(a, h.bloom, u0);
        if (tid < DOT_USERS) h.row[tid] = u0 + tid < a.G ? a.users + (u0 + tid) * a.d : nullptr;
        dot_tile(a, s, u0);
        psm_coefficients(q, s, h, u0, q0);
        psm_accumulate<NB, true>(acc, s, h, a.d);
        __syncthreads();
    }
    psm_store<NB>(acc, q.d_rows + q0 * a.d, pend - q0, a.d, q.scale);
}

// One carve for both entries: the flags, keys, records and (backward) scores of the targets, the forward's (reference, sum) pairs, c,
// the tiles' live flags and the backward's partial blocks — min(tiles chunks, 256 + tiles) of them, 64 x d floats each.
struct PsmCarve {
    size_t rank, key, score, rec, part, c, live, partial, total;
};

static long psm_groups(long tiles, long chunks) {
    const long most = (256 + tiles - 1) / (tiles > 0 ? tiles : 1);
    return chunks < most ? (chunks > 0 ? chunks : 1) : most;
}

static PsmCarve psm_carve(int64_t G, int64_t P, int64_t T, int d) {
    PsmCarve c;
    const size_t tiles = (size_t)dot_tiles((long)G), chunks = (size_t)dot_chunks((long)P);
    const size_t blocks = tiles * chunks < 256 + tiles ? tiles * chunks : 256 + tiles;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t was = at; at += align_up(bytes, 256); return was; };
    c.rank = take((size_t)T * 4);
    c.key = take((size_t)T * 4);
    c.score = take((size_t)T * 4);
    c.rec = take((size_t)T * 8);
    c.part = take((size_t)G * chunks * 8);
    c.c = take((size_t)G * 4);
    c.live = take(tiles * 4);
    c.partial = take(blocks * DOT_USERS * (size_t)(d > 0 ? d : 0) * 4);
    c.total = at;
    return c;
}

static int psm_check(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t*& skip,
                     int& skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, const void* workspace,
                     size_t workspace_bytes) {
    if (!target_pos || !target_start || T < 0) return DIGAT_ERR_ARG;
    const size_t need = digat_pool_softmax_workspace_bytes(G, P, T, d);
    const int rc = topk_check_args(1, skip, skip_len, dot_check(users, news, pool, G, N, P, d), need > 0, workspace);
    if (rc != DIGAT_OK) return rc;
    if (T > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < need) return DIGAT_ERR_WORKSPACE;
    return DIGAT_OK;
}

static PsmArgs psm_args(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t* skip,
                        int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, float scale, float* scores,
                        void* workspace) {
    const PsmCarve c = psm_carve(G, P, T, d);
    char* w = (char*)workspace;
    PsmArgs q{};
    q.r = RankArgs{{users, news, pool, (long)G, (long)N, (long)P, d, skip, skip_len, 0, dot_tiles((long)G), dot_chunks((long)P), nullptr,
                    nullptr, nullptr, nullptr, nullptr},
                   target_pos, target_start, (long)T, (int32_t*)(w + c.rank), scores ? scores : (float*)(w + c.score), (unsigned*)(w + c.key)};
    q.scale = scale;
    q.part = (float2*)(w + c.part);
    q.c = (float*)(w + c.c);
    q.rec = (long long*)(w + c.rec);
    q.live = (int*)(w + c.live);
    q.partial = (float*)(w + c.partial);
    q.groups = psm_groups(q.r.dot.tiles, q.r.dot.chunks);
    q.per_group = (q.r.dot.chunks + q.groups - 1) / q.groups;
    return q;
}

extern "C" {

size_t digat_pool_softmax_workspace_bytes(int64_t users, int64_t pool, int64_t targets, int d) {
    if (users < 0 || pool < 0 || targets < 0 || d <= 0) return 0;
    return psm_carve(users, pool, targets, d).total;
}

int digat_pool_softmax_fwd(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                           const int64_t* skip, int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, float scale,
                           float* out_loss, float* out_lse, float* out_target_score, void* workspace, size_t workspace_bytes, void* stream) {
    if (!out_loss || !out_lse || !out_target_score) return DIGAT_ERR_ARG;
    const int rc = psm_check(users, news, pool, G, N, P, d, skip, skip_len, target_pos, target_start, T, workspace, workspace_bytes);
    if (rc != DIGAT_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    PsmArgs q = psm_args(users, news, pool, G, N, P, d, skip, skip_len, target_pos, target_start, T, scale, out_target_score, workspace);
    q.loss = out_loss;
    q.lse = out_lse;
    if (T > 0) {
        hipLaunchKernelGGL(psm_init_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, q);
        DIGAT_CHECK_LAUNCH();
    }
    if (G == 0) return DIGAT_OK;                                  // nobody owns a target
    const dim3 tiles((unsigned)q.r.dot.tiles);
    if (T > 0) {
        hipLaunchKernelGGL(dot_rank_target_kernel, tiles, dim3(256), 0, st, q.r);
        DIGAT_CHECK_LAUNCH();
    }
    if (P > 0) {
        const dim3 grid((unsigned)(q.r.dot.tiles * q.r.dot.chunks));
        if (skip) hipLaunchKernelGGL(psm_chunk_kernel<true>, grid, dim3(256), 0, st, q);
        else hipLaunchKernelGGL(psm_chunk_kernel<false>, grid, dim3(256), 0, st, q);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(psm_finish_kernel, tiles, dim3(256), 0, st, q);      // P == 0: no chunk, every lse -inf
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_pool_softmax_bwd(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                           const int64_t* skip, int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, float scale,
                           const float* lse, const float* grad_loss, float* d_users, float* d_rows, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (!lse || !grad_loss || !d_users || !d_rows) return DIGAT_ERR_ARG;
    const int rc = psm_check(users, news, pool, G, N, P, d, skip, skip_len, target_pos, target_start, T, workspace, workspace_bytes);
    if (rc != DIGAT_OK) return rc;
    if (d > PSM_MAX_D || (double)G * (double)d > 549755813632.0 || (P + DOT_SUB - 1) / DOT_SUB > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (G == 0 || P == 0 || T == 0) {                             // no coefficient is non-zero
        if (G > 0 && hipMemsetAsync(d_users, 0, (size_t)G * d * 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
        if (P > 0 && hipMemsetAsync(d_rows, 0, (size_t)P * d * 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
        return DIGAT_OK;
    }
    PsmArgs q = psm_args(users, news, pool, G, N, P, d, skip, skip_len, target_pos, target_start, T, scale, nullptr, workspace);
    q.lse = const_cast<float*>(lse);
    q.grad_loss = grad_loss;
    q.d_users = d_users;
    q.d_rows = d_rows;
    const dim3 tiles((unsigned)q.r.dot.tiles), block(256);
    hipLaunchKernelGGL(psm_init_kernel, dim3((unsigned)((T + 255) / 256)), block, 0, st, q);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(dot_rank_target_kernel, tiles, block, 0, st, q.r);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(psm_prep_kernel, tiles, block, 0, st, q);
    DIGAT_CHECK_LAUNCH();
    const dim3 ugrid((unsigned)(q.r.dot.tiles * q.groups)), rgrid((unsigned)((P + DOT_SUB - 1) / DOT_SUB));
    const int nb = (d + 63) / 64;                                 // column blocks of 16 per wave
    if (nb <= 1) hipLaunchKernelGGL(psm_users_kernel<1>, ugrid, block, 0, st, q);
    else if (nb <= 2) hipLaunchKernelGGL(psm_users_kernel<2>, ugrid, block, 0, st, q);
    else if (nb <= 4) hipLaunchKernelGGL(psm_users_kernel<4>, ugrid, block, 0, st, q);
    else hipLaunchKernelGGL(psm_users_kernel<8>, ugrid, block, 0, st, q);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(psm_users_reduce_kernel, dim3((unsigned)(((size_t)G * d + 255) / 256)), block, 0, st, q);
    DIGAT_CHECK_LAUNCH();
    if (nb <= 1) hipLaunchKernelGGL(psm_rows_kernel<1>, rgrid, block, 0, st, q);
    else if (nb <= 2) hipLaunchKernelGGL(psm_rows_kernel<2>, rgrid, block, 0, st, q);
    else if (nb <= 4) hipLaunchKernelGGL(psm_rows_kernel<4>, rgrid, block, 0, st, q);
    else hipLaunchKernelGGL(psm_rows_kernel<8>, rgrid, block, 0, st, q);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
