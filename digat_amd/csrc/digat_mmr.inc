// digat_mmr.inc — diversified top-k: greedy maximal-marginal-relevance selection over a short list per user (the last stage behind
// util.recommend / nrms.recommend: "the k best that are not copies of each other").  Included at the end of digat_kernels.hip,
// behind digat_topk.inc (topk_key: the order of a step's winner is that of digat_topk_segments) and digat_dot_topk.inc (dot_load4,
// DOT_KB, DOT_LD, dot_wave_sync: the product below is dot_tile's loop, so sim(i, j) has the bits of digat_dot_scores).
//
// mmr_kernel, one workgroup (4 waves) per user:
//   the list's ids (-1: beyond count[g] or outside [0, N): a zero row, no element), then the [Mu, Mu] Gram of the gathered rows
//   (mmr_gram), Mu = count rounded up to 16 — wave w owns the 16-row tile rows w and w + 4 and every tile column as 2 x 8 MFMA tiles, the rows
//   staged through LDS in K blocks of DOT_KB channels (tail padded with zeros, k-steps wholly beyond d not issued), the next block's
//   global loads in flight under the MFMAs.  The Gram lands in LDS over the staging area (the accumulators are in registers by
//   then), row stride Mp + 4 with Mp = M rounded up to 16: 128 * 132 * 4 = 67 584 B at M = 128, two workgroups per CU.
//   Then wave 0 alone runs the k greedy steps, list positions lane and lane + 64 per lane: scores, pen, the step a position was
//   picked at and its category counter live in registers; a step is the two keys, a wave max over the 32-bit keys, two ballots for
//   the lowest position that holds the max, the picked row of the Gram from LDS and — with a cap — the picked category from LDS.
//   No workgroup barrier inside the loop; waves 1 .. 3 have left, so another workgroup's product runs under this one's steps.
//   value = lam * s - mu * pen is three rounded operations (mmr_value: contraction switched off for that expression).
//   The outputs are written once, behind the loop: position p picked at step t writes slot t, slots from the count on get -1 / -inf.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup; dynamic LDS
// 4 Mp max(Mp + 4, DOT_LD) bytes (2 304 B at M <= 16, 67 584 B at M = 128):
//   mmr_kernel   VGPRs 46 + AGPRs 64 (the 2 x 8 accumulator tiles)   SGPRs 87   LDS 1536 B static   scratch 0   occupancy 4 waves / SIMD
//   (by registers; at M = 128 the 69 120 B of LDS allow two workgroups = 2 waves / SIMD)
// The Gram is mmr_gram, a __device__ function that digat_listq.inc calls too: one product in the sources.  With the loop written out
// inside mmr_kernel the compiler reported 44 VGPRs; 44 + 64 and 46 + 64 both allocate 112 registers a lane (granule 8), scratch is 0
// either way and the selection's bits are the same (tests/test_hip_diversify.py), so the function is shared and not copied.
// The count clamp and the fill of unused slots (sel_count, sel_fill) are __device__ functions too, called by digat_calibrate.inc and
// digat_rerank.inc: the line above is what the compiler reports with them, as it was without.  The one-wave winner is not (below).

#define MMR_MAX_M TOPK_MAX_K

static_assert(MMR_MAX_M == 128, "mmr_kernel holds a list as two positions per lane of one wave and 8 x 8 MFMA tiles");
static_assert(DOT_KB == 32, "mmr_kernel stages 8 threads x 4 channels per row");

struct MmrArgs {
    const int64_t* ids;
    const float* scores;
    const int32_t* count;
    long G;
    int M;
    const float* vectors;
    long N;
    int d;
    const int32_t* category;
    int q;
    float lam, mu;
    int k;
    int64_t* out_ids;
    float* out_scores;
    int32_t* out_count;
    int ld;                  // row stride of the Gram in LDS: M rounded up to 16, + 4
};

// lam * s - mu * pen with each product and the difference rounded: never an fma.
__device__ __forceinline__ float mmr_value(float lam, float s, float mu, float pen) {
#pragma clang fp contract(off)
    const float rel = lam * s;
    const float red = mu * pen;
    return rel - red;
}

// The pieces every greedy re-rank kernel shares (cal_kernel, rr_kernel and rr_gram_kernel call them too).
// A list's count clamped to [0, M]; no count: M.
__device__ __forceinline__ int sel_count(const int32_t* count, const long g, const int M) {
    const int cnt = count ? count[g] : M;
    return cnt < 0 ? 0 : (cnt > M ? M : cnt);
}

// Slots t .. k - 1 of list g hold no pick: -inf / -1.  Thread `tid` of `threads`.
__device__ __forceinline__ void sel_fill(float* out_scores, int64_t* out_ids, const long g, const int k, const int t, const int tid,
                                         const int threads) {
    for (int x = t + tid; x < k; x += threads) {
        out_scores[g * k + x] = -INFINITY;
        out_ids[g * k + x] = -1;
    }
}

// NOT shared: the one-wave winner (a wave max over the 32-bit keys, two ballots for the lowest position that holds it), which
// mmr_kernel and rr_gram_kernel (digat_rerank.inc) each write out.  As a function — returning j, or j through a reference — the
// "nothing eligible" exit merges with the found position and j becomes a per-lane value: a VGPR, the Gram's row address a vector
// multiply, where the ballots give a scalar.  Registers, LDS and occupancy did not move, but both kernels measured about 1 % slower.

// The [16 T, 16 T] Gram of the rows lid[] names (-1: a zero row) into L as S[col][row], row stride ld — the one product of this file and
// of digat_listq.inc.  Called by all 256 threads of the workgroup, lid[] written and a barrier passed; returns behind the barrier
// that makes the Gram visible.  L holds max(16 T * DOT_LD, 16 T * ld) floats.
__device__ __forceinline__ void mmr_gram(float* const L, const long long* lid, const float* vectors, const int d, const int T, const int ld) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;     // this thread stages rows r0 + 32 h, channels c4 .. c4 + 3
    const bool vec = (d & 3) == 0 && (((uintptr_t)vectors) & 15) == 0;
    const float* row[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const long long id = lid[r0 + 32 * h];
        row[h] = id >= 0 ? vectors + id * d : nullptr;
    }
    v4f acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int tc = 0; tc < 8; ++tc) acc[i][tc] = (v4f){0.f, 0.f, 0.f, 0.f};
    float4 rv[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) rv[h] = dot_load4(row[h], c4, d, vec);
    for (int kb = 0; kb < d; kb += DOT_KB) {
#pragma unroll
        for (int h = 0; h < 4; ++h)
            if (r0 + 32 * h < 16 * T) *(float4*)&L[(r0 + 32 * h) * DOT_LD + c4] = rv[h];
        __syncthreads();
        if (kb + DOT_KB < d) {
#pragma unroll
            for (int h = 0; h < 4; ++h) rv[h] = dot_load4(row[h], kb + DOT_KB + c4, d, vec);
        }
        if (wave < T) {                               // wave-uniform: this wave owns a tile row of the user's Gram
#pragma unroll
            for (int ks = 0; ks < DOT_KB / 4; ++ks) {
                if (kb + ks * 4 < d) {                // workgroup-uniform: no k-step wholly beyond d
                    const int k = ks * 4 + lq;
                    const float a0 = L[(16 * wave + lr) * DOT_LD + k];
                    const float a1 = wave + 4 < T ? L[(16 * (wave + 4) + lr) * DOT_LD + k] : 0.f;
#pragma unroll
                    for (int tc = 0; tc < 8; ++tc) {
                        if (tc < T) {
                            const float b = L[(16 * tc + lr) * DOT_LD + k];
                            acc[0][tc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][tc], 0, 0, 0);
                            if (wave + 4 < T) acc[1][tc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][tc], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // D[row = position 16 tr + 4 lq + r][col = position 16 tc + lr], stored as S[col][row .. row + 3]: the product is symmetric
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int tr = wave + 4 * i;
        if (tr < T) {
#pragma unroll
            for (int tc = 0; tc < 8; ++tc)
                if (tc < T)
                    *(float4*)&L[(16 * tc + lr) * ld + 16 * tr + 4 * lq] = make_float4(acc[i][tc][0], acc[i][tc][1], acc[i][tc][2], acc[i][tc][3]);
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) mmr_kernel(const MmrArgs a) {
    extern __shared__ float4 mmr_lds[];              // the staged rows [Mu][DOT_LD], then the Gram [Mu][ld]
    __shared__ long long lid[MMR_MAX_M];             // vectors row of every list position, -1: not an element
    __shared__ int lcat[MMR_MAX_M];
    float* const L = (float*)mmr_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int cnt = sel_count(a.count, g, a.M);
    const int T = (cnt + 15) >> 4;                   // 16-row tiles of this user's Gram: <= 8, and 16 T <= ld - 4
    if (tid < MMR_MAX_M) {
        long long id = -1;
        if (tid < cnt) {
            id = (long long)a.ids[g * a.M + tid];
            if (id < 0 || id >= a.N) id = -1;
        }
        lid[tid] = id;
    }
    __syncthreads();

    // ---- the Gram: dot_tile's loop over 16 T rows on both sides
    mmr_gram(L, lid, a.vectors, a.d, T, a.ld);
    if (wave != 0) return;

    // ---- the greedy steps: one wave, positions lane and lane + 64
    float s[2], pen[2];
    long long id[2];
    int cat[2], picked[2];
    unsigned same[2];                                // already-selected elements of this position's category
    bool el[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pos = lane + 64 * h;
        id[h] = lid[pos];
        el[h] = id[h] >= 0;                          // then pos < cnt <= M
        s[h] = el[h] ? a.scores[g * a.M + pos] : 0.f;
        cat[h] = el[h] && a.q > 0 ? a.category[id[h]] : 0;
        pen[h] = 0.f;
        picked[h] = -1;
        same[h] = 0u;
        if (a.q > 0) lcat[pos] = cat[h];
    }
    dot_wave_sync();
    int t = 0;
    for (; t < a.k; ++t) {
        unsigned key[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool eligible = el[h] && picked[h] < 0 && (a.q == 0 || same[h] < (unsigned)a.q);
            key[h] = eligible ? topk_key(mmr_value(a.lam, s[h], a.mu, pen[h])) : 0u;
        }
        unsigned best = key[0] > key[1] ? key[0] : key[1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)best, o, 64);
            best = other > best ? other : best;
        }
        if (best == 0u) break;                       // nothing eligible
        const unsigned long long low = __ballot(key[0] == best);
        const int j = low ? __ffsll((long long)low) - 1 : 64 + __ffsll((long long)__ballot(key[1] == best)) - 1;
        if (j == lane) picked[0] = t;
        if (j == lane + 64) picked[1] = t;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float sim = el[h] ? L[j * a.ld + lane + 64 * h] : 0.f;
            pen[h] = fmaxf(pen[h], sim);
        }
        if (a.q > 0) {
            const int cj = lcat[j];
#pragma unroll
            for (int h = 0; h < 2; ++h) same[h] += cat[h] == cj;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (picked[h] >= 0) {
            a.out_scores[g * a.k + picked[h]] = s[h];
            a.out_ids[g * a.k + picked[h]] = (int64_t)id[h];
        }
    }
    sel_fill(a.out_scores, a.out_ids, g, a.k, t, lane, 64);
    if (lane == 0) a.out_count[g] = t;
}

extern "C" {

size_t digat_mmr_select_workspace_bytes(int64_t users, int m, int k) {
    (void)users; (void)m; (void)k;
    return 0;                                        // the Gram never leaves LDS
}

int digat_mmr_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const float* vectors, int64_t N, int d,
                     const int32_t* category, int max_per_category, float lam, float mu, int k, int64_t* out_ids, float* out_scores,
                     int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!ids || !scores || !vectors || !out_ids || !out_scores || !out_count || G < 0 || N < 0 || max_per_category < 0) return DIGAT_ERR_ARG;
    if (!(lam >= 0.f && lam <= 1.f) || (max_per_category > 0 && !category)) return DIGAT_ERR_ARG;
    if (k < 1 || k > TOPK_MAX_K || M < 1 || M > MMR_MAX_M || d < 1 || d > (1 << 24) || G > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    const int Mp = (M + 15) / 16 * 16;
    MmrArgs a{ids, scores, count, (long)G, M, vectors, (long)N, d, category, max_per_category, lam, mu, k, out_ids, out_scores, out_count,
              Mp + 4};
    const size_t lds = (size_t)Mp * (size_t)(Mp + 4 > DOT_LD ? Mp + 4 : DOT_LD) * sizeof(float);
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)mmr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DIGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(mmr_kernel, dim3((unsigned)G), dim3(256), lds, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
