// digat_train_input.inc — the training input on the device: an epoch's negative samples (digat_negative_sample) and the index
// lists of a step (digat_train_batch_ids).  Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

// =================================================================================================
// negative sampling (MIND_dataset.py:26-47)
// =================================================================================================
// Behaviour i has one clicked news and a pool of m non-clicked ones (pool[pool_offsets[i] .. pool_offsets[i+1])); its row of
// samples is [click | K negatives]:
//   m == 0        every column is the click (the reference cannot handle such a behaviour; defined here, nothing is read)
//   1 <= m <= K   negative j = pool_i[j % m]                        (the reference's cyclic rule)
//   m > K         K distinct pool positions in draw order, every ordered K-subset equally likely (the distribution of the
//                 reference's rejection loop), by a partial Fisher-Yates shuffle over positions 0 .. m-1 that are never
//                 materialised: draw j takes r = j + floor(word (m - j) / 2^32) in [j, m) and picks the value now at position r,
//                 then moves the value at position j to r.  Position j is never looked at again (later draws have r > j), so the
//                 shuffle's state is the at most K (position, value) moves made so far, kept in registers; the value at a
//                 position is the last move onto it, or the position itself.  Exactly K draws, no data-dependent loop.
// The word of draw j is a pure function of (seed, epoch, i, j): drop_keep's construction with the counter e = i K + j,
//   word = hash32((uint32)e * 0x9E3779B9 + hash32(seed' + (uint32)(e >> 32))),   seed' = hash32(seed ^ hash32(epoch + 0x9E3779B9)),
// so an epoch's samples do not depend on the launch shape, and train_input.negative_samples_host restates them bit for bit.
// The multiply-shift map onto [0, m - j) is biased by at most (m - j) / 2^32 per position; ignored (a pool is a few hundred
// news at most).  A pool of 2^31 or more entries is sampled from its first 2^31 - 1.
// One thread per behaviour, grid-stride.  K <= NEG_MAX_K: the loops below are unrolled to that bound with the live part
// predicated, so the moves are indexed statically (registers, no scratch).
constexpr int NEG_MAX_K = 16;
constexpr int NEG_MAX_BLOCKS = 1024;

__device__ __forceinline__ unsigned neg_word(unsigned seed_e, long e) {
    return hash32((unsigned)e * 0x9E3779B9U + hash32(seed_e + (unsigned)(e >> 32)));
}

__global__ void __launch_bounds__(256) negative_sample_kernel(const int64_t* __restrict__ click, const int64_t* __restrict__ pool_offsets,
                                                              const int64_t* __restrict__ pool, long n, int K, unsigned seed_e,
                                                              int64_t* __restrict__ samples) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int64_t c = click[i];
        const int64_t lo = pool_offsets[i];
        const int64_t len = pool_offsets[i + 1] - lo;
        int64_t* row = samples + i * (1 + K);
        row[0] = c;
        if (len <= 0) {
            for (int j = 0; j < K; ++j) row[1 + j] = c;
        } else if (len <= K) {
            const int m = (int)len;
            for (int j = 0, p = 0; j < K; ++j) {
                row[1 + j] = pool[lo + p];
                if (++p == m) p = 0;
            }
        } else {
            const unsigned m = (unsigned)(len < 0x7FFFFFFFL ? len : 0x7FFFFFFFL);
            unsigned pos[NEG_MAX_K], val[NEG_MAX_K];
#pragma unroll
            for (int j = 0; j < NEG_MAX_K; ++j) {
                if (j < K) {
                    const unsigned word = neg_word(seed_e, i * K + j);
                    const unsigned r = (unsigned)j + (unsigned)(((unsigned long long)word * (m - (unsigned)j)) >> 32);
                    unsigned vr = r, vj = (unsigned)j;
#pragma unroll
                    for (int t = 0; t < j; ++t) {            // in move order: a later move onto the same position wins
                        vr = pos[t] == r ? val[t] : vr;
                        vj = pos[t] == (unsigned)j ? val[t] : vj;
                    }
                    pos[j] = r; val[j] = vj;
                    row[1 + j] = pool[lo + vr];              // vr < m: a position of [0, m) or a value moved from one
                }
            }
        }
    }
}

extern "C" int digat_negative_sample(const int64_t* click, const int64_t* pool_offsets, const int64_t* pool, long n, int K, uint32_t seed,
                                     uint32_t epoch, int64_t* samples, void* stream) {
    if (!click || !pool_offsets || !pool || !samples || n < 0 || K < 1) return DIGAT_ERR_ARG;
    if (K > NEG_MAX_K) return DIGAT_ERR_SHAPE;
    if (n == 0) return DIGAT_OK;
    const unsigned seed_e = hash32(seed ^ hash32(epoch + 0x9E3779B9U));
    long blocks = (n + 255) / 256;
    if (blocks > NEG_MAX_BLOCKS) blocks = NEG_MAX_BLOCKS;
    hipLaunchKernelGGL(negative_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, click, pool_offsets, pool, n, K,
                       seed_e, samples);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// =================================================================================================
// the index lists of a training step
// =================================================================================================
// Batch row b is behaviour o = order[b] of the epoch (order: a device pointer INTO the epoch's permutation).  One launch writes
//   imp[b]                 = impression[o]
//   news[b (1+K) + k]      = samples[o (1+K) + k]
//   node_ids[(b (1+K) + k) N + t] = news_node_ID[news[b (1+K) + k]][t]
//   hist[b H + t]          = history[imp[b]][t]
// each element from its sources (no thread reads what another one writes).  The large rows of the step then go through ONE
// digat_gather_tables call whose jobs index with these lists (trainer.Trainer.gather).
// Every index is clamped into its table (behaviours, news, impressions), so no read leaves one; the caller keeps them inside
// (train_input.DeviceTrainSet checks its arrays once, on the host, when it is built).
__device__ __forceinline__ long clamp_index(int64_t v, long count) { return v < 0 ? 0 : (v >= count ? count - 1 : (long)v); }

__global__ void __launch_bounds__(256) train_batch_ids_kernel(const int64_t* __restrict__ order, long B, const int64_t* __restrict__ impression,
                                                              const int64_t* __restrict__ samples, long n, int K1,
                                                              const int64_t* __restrict__ news_node_ID, long news_num, int N,
                                                              const int64_t* __restrict__ history, long impressions, int H,
                                                              int64_t* __restrict__ imp, int64_t* __restrict__ news,
                                                              int64_t* __restrict__ node_ids, int64_t* __restrict__ hist) {
    const long n_node = B * K1 * N, n_hist = B * H, n_news = B * K1;
    const long total = n_node + n_hist + n_news + B;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e < n_node) {
            const long q = e / N, t = e - q * N, b = q / K1, k = q - b * K1;
            const long o = clamp_index(order[b], n);
            node_ids[e] = news_node_ID[clamp_index(samples[o * K1 + k], news_num) * N + t];
        } else if (e < n_node + n_hist) {
            const long f = e - n_node, b = f / H, t = f - b * H;
            const long o = clamp_index(order[b], n);
            hist[f] = history[clamp_index(impression[o], impressions) * H + t];
        } else if (e < n_node + n_hist + n_news) {
            const long f = e - n_node - n_hist, b = f / K1, k = f - b * K1;
            news[f] = clamp_index(samples[clamp_index(order[b], n) * K1 + k], news_num);
        } else {
            const long b = e - n_node - n_hist - n_news;
            imp[b] = clamp_index(impression[clamp_index(order[b], n)], impressions);
        }
    }
}

extern "C" int digat_train_batch_ids(const int64_t* order, long B, const int64_t* impression, const int64_t* samples, long n, int K,
                                     const int64_t* news_node_ID, long news_num, int N, const int64_t* history, long impressions, int H,
                                     int64_t* imp, int64_t* news, int64_t* node_ids, int64_t* hist, void* stream) {
    if (!order || !impression || !samples || !news_node_ID || !history || !imp || !news || !node_ids || !hist) return DIGAT_ERR_ARG;
    if (B < 0 || n < 0 || K < 1 || N < 0 || H < 0 || news_num < 0 || impressions < 0) return DIGAT_ERR_ARG;
    if (K > NEG_MAX_K || N < 1 || H < 1) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    if (n < 1 || news_num < 1 || impressions < 1) return DIGAT_ERR_ARG;       // a batch row has nothing to point at
    const int K1 = 1 + K;
    const long total = B * K1 * N + B * H + B * K1 + B;
    long blocks = (total + 255) / 256;
    if (blocks > NEG_MAX_BLOCKS) blocks = NEG_MAX_BLOCKS;
    hipLaunchKernelGGL(train_batch_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, order, B, impression, samples, n, K1,
                       news_node_ID, news_num, N, history, impressions, H, imp, news, node_ids, hist);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
