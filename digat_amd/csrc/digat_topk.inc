// digat_topk.inc — segmented top-k: for every segment of a ragged score array, the k best elements in order (what a recommender
// is asked in service; nothing in the reference selects on the device).  Included at the end of digat_kernels.hip.
//
// Order inside a segment: score descending, ties by position ascending — the order of rank_metrics_kernel and of
// list.sort(reverse=True).  -0.0 == +0.0; a NaN comes after every number (-inf included), NaNs among themselves by position.
// Every score maps to a 32-bit key that is monotone in that order:
//   NaN -> 1;  -0.0 -> +0.0;  non-negative: bits | 0x80000000;  negative: ~bits   (-inf -> 0x007fffff: the smallest number's key)
//   0 is no score's key: it marks "not an element" (a skipped id, an unused candidate slot).
//
// Two launches, both sized by what the host knows (no read of seg_start on the host):
//   level 1, one workgroup per chunk of DIGAT_TOPK_CHUNK elements: segment s owns the chunk ids
//       [seg_start[s] / CHUNK + s,  ... + ceil(len_s / CHUNK)) — disjoint for different segments, below rows / CHUNK + segments;
//       a workgroup finds its segment by bisection over seg_start and leaves if its id is nobody's.  It writes the chunk's <= k
//       winners as (key, position in the segment), in POSITION order, into workspace slot [chunk id]; unused slots get key 0.
//   level 2, one workgroup per segment: the same selection over the segment's candidate slots (contiguous, in position order),
//       then topk_finish (as in digat_dot_topk.inc): the <= k winners ordered by counting, their score bits and ids, the fill.
//       A segment of at most TOPK_SMALL = 256 elements (a dev impression has ~37) is level 2's alone: one element per thread, keys
//       in LDS, every thread counts the elements that order before its own — level 1's workgroups for it leave at once.
// The selection (topk_select): four rounds of radix select on 256-bin LDS histograms find the k-th key T; every key above T wins,
// and of the keys equal to T the first (k - #above) in index order — a running workgroup prefix over wave ballots, which ends as
// soon as enough are found.  The passes re-read their input (level 1: 64 KB of scores per chunk, cache-resident after the first
// pass; validity of an element against the skip row is decided once and kept as one bit per element in a register pair).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   topk_chunk_kernel     VGPRs 31   SGPRs 65   LDS 4688 B   scratch 0   occupancy 8 waves / SIMD
//   topk_segment_kernel   VGPRs 26   SGPRs 79   LDS 4688 B   scratch 0   occupancy 8 waves / SIMD   (80 SGPRs before topk_finish)

#define TOPK_MAX_K 128
#define TOPK_MAX_SKIP 256
#define TOPK_SMALL 256           // segments of at most this many elements are ranked directly by level 2 (one element per thread)

struct TopkShared {
    unsigned hist[256];
    unsigned wave_tot[4];
    unsigned tie_cnt[2][4];
    unsigned win_key[TOPK_MAX_K];
    long long win_idx[TOPK_MAX_K];
    unsigned nvalid, nwin, bin, krem, bin_count;
};

__device__ __forceinline__ unsigned topk_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 1u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// hist[d] += 1 for every lane with `in`.  Scores of one sign and magnitude share their leading digit, and an all-equal segment
// shares all four: up to two digits per wave are counted by one lane for all their holders, the rest by their own atomics.
// Called by whole waves.
__device__ __forceinline__ void topk_hist_add(unsigned* hist, unsigned d, bool in, int lane) {
    unsigned long long todo = __ballot(in);
    for (int t = 0; t < 2 && todo; ++t) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d0 = (unsigned)__shfl((int)d, leader, 64);
        const bool mine = in && d == d0;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(same));
        if (mine) in = false;
        todo &= ~same;
    }
    if (in) atomicAdd(&hist[d], 1u);
}

__device__ __forceinline__ void topk_win(TopkShared& sh, unsigned key, long i) {
    const unsigned slot = atomicAdd(&sh.nwin, 1u);
    if (slot < TOPK_MAX_K) { sh.win_key[slot] = key; sh.win_idx[slot] = i; }       // never more than k: the list cannot be overrun
}

// The k-th largest key T of ld.key(0 .. n-1) (key 0: not an element) and the number `need` of elements equal to T that win beside
// every key above T; T = 0, need = 0 when at most k elements exist: all of them win.  Four rounds of radix select on sh.hist.
// `Shared`: TopkShared here, ShortShared in digat_shortlist.inc.  Called by the whole workgroup (256 threads); every thread gets the
// same T and need.
template <class Load, class Shared>
__device__ __forceinline__ void topk_threshold(const Load& ld, long n, int k, Shared& sh, unsigned& T, unsigned& need) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    sh.hist[tid] = 0;
    if (tid == 0) sh.nvalid = 0;
    __syncthreads();
    unsigned prefix = 0, mask = 0, krem = 0;
    T = 0; need = 0;                               // winners: key > T, and the first `need` with key == T
    for (int round = 0; round < 4; ++round) {
        const int shift = 24 - 8 * round;
        unsigned mine = 0;
        for (long base = 0; base < n; base += 256) {
            const long i = base + tid;
            const unsigned key = i < n ? ld.key(i) : 0u;
            const bool in = key != 0u && (key & mask) == prefix;
            topk_hist_add(sh.hist, (key >> shift) & 255u, in, lane);
            mine += in;
        }
        if (round == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor((int)mine, o, 64);
            if (lane == 0 && mine) atomicAdd(&sh.nvalid, mine);
        }
        __syncthreads();
        if (round == 0) {
            if (sh.nvalid <= (unsigned)k) break;    // everything that is an element wins (T = 0, need = 0)
            krem = (unsigned)k;
        }
        // the digit whose bin holds the krem-th largest of the elements still in play: suffix sums over the 256 bins
        const unsigned h = sh.hist[tid];
        sh.hist[tid] = 0;
        unsigned s = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = (unsigned)__shfl_down((int)s, o, 64);
            if (lane + o < 64) s += up;
        }
        if (lane == 0) sh.wave_tot[wave] = s;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) s += sh.wave_tot[w];
        if (s >= krem && s - h < krem) { sh.bin = (unsigned)tid; sh.krem = krem - (s - h); sh.bin_count = h; }
        __syncthreads();
        prefix |= sh.bin << shift;
        mask |= 255u << shift;
        krem = sh.krem;
        if (round == 3) {
            T = prefix; need = krem;
            if (sh.bin_count == need) { T -= 1; need = 0; }      // every element equal to T wins: key >= T, nothing to order
        }
    }
}

// The k best of the n elements ld.key(0 .. n-1) (key 0: not an element): sh.nwin <= k winners in sh.win_key / sh.win_idx, in no
// particular order.  Called by the whole workgroup (256 threads); ends behind a barrier.
template <class Load>
__device__ void topk_select(const Load& ld, long n, int k, TopkShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) sh.nwin = 0;
    unsigned T, need;
    topk_threshold(ld, n, k, sh, T, need);
    unsigned run = 0;                               // elements equal to T met so far (the same in every thread)
    int buf = 0;
    for (long base = 0; base < n; base += 256) {
        const long i = base + tid;
        const unsigned key = i < n ? ld.key(i) : 0u;
        if (key > T) {
            topk_win(sh, key, i);
        }
        if (run < need) {
            const bool tie = key == T;
            const unsigned long long b = __ballot(tie);
            if (lane == 0) sh.tie_cnt[buf][wave] = (unsigned)__popcll(b);
            __syncthreads();
            unsigned before = run, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned c = sh.tie_cnt[buf][w];
                if (w < wave) before += c;
                total += c;
            }
            before += (unsigned)__popcll(b & ((1ull << lane) - 1ull));
            if (tie && before < need) {
                topk_win(sh, key, i);
            }
            run += total;
            buf ^= 1;
        }
    }
    __syncthreads();
    if (tid == 0 && sh.nwin > TOPK_MAX_K) sh.nwin = TOPK_MAX_K;
    __syncthreads();
}

// The end of level 2, called by the whole workgroup after topk_select: the m <= k winners, ranked by counting (key descending,
// index ascending), go to one output row — winner(index, score, id) hands over each one's original score and id —, fill, count.
template <class Winner>
__device__ __forceinline__ void topk_finish(const TopkShared& sh, int k, float* out_scores, int64_t* out_ids, int32_t* out_count,
                                            const Winner& winner) {
    const int tid = threadIdx.x, m = (int)sh.nwin;
    if (tid == 0) *out_count = m;
    if (tid < k && tid < m) {
        const unsigned key = sh.win_key[tid];
        const long long mine = sh.win_idx[tid];
        int r = 0;
        for (int q = 0; q < m; ++q) r += sh.win_key[q] > key || (sh.win_key[q] == key && sh.win_idx[q] < mine);
        winner(mine, out_scores[r], out_ids[r]);
    } else if (tid < k) { out_scores[tid] = -INFINITY; out_ids[tid] = -1; }
}

struct TopkArgs {
    const float* scores;
    const int64_t* seg_start;
    long rows, segments;
    const int64_t* ids;
    const int64_t* skip;
    int skip_len, k;
    float* out_scores;
    int64_t* out_ids;
    int32_t* out_count;
    unsigned* ws_key;        // [chunk slots][k]
    int64_t* ws_pos;         // [chunk slots][k]: position inside the segment
};

// Row range of segment s, held inside [0, rows] whatever seg_start says: no read leaves the arrays.
__device__ __forceinline__ void topk_bounds(const TopkArgs& a, long s, long& st, long& en) {
    long b = a.seg_start[s], e = a.seg_start[s + 1];
    b = b < 0 ? 0 : (b > a.rows ? a.rows : b);
    e = e < b ? b : (e > a.rows ? a.rows : e);
    st = b; en = e;
}
__device__ __forceinline__ long topk_first_slot(const TopkArgs& a, long s) {
    long b = a.seg_start[s];
    b = b < 0 ? 0 : (b > a.rows ? a.rows : b);
    return b / DIGAT_TOPK_CHUNK + s;
}

struct TopkChunkLoad {
    const float* sc;
    unsigned long long valid;      // bit t: this thread's element t * 256 + threadIdx.x is not skipped
    __device__ __forceinline__ unsigned key(long i) const { return ((valid >> (i >> 8)) & 1ull) ? topk_key(sc[i]) : 0u; }
};
struct TopkSlotLoad {
    const unsigned* keys;
    __device__ __forceinline__ unsigned key(long i) const { return keys[i]; }
};

__global__ void __launch_bounds__(256) topk_chunk_kernel(const TopkArgs a) {
    __shared__ TopkShared sh;
    __shared__ long long skip_row[TOPK_MAX_SKIP];
    const int tid = threadIdx.x;
    const long c = blockIdx.x;
    long lo = 0, hi = a.segments;                   // first segment whose first slot lies beyond c
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (topk_first_slot(a, mid) <= c) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return;
    const long s = lo - 1;
    long st, en;
    topk_bounds(a, s, st, en);
    const long j = c - topk_first_slot(a, s);
    if (j * DIGAT_TOPK_CHUNK >= en - st || en - st <= TOPK_SMALL) return;      // small segments are level 2's alone
    const long c0 = st + j * DIGAT_TOPK_CHUNK;
    const long n = en - c0 < DIGAT_TOPK_CHUNK ? en - c0 : DIGAT_TOPK_CHUNK;
    TopkChunkLoad ld{a.scores + c0, ~0ull};
    if (a.skip) {
        for (int q = tid; q < a.skip_len; q += 256) skip_row[q] = a.skip[s * a.skip_len + q];
        __syncthreads();
        unsigned long long valid = 0;
        for (int t = 0; t < DIGAT_TOPK_CHUNK / 256; ++t) {
            const long i = (long)t * 256 + tid;
            if (i >= n) break;
            const long long id = a.ids[c0 + i];
            bool ok = true;
            for (int q = 0; q < a.skip_len; ++q) ok = ok && skip_row[q] != id;
            valid |= (unsigned long long)ok << t;
        }
        ld.valid = valid;
    }
    topk_select(ld, n, a.k, sh);
    const int m = (int)sh.nwin;
    if (tid < a.k) {
        const long o = c * a.k;
        if (tid < m) {
            const long long mine = sh.win_idx[tid];
            int r = 0;
            for (int q = 0; q < m; ++q) r += sh.win_idx[q] < mine;
            a.ws_key[o + r] = sh.win_key[tid];
            a.ws_pos[o + r] = j * DIGAT_TOPK_CHUNK + mine;
        } else {
            a.ws_key[o + tid] = 0u;
            a.ws_pos[o + tid] = -1;
        }
    }
}

__global__ void __launch_bounds__(256) topk_segment_kernel(const TopkArgs a) {
    __shared__ TopkShared sh;
    __shared__ long long skip_row[TOPK_MAX_SKIP];
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    long st, en;
    topk_bounds(a, s, st, en);
    if (en - st <= TOPK_SMALL) {
        // at most one element per thread (a dev impression has ~37): keys in LDS, every thread counts who comes before its own
        const int len = (int)(en - st);
        unsigned* keys = sh.hist;
        if (a.skip) {
            for (int q = tid; q < a.skip_len; q += 256) skip_row[q] = a.skip[s * a.skip_len + q];
            __syncthreads();
        }
        unsigned key = 0u;
        if (tid < len) {
            key = topk_key(a.scores[st + tid]);
            if (a.skip) {
                const long long id = a.ids[st + tid];
                for (int q = 0; q < a.skip_len; ++q)
                    if (skip_row[q] == id) key = 0u;
            }
        }
        keys[tid] = key;
        __syncthreads();
        int r = 0, m = 0;
        for (int q = 0; q < len; ++q) {
            const unsigned kq = keys[q];
            m += kq != 0u;
            r += kq > key || (kq == key && q < tid);
        }
        if (m > a.k) m = a.k;
        if (key != 0u && r < a.k) {
            a.out_scores[s * a.k + r] = a.scores[st + tid];
            a.out_ids[s * a.k + r] = a.ids ? a.ids[st + tid] : (int64_t)tid;
        }
        if (tid >= m && tid < a.k) {
            a.out_scores[s * a.k + tid] = -INFINITY;
            a.out_ids[s * a.k + tid] = -1;
        }
        if (tid == 0) a.out_count[s] = m;
        return;
    }
    const long chunks = (en - st + DIGAT_TOPK_CHUNK - 1) / DIGAT_TOPK_CHUNK;
    const long o = topk_first_slot(a, s) * a.k;
    const TopkSlotLoad ld{a.ws_key + o};
    topk_select(ld, chunks * a.k, a.k, sh);
    topk_finish(sh, a.k, a.out_scores + s * a.k, a.out_ids + s * a.k, a.out_count + s, [&](long long c, float& score, int64_t& id) {
        long pos = a.ws_pos[o + c];                              // candidates lie in position order
        if (pos < 0 || pos >= en - st) pos = 0;                  // a seg_start that is not non-decreasing: stay inside the segment
        score = a.scores[st + pos];
        id = a.ids ? a.ids[st + pos] : pos;
    });
}

static long topk_slots(long rows, long segments) { return rows / DIGAT_TOPK_CHUNK + segments; }

// What the selection entries ask of k (at most `max_k`: digat_shortlist.inc takes longer lists), the skip rows and the workspace; the
// entry's verdict `rc` on the rest ranks in between.
static int topk_check_args(int k, const int64_t*& skip, int& skip_len, int rc, bool need_workspace, const void* workspace,
                           int max_k = TOPK_MAX_K) {
    if (k < 1 || k > max_k || skip_len < 0 || skip_len > TOPK_MAX_SKIP) return DIGAT_ERR_ARG;
    if (rc != DIGAT_OK) return rc;
    if (!skip || skip_len == 0) { skip = nullptr; skip_len = 0; }
    return need_workspace && (!workspace || ((uintptr_t)workspace & 7)) ? DIGAT_ERR_ARG : DIGAT_OK;
}

extern "C" {

size_t digat_topk_segments_workspace_bytes(int64_t rows, int64_t segments, int k) {
    if (rows < 0 || segments <= 0 || k < 1) return 0;
    const size_t slots = (size_t)topk_slots(rows, segments);
    return align_up(slots * (size_t)k * 4, 256) + slots * (size_t)k * 8;
}

int digat_topk_segments(const float* scores, const int64_t* seg_start, int64_t rows, int64_t segments, const int64_t* ids,
                        const int64_t* skip, int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !seg_start || !out_scores || !out_ids || !out_count || rows < 0 || segments < 0) return DIGAT_ERR_ARG;
    if (skip && !ids) return DIGAT_ERR_ARG;
    if (topk_check_args(k, skip, skip_len, DIGAT_OK, segments > 0, workspace) != DIGAT_OK) return DIGAT_ERR_ARG;
    if (topk_slots(rows, segments) > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < digat_topk_segments_workspace_bytes(rows, segments, k)) return DIGAT_ERR_WORKSPACE;
    if (segments == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t slots = (size_t)topk_slots(rows, segments);
    TopkArgs a{scores, seg_start, (long)rows, (long)segments, ids, skip, skip_len, k, out_scores, out_ids, out_count,
               (unsigned*)workspace, (int64_t*)((char*)workspace + align_up(slots * (size_t)k * 4, 256))};
    if (rows > 0) {
        hipLaunchKernelGGL(topk_chunk_kernel, dim3((unsigned)slots), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(topk_segment_kernel, dim3((unsigned)segments), dim3(256), 0, st, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
