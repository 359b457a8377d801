// digat_shortlist.inc — long shortlists: digat_topk_segments' and digat_dot_topk's contracts for 1 <= m <= DIGAT_SHORTLIST_MAX_K = 1024
// (nrms.shortlist: the retrieval stage in front of a re-rank, where a shortlist that keeps the clicked news is in the hundreds).
// Included at the end of digat_kernels.hip, behind digat_dot_topk.inc: topk_key, topk_threshold and TopkChunkLoad are
// digat_topk.inc's, dot_chunk_kernel is digat_dot_topk.inc's.  The selection kernels of those two files stay as they are: at 1024
// entries TopkShared's winner lists alone would be 12 KB in each of them, their write-back is one thread per winner (k <= 256),
// and ranking by counting is m^2 compares per list.
//
// Order, keys, skip rows, the clamped seg_start and the chunk slots are digat_topk.inc's: key descending, ties by position, key 0 =
// not an element; segment s owns the chunk slots [seg_start[s] / CHUNK + s, ... + ceil(len / CHUNK)).
//   level 1, shortlist_chunk_kernel, one workgroup per chunk slot: topk_threshold — topk_select's four rounds of radix select on
//       256-bin LDS histograms — finds the m-th key T and the number `need` of elements equal to T that still win;
//       short_collect then walks the chunk once in base + tid order and gives every winner (key > T, or one of the first `need`
//       with key == T) its ordinal among the winners from a workgroup prefix over two wave ballots: one barrier per 256 elements,
//       no atomics, no rank by counting.  The <= m winners go to the chunk's m workspace slots as (key, position in the chunk), in
//       position order; unused slots get key 0.
//   level 2, shortlist_segment_kernel, one workgroup per segment: the same two steps over the segment's chunks * m slots; the
//       <= m winners land in LDS as unique 64-bit words (key, ~ordinal) — the ordinal grows with the position — beside their
//       positions, a bitonic network over the next power of two (at most 1024 words, 8 KB, two pairs per thread and step;
//       short_bitonic, which digat_pl_sample.inc runs over its own records) orders them,
//       and the row is written: score bits and ids read back by position, then the fill, then the count.
//       A segment of at most SHORT_SMALL = 1024 elements is level 2's alone: load, sort, write; level 1 leaves at once.
// Uniform mode (seg_start == nullptr): `segments` segments of seg_len elements each, segment s at s * seg_len with the chunk slots
//   [s * seg_chunks, + seg_chunks); the id of position p is ids[p] — one row shared by all segments, digat_dot_shortlist's pool — or
//   p; an id outside [0, id_limit) is no element.  No offsets and no [segments * seg_len] ids in memory.
// digat_dot_shortlist walks the users in slabs: dot_chunk_kernel<false, SHORT_DOT_CHUNK> stores the slab's [slab, P] scores in the
//   workspace — digat_dot_scores' kernel over chunks of 256 pool positions in place of 2 048: the same sub-tiles through the same
//   dot_tile, so the same bits, but 1 020 workgroups for a slab of 256 users at P = 65 237 where chunks of 2 048 give 128, half
//   the chip's CUs, each walking 32 sub-tiles (measured on an MI355X, G = 4 096, m = 256: 17.9 ms per call with the long chunks) —,
//   and the two levels select from them in uniform mode.  The launches depend on G, P and the slab alone.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   shortlist_chunk_kernel     VGPRs 33   SGPRs 68   LDS 3176 B    scratch 0   occupancy 8 waves / SIMD
//   shortlist_segment_kernel   VGPRs 32   SGPRs 76   LDS 19560 B   scratch 0   occupancy 8 waves / SIMD (eight 19.1 KB workgroups per CU)
//   dot_chunk_kernel<false, 256>   VGPRs 74   SGPRs 69   LDS 43008 B static   scratch 0   occupancy 3 waves / SIMD (by static LDS): the
//                              lines of dot_chunk_kernel<false> at its own chunk of 2 048
// topk_chunk_kernel, topk_segment_kernel and dot_topk_user_kernel (topk_select now calls the shared topk_threshold), dot_chunk_kernel<true>
// and <false> keep the lines of their files, restated from the same build as VGPRs / SGPRs / LDS: 31 / 65 / 4688, 26 / 79 / 4688,
// 26 / 68 / 2632, 118 / 106 / 43008, 74 / 69 / 43008.

#define SHORT_MAX_K DIGAT_SHORTLIST_MAX_K
#define SHORT_SMALL 1024         // segments of at most this many elements are sorted directly by level 2
#define SHORT_SLAB_USERS 256     // digat_dot_shortlist's slab when the caller names none
#define SHORT_DOT_CHUNK 256      // pool positions per workgroup of the slab's score launch

static_assert(SHORT_MAX_K == 1024 && SHORT_SMALL == 1024, "ShortSort holds 1024 words: the longest list, and the longest segment sorted directly");
static_assert(DIGAT_TOPK_CHUNK / 256 <= 64, "a thread keeps the validity of its elements of a chunk in one 64-bit mask");

struct ShortArgs {
    const float* scores;
    const int64_t* seg_start;    // nullptr: uniform mode
    long rows, segments, seg_len, seg_chunks;
    const int64_t* ids;          // [rows]; uniform mode: [seg_len], shared by all segments; nullptr: positions
    long id_limit;               // uniform mode with ids: ids outside [0, id_limit) are no elements; 0: no such test
    const int64_t* skip;
    int skip_len, m;
    float* out_scores;
    int64_t* out_ids;
    int32_t* out_count;
    uint2* ws;                   // [chunk slots][m]: (key, position inside the chunk)
};

struct ShortSeg {
    long st, len, slot0;         // first row, elements, first chunk slot
    const int64_t* ids;          // id of position p: ids[p], or p
};

// Segment s, held inside [0, rows] whatever seg_start says: no read leaves the arrays.
__device__ __forceinline__ ShortSeg short_segment(const ShortArgs& a, long s) {
    if (!a.seg_start) return ShortSeg{s * a.seg_len, a.seg_len, s * a.seg_chunks, a.ids};
    long b = a.seg_start[s], e = a.seg_start[s + 1];
    b = b < 0 ? 0 : (b > a.rows ? a.rows : b);
    e = e < b ? b : (e > a.rows ? a.rows : e);
    return ShortSeg{b, e - b, b / DIGAT_TOPK_CHUNK + s, a.ids ? a.ids + b : nullptr};
}

// Is position p of the segment an element: its id inside the limit and not in the skip row (LDS).
__device__ __forceinline__ bool short_valid(const ShortArgs& a, const ShortSeg& g, const long long* skip_row, long p) {
    const long long id = g.ids ? (long long)g.ids[p] : (long long)p;
    bool ok = a.id_limit == 0 || (id >= 0 && id < a.id_limit);
    for (int q = 0; q < a.skip_len; ++q) ok = ok && skip_row[q] != id;
    return ok;
}

struct ShortShared {
    unsigned hist[256];
    unsigned wave_tot[4];
    unsigned cnt[2][4][2];       // [buffer][wave]: elements above T, elements equal to T
    unsigned nvalid, bin, krem, bin_count, count;
};

struct ShortSlotLoad {
    const uint2* e;
    __device__ __forceinline__ unsigned key(long i) const { return e[i].x; }
};

// One pass over ld.key(0 .. n-1) in index order: emit(ordinal, key, index) for every winner — key > T, or one of the first `need`
// elements with key == T —, the ordinals counting the winners in index order.  Returns their number, in every thread.  Per 256
// elements: two ballots per wave, the waves' counts through LDS (double-buffered: one barrier), and each thread adds up what the
// waves before it and the lanes below it contribute.  Called by the whole workgroup.
template <class Load, class Emit>
__device__ unsigned short_collect(const Load& ld, long n, unsigned T, unsigned need, ShortShared& sh, const Emit& emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lower = (1ull << lane) - 1ull;
    unsigned run_win = 0, run_tie = 0;               // winners, and elements equal to T, met so far (the same in every thread)
    int buf = 0;
    for (long base = 0; base < n; base += 256) {
        const long i = base + tid;
        const unsigned key = i < n ? ld.key(i) : 0u;
        const bool above = key > T, tie = need != 0u && key == T;
        const unsigned long long ba = __ballot(above), bt = __ballot(tie);
        if (lane == 0) { sh.cnt[buf][wave][0] = (unsigned)__popcll(ba); sh.cnt[buf][wave][1] = (unsigned)__popcll(bt); }
        __syncthreads();
        unsigned win_before = run_win, tie_before = run_tie;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned ca = sh.cnt[buf][w][0], ct = sh.cnt[buf][w][1];
            const unsigned left = run_tie < need ? need - run_tie : 0u;            // ties that can still win when wave w begins
            const unsigned won = ca + (ct < left ? ct : left);
            if (w < wave) { win_before += won; tie_before += ct; }
            run_win += won;
            run_tie += ct;
        }
        const unsigned tl = (unsigned)__popcll(bt & lower);
        const unsigned left = tie_before < need ? need - tie_before : 0u;
        if (above || (tie && tl < left)) emit(win_before + (unsigned)__popcll(ba & lower) + (tl < left ? tl : left), key, i);
        buf ^= 1;
    }
    return run_win;
}

__global__ void __launch_bounds__(256) shortlist_chunk_kernel(const ShortArgs a) {
    __shared__ ShortShared sh;
    __shared__ long long skip_row[TOPK_MAX_SKIP];
    const int tid = threadIdx.x;
    const long c = blockIdx.x;
    long s;
    if (!a.seg_start) {
        s = c / a.seg_chunks;
    } else {
        long lo = 0, hi = a.segments;               // first segment whose first slot lies beyond c
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (short_segment(a, mid).slot0 <= c) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) return;
        s = lo - 1;
    }
    const ShortSeg g = short_segment(a, s);
    const long p0 = (c - g.slot0) * DIGAT_TOPK_CHUNK;
    if (p0 >= g.len || g.len <= SHORT_SMALL) return;                          // small segments are level 2's alone
    const long n = g.len - p0 < DIGAT_TOPK_CHUNK ? g.len - p0 : DIGAT_TOPK_CHUNK;
    TopkChunkLoad ld{a.scores + g.st + p0, ~0ull};
    if (a.skip || a.id_limit) {
        for (int q = tid; q < a.skip_len; q += 256) skip_row[q] = a.skip[s * a.skip_len + q];
        __syncthreads();
        unsigned long long valid = 0;
        for (int t = 0; t < DIGAT_TOPK_CHUNK / 256; ++t) {
            const long i = (long)t * 256 + tid;
            if (i >= n) break;
            valid |= (unsigned long long)short_valid(a, g, skip_row, p0 + i) << t;
        }
        ld.valid = valid;
    }
    unsigned T, need;
    topk_threshold(ld, n, a.m, sh, T, need);
    uint2* slot = a.ws + c * a.m;
    const unsigned total = short_collect(ld, n, T, need, sh, [&](unsigned o, unsigned key, long i) {
        if (o < (unsigned)a.m) slot[o] = make_uint2(key, (unsigned)i);           // never more than m: the slot cannot be overrun
    });
    for (unsigned q = total + tid; q < (unsigned)a.m; q += 256) slot[q] = make_uint2(0u, 0u);
}

struct ShortSort {
    unsigned long long w[SHORT_MAX_K];       // (key, ~ordinal): a larger word orders first, no two winners share one; 0: no winner
    long long pos[SHORT_MAX_K];              // by ordinal: the winner's position inside the segment
};

// The bitonic network over w[0 .. n2) in LDS, n2 a power of two of at most SHORT_MAX_K records, two pairs per thread and step:
// afterwards x stands in front of y wherever before(x, y) — a strict total order over the records (no two compare equal).  Called
// by the whole workgroup of 256 threads behind a barrier; ends on one.  digat_pl_sample.inc orders its (key, position) records here.
template <class T, class Before>
__device__ __forceinline__ void short_bitonic(T* w, int n2, const Before& before) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const T x = w[i], y = w[p];
                if ((i & k) == 0 ? before(y, x) : before(x, y)) { w[i] = y; w[p] = x; }
            }
            __syncthreads();
        }
}

__global__ void __launch_bounds__(256) shortlist_segment_kernel(const ShortArgs a) {
    __shared__ ShortShared sh;
    __shared__ ShortSort so;
    __shared__ long long skip_row[TOPK_MAX_SKIP];
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    const ShortSeg g = short_segment(a, s);
    if (tid == 0) sh.count = 0;
    int held;                                       // so.w[0 .. held) may hold winners
    if (g.len <= SHORT_SMALL) {
        const bool test = a.skip || a.id_limit;
        if (test) {
            for (int q = tid; q < a.skip_len; q += 256) skip_row[q] = a.skip[s * a.skip_len + q];
            __syncthreads();
        }
        for (int i = tid; i < SHORT_SMALL; i += 256) {
            unsigned key = 0u;
            if (i < g.len) {
                key = topk_key(a.scores[g.st + i]);
                if (test && !short_valid(a, g, skip_row, i)) key = 0u;
            }
            so.w[i] = key ? ((unsigned long long)key << 32) | (unsigned)~i : 0ull;
            so.pos[i] = i;
        }
        held = (int)g.len;
    } else {
        const long chunks = (g.len + DIGAT_TOPK_CHUNK - 1) / DIGAT_TOPK_CHUNK;
        const uint2* slots = a.ws + g.slot0 * a.m;
        const ShortSlotLoad ld{slots};
        for (int i = tid; i < SHORT_MAX_K; i += 256) so.w[i] = 0ull;
        unsigned T, need;
        topk_threshold(ld, chunks * a.m, a.m, sh, T, need);                  // its barriers stand between the zeros and the winners
        const unsigned total = short_collect(ld, chunks * a.m, T, need, sh, [&](unsigned o, unsigned key, long i) {
            if (o < SHORT_MAX_K) {
                so.w[o] = ((unsigned long long)key << 32) | (unsigned)~o;
                so.pos[o] = (i / a.m) * DIGAT_TOPK_CHUNK + (long)slots[i].y;   // slots lie in position order
            }
        });
        held = total < SHORT_MAX_K ? (int)total : SHORT_MAX_K;
    }
    __syncthreads();
    int n2 = 2;
    while (n2 < held) n2 <<= 1;
    short_bitonic(so.w, n2, [](unsigned long long x, unsigned long long y) { return x > y; });
    for (int j = tid; j < n2; j += 256)             // the winners stand in front: the last of them says how many they are
        if (so.w[j] != 0ull && (j + 1 == n2 || so.w[j + 1] == 0ull)) sh.count = (unsigned)(j + 1 < a.m ? j + 1 : a.m);
    __syncthreads();
    const int count = (int)sh.count;
    float* out_scores = a.out_scores + s * a.m;
    int64_t* out_ids = a.out_ids + s * a.m;
    for (int j = tid; j < a.m; j += 256) {
        if (j < count) {
            long pos = so.pos[~(unsigned)so.w[j] & (SHORT_MAX_K - 1)];
            if (pos < 0 || pos >= g.len) pos = 0;                             // slots of a malformed seg_start: stay inside the segment
            out_scores[j] = a.scores[g.st + pos];
            out_ids[j] = g.ids ? g.ids[pos] : (int64_t)pos;
        } else {
            out_scores[j] = -INFINITY;
            out_ids[j] = -1;
        }
    }
    if (tid == 0) a.out_count[s] = count;
}

static long short_chunks(long len) { return (len + DIGAT_TOPK_CHUNK - 1) / DIGAT_TOPK_CHUNK; }

// Both levels on `st`: level 1 over `slots` chunk slots (0: every segment is level 2's alone), level 2 over the segments.
static int short_launch(const ShortArgs& a, long slots, hipStream_t st) {
    if (slots > 0) {
        hipLaunchKernelGGL(shortlist_chunk_kernel, dim3((unsigned)slots), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(shortlist_segment_kernel, dim3((unsigned)a.segments), dim3(256), 0, st, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

static long short_dot_chunks(long pool) { return (pool + SHORT_DOT_CHUNK - 1) / SHORT_DOT_CHUNK; }
static long short_slab(int64_t slab_users) { return slab_users > 0 ? (long)slab_users : SHORT_SLAB_USERS; }

static size_t short_dot_workspace_bytes(int64_t G, int64_t P, int m, int64_t slab_users) {
    if (G < 0 || P < 0 || m < 1 || m > SHORT_MAX_K) return 0;
    const size_t slab = (size_t)short_slab(slab_users);
    return align_up(slab * (size_t)P * sizeof(float), 256) + slab * (size_t)short_chunks((long)P) * (size_t)m * sizeof(uint2);
}

// digat_dot_shortlist behind its product, shared with digat_qdot_shortlist: `check(slab)` is the entry's verdict on its operands for
// launches of `slab` users, `scores(g0, gs, out, st)` launches the [gs, P] scores of users g0 .. g0 + gs into `out` on `st`.
template <class Check, class Scores>
static int short_dot_slabs(const int64_t* pool, int64_t G, int64_t N, int64_t P, const int64_t* skip, int skip_len, int m, int64_t slab_users,
                           float* out_scores, int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes, hipStream_t st,
                           const Check& check, const Scores& scores) {
    if (!out_scores || !out_ids || !out_count) return DIGAT_ERR_ARG;
    const long slab = G > 0 && G < short_slab(slab_users) ? (long)G : short_slab(slab_users);      // users per launch
    int rc = check(slab);
    if (rc == DIGAT_OK && ((double)slab * (double)short_chunks((long)P) > 2147483647.0 ||
                           (double)dot_tiles(slab) * (double)short_dot_chunks((long)P) > 2147483647.0)) rc = DIGAT_ERR_SHAPE;
    rc = topk_check_args(m, skip, skip_len, rc, G > 0 && P > 0, workspace, SHORT_MAX_K);
    if (rc != DIGAT_OK) return rc;
    if (G > 0 && P > 0 && workspace_bytes < short_dot_workspace_bytes(G, P, m, slab_users)) return DIGAT_ERR_WORKSPACE;
    float* slab_scores = (float*)workspace;
    uint2* ws = (uint2*)((char*)workspace + align_up((size_t)short_slab(slab_users) * (size_t)P * sizeof(float), 256));
    for (long g0 = 0; g0 < (long)G; g0 += slab) {
        const long gs = (long)G - g0 < slab ? (long)G - g0 : slab;
        if (P > 0) {
            scores(g0, gs, slab_scores, st);
            DIGAT_CHECK_LAUNCH();
        }
        const ShortArgs a{slab_scores, nullptr, gs * (long)P, gs, (long)P, short_chunks((long)P), pool, pool ? (long)N : 0,
                          skip ? skip + g0 * skip_len : nullptr, skip_len, m, out_scores + g0 * m, out_ids + g0 * m, out_count + g0, ws};
        rc = short_launch(a, P > SHORT_SMALL ? gs * a.seg_chunks : 0, st);
        if (rc != DIGAT_OK) return rc;
    }
    return DIGAT_OK;
}

extern "C" {

size_t digat_shortlist_segments_workspace_bytes(int64_t rows, int64_t segments, int m) {
    if (rows < 0 || segments <= 0 || m < 1 || m > SHORT_MAX_K) return 0;
    return (size_t)topk_slots(rows, segments) * (size_t)m * sizeof(uint2);
}

int digat_shortlist_segments(const float* scores, const int64_t* seg_start, int64_t rows, int64_t segments, const int64_t* ids,
                             const int64_t* skip, int skip_len, int m, float* out_scores, int64_t* out_ids, int32_t* out_count,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !seg_start || !out_scores || !out_ids || !out_count || rows < 0 || segments < 0) return DIGAT_ERR_ARG;
    if (skip && !ids) return DIGAT_ERR_ARG;
    if (topk_check_args(m, skip, skip_len, DIGAT_OK, segments > 0, workspace, SHORT_MAX_K) != DIGAT_OK) return DIGAT_ERR_ARG;
    if (topk_slots(rows, segments) > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < digat_shortlist_segments_workspace_bytes(rows, segments, m)) return DIGAT_ERR_WORKSPACE;
    if (segments == 0) return DIGAT_OK;
    const ShortArgs a{scores, seg_start, (long)rows, (long)segments, 0, 0, ids, 0, skip, skip_len, m, out_scores, out_ids, out_count,
                      (uint2*)workspace};
    return short_launch(a, rows > SHORT_SMALL ? topk_slots(rows, segments) : 0, (hipStream_t)stream);
}

size_t digat_dot_shortlist_workspace_bytes(int64_t G, int64_t P, int m, int64_t slab_users) {
    return short_dot_workspace_bytes(G, P, m, slab_users);
}

int digat_dot_shortlist(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                        const int64_t* skip, int skip_len, int m, int64_t slab_users, float* out_scores, int64_t* out_ids,
                        int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    return short_dot_slabs(
        pool, G, N, P, skip, skip_len, m, slab_users, out_scores, out_ids, out_count, workspace, workspace_bytes, (hipStream_t)stream,
        [&](long slab) { return dot_check(users, news, pool, G < 0 ? G : slab, N, P, d); },
        [&](long g0, long gs, float* slab_scores, hipStream_t st) {
            DotArgs da{users + g0 * d, news, pool, gs, (long)N, (long)P, d, nullptr, 0, 0, dot_tiles(gs), short_dot_chunks((long)P), slab_scores,
                       nullptr, nullptr, nullptr, nullptr};
            hipLaunchKernelGGL((dot_chunk_kernel<false, SHORT_DOT_CHUNK>), dim3((unsigned)(da.tiles * da.chunks)), dim3(256), 0, st, da);
        });
}

}  // extern "C"
