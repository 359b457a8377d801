// digat_dot_topk.inc — inner-product retrieval: for every user vector the k best rows of a news table by <user, news>, without the
// [G, P] score matrix ever reaching memory (nrms.recommend; the candidate generator in front of util.recommend).  Included at the
// end of digat_kernels.hip, behind digat_topk.inc whose topk_key / topk_select / TopkShared it uses: the order of a user's elements
// is that of digat_topk_segments (key descending, ties by pool position, NaNs last, key 0 = not an element).
//
// score(g, p) = the fp32 fmaf chain over c = 0 .. d-1 from 0, on v_mfma_f32_16x16x4_f32 (k-ordered inside and across instructions).
// Every score runs through the same loop — K blocks of DOT_KB channels, the tail padded with zeros in BOTH operands, k-steps wholly
// beyond d not issued — so its bits depend on the two vectors and d alone, whichever entry, tile or pool order computed it.
//
// Level 1, dot_chunk_kernel, one workgroup (4 waves) per (tile of 64 users, chunk of DIGAT_DOT_TOPK_CHUNK pool positions):
//   per sub-tile of 64 pool positions: the pool ids (-1: beyond P or outside [0, N): a zero row, key 0), then the 64 x 64 product
//   — wave w owns users 32 (w / 2) .. + 32 and positions 32 (w % 2) .. + 32 as 2 x 2 MFMA tiles, news = A, users = B, operands
//   staged through LDS in K blocks, the next block's global loads in flight under the MFMAs — lands in LDS (Ss).
//   digat_dot_scores stores Ss and is done.  digat_dot_topk: wave w owns users 16 w .. + 16 and their lists outright (no barrier in
//   the epilogue), one position per lane.  It first notes which of its users have a key above their threshold (0 at first); for
//   those, the keys above the threshold and not in the user's skip row (checked for those keys only: the lanes hold the skip row,
//   and either the passing ids or the row's entries are broadcast one by one, whichever are fewer) are appended, in position
//   order, to the user's candidate list in LDS (k + 64 entries of (score bits, position in the chunk)).  A list that would grow
//   beyond max(2 k, 32) entries — or beyond its k + 64 — is first cut back to its k best by the wave (dot_cut: every entry's rank
//   counted against (key, ~index) words broadcast from LDS), in list = position order; the threshold becomes the smallest key
//   kept — a later key has to beat it, an equal one loses the position tie.  Cutting early keeps the cuts short and the
//   threshold fresh.  At the end of the chunk lists longer than k are cut, and the <= k entries go to workspace slot
//   [user][chunk][k]; unused entries carry position DOT_NOPOS.
// Level 2, dot_topk_user_kernel, one workgroup per user: topk_select over the user's chunks * k slots (position order), then
//   topk_finish (digat_topk.inc: order by counting, fill, count) with score bits from the slots and ids from the pool.
// The cut is a wave's own count and not topk_select: measured on an MI355X at G = 4 096, P = 65 237, d = 400, topk_select over a
// list (the whole workgroup behind barriers, one user at a time) made the call 7.7 ms at k = 10 and 42.8 ms at k = 100; the
// wave-local cut with the early limit 4.4 and 13.1 ms (DESIGN section 8).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup; the fused kernel
// adds 512 (k + 64) bytes of dynamic LDS for the lists (37 KB at k = 10, 96 KB at k = 128: two workgroups per CU, then one):
//   dot_chunk_kernel<true>    VGPRs 118   SGPRs 106   LDS 43008 B static   scratch 0   occupancy 3 waves / SIMD (by static LDS)
//   dot_chunk_kernel<false>   VGPRs 74    SGPRs 69    LDS 43008 B static   scratch 0   occupancy 3 waves / SIMD (by static LDS)
//   dot_topk_user_kernel      VGPRs 26    SGPRs 68    LDS 2632 B           scratch 0   occupancy 8 waves / SIMD
// (unchanged by dot_chunk_kernel's CHUNK parameter, whose default instantiations these are; digat_shortlist.inc adds <false, 256>.)

#define DOT_USERS DIGAT_DOT_TOPK_USERS
#define DOT_SUB DIGAT_DOT_TOPK_SUB
#define DOT_KB 32                        // channels per staged K block
#define DOT_LD (DOT_KB + 4)              // row stride of the operand tiles: 36 lr + lq hits 64 different banks, rows stay 16-byte aligned
#define DOT_SLD (DOT_SUB + 4)
#define DOT_NOPOS 0xffffffffu
#define DOT_CAP_MAX (TOPK_MAX_K + DOT_SUB)  // the longest list: three entries per lane of the wave that cuts it

static_assert(DOT_USERS == 64 && DOT_SUB == 64, "dot_chunk_kernel's wave layout is written for 64 x 64 tiles");
static_assert(DIGAT_DOT_TOPK_CHUNK % DOT_SUB == 0, "a chunk is a whole number of sub-tiles");
static_assert(DOT_CAP_MAX == 3 * 64, "dot_cut holds a list in three registers per lane");

struct DotArgs {
    const float* users;
    const float* news;
    const int64_t* pool;
    long G, N, P;
    int d;
    const int64_t* skip;
    int skip_len, k;
    long tiles, chunks;
    float* out;              // digat_dot_scores: [G, P]
    uint2* ws;               // [G][chunks][k]: (score bits, position inside the chunk or DOT_NOPOS)
    float* out_scores;
    int64_t* out_ids;
    int32_t* out_count;
};

struct alignas(16) DotShared {
    float Us[DOT_USERS][DOT_LD];
    float Ns[DOT_SUB][DOT_LD];
    float Ss[DOT_USERS][DOT_SLD];            // the sub-tile's scores [user][position]
    long long id[DOT_SUB];                   // news row of every position of the sub-tile, -1: not an element
    unsigned cnt[DOT_USERS], thr[DOT_USERS];
    unsigned long long keys[4][DOT_CAP_MAX]; // a wave's scratch for the cut of one of its users' lists: (key, ~list index)
};

__device__ __forceinline__ float4 dot_load4(const float* row, int k0, int d, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row) {
        if (vec) {
            if (k0 < d) v = *(const float4*)(row + k0);
        } else {
            if (k0 < d) v.x = row[k0];
            if (k0 + 1 < d) v.y = row[k0 + 1];
            if (k0 + 2 < d) v.z = row[k0 + 2];
            if (k0 + 3 < d) v.w = row[k0 + 3];
        }
    }
    return v;
}

// Ss[u][j] = <users[u0 + u], news[id[j]]> for the 64 x 64 sub-tile (rows beyond G and positions with id -1: zero rows).
// Called by the whole workgroup; ends behind a barrier.
__device__ __forceinline__ void dot_tile(const DotArgs& a, DotShared& s, long u0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;                 // this thread stages rows r0 and r0 + 32, channels c4 .. c4 + 3
    const bool vec = (a.d & 3) == 0 && ((((uintptr_t)a.users) | ((uintptr_t)a.news)) & 15) == 0;
    const float* urow[2];
    const float* nrow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long g = u0 + r0 + 32 * h;
        const long long id = s.id[r0 + 32 * h];
        urow[h] = g < a.G ? a.users + g * a.d : nullptr;
        nrow[h] = id >= 0 ? a.news + id * a.d : nullptr;
    }
    const int ur = (wave >> 1) * 32, nc = (wave & 1) * 32;
    v4f acc[2][2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tu = 0; tu < 2; ++tu) acc[tn][tu] = (v4f){0.f, 0.f, 0.f, 0.f};
    float4 ru[2], rn[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) { ru[h] = dot_load4(urow[h], c4, a.d, vec); rn[h] = dot_load4(nrow[h], c4, a.d, vec); }
    for (int kb = 0; kb < a.d; kb += DOT_KB) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(float4*)&s.Us[r0 + 32 * h][c4] = ru[h];
            *(float4*)&s.Ns[r0 + 32 * h][c4] = rn[h];
        }
        __syncthreads();
        if (kb + DOT_KB < a.d) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ru[h] = dot_load4(urow[h], kb + DOT_KB + c4, a.d, vec);
                rn[h] = dot_load4(nrow[h], kb + DOT_KB + c4, a.d, vec);
            }
        }
#pragma unroll
        for (int ks = 0; ks < DOT_KB / 4; ++ks) {
            if (kb + ks * 4 < a.d) {                              // workgroup-uniform: no k-step wholly beyond d
                const int k = ks * 4 + lq;
                const float n0 = s.Ns[nc + lr][k], n1 = s.Ns[nc + 16 + lr][k];
                const float x0 = s.Us[ur + lr][k], x1 = s.Us[ur + 16 + lr][k];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(n0, x0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(n0, x1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(n1, x0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(n1, x1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D[row = position nc + 16 tn + 4 lq + r][col = user ur + 16 tu + lr]
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tu = 0; tu < 2; ++tu)
            *(float4*)&s.Ss[ur + 16 * tu + lr][nc + 16 * tn + 4 * lq] =
                make_float4(acc[tn][tu][0], acc[tn][tu][1], acc[tn][tu][2], acc[tn][tu][3]);
    __syncthreads();
}

__device__ __forceinline__ long long dot_readlane(long long v, int l) {         // l wave-uniform
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// Of the lanes in `pass`, those whose id occurs in the skip row (whole wave; ids of passing lanes are >= 0, -1 pads the row).  The
// lanes hold the row; whichever is shorter is broadcast entry by entry: the passing ids, or the row.
__device__ __forceinline__ unsigned long long dot_skipped(const int64_t* row, int len, long long id, unsigned long long pass, int lane) {
    long long sk[TOPK_MAX_SKIP / 64];
#pragma unroll
    for (int q = 0; q < TOPK_MAX_SKIP / 64; ++q) sk[q] = lane + 64 * q < len ? (long long)row[lane + 64 * q] : -1ll;
    if (__popcll(pass) > len) {
        bool hit = false;
#pragma unroll
        for (int q = 0; q < TOPK_MAX_SKIP / 64; ++q) {
            const int m = len - 64 * q < 64 ? len - 64 * q : 64;
            for (int l = 0; l < m; ++l) hit = hit || id == dot_readlane(sk[q], l);
        }
        return __ballot(hit) & pass;
    }
    unsigned long long out = 0;
    while (pass) {
        const int b = __ffsll((long long)pass) - 1;
        pass &= pass - 1;
        const long long x = dot_readlane(id, b);
        bool hit = false;
#pragma unroll
        for (int q = 0; q < TOPK_MAX_SKIP / 64; ++q) hit = hit || sk[q] == x;
        if (__ballot(hit)) out |= 1ull << b;
    }
    return out;
}

// What one wave has written to LDS is read back by its other lanes: LDS serves a wave's accesses in order, the compiler must too.
__device__ __forceinline__ void dot_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave, user u of the tile, one position of the sub-tile per lane: append the keys that beat the user's threshold and are not
// skipped to its list (rows of `cap` entries), in position order.  Returns false, and appends nothing, when the list would then hold
// more than `limit` entries.
__device__ __forceinline__ bool dot_append(const DotArgs& a, DotShared& s, uint2* list, int cap, int limit, int u, long g, unsigned sub0,
                                           int lane) {
    const long long id = s.id[lane];
    const float sc = s.Ss[u][lane];
    const unsigned key = id >= 0 ? topk_key(sc) : 0u;
    unsigned long long pass = __ballot(key > s.thr[u]);
    if (pass && a.skip) pass &= ~dot_skipped(a.skip + g * a.skip_len, a.skip_len, id, pass, lane);
    const unsigned np = (unsigned)__popcll(pass), c = s.cnt[u];
    if (np == 0) return true;
    if (c + np > (unsigned)limit) return false;
    if ((pass >> lane) & 1ull)
        list[(unsigned)u * cap + c + (unsigned)__popcll(pass & ((1ull << lane) - 1ull))] = make_uint2(__float_as_uint(sc), sub0 + lane);
    if (lane == 0) s.cnt[u] = c + np;
    dot_wave_sync();
    return true;
}

struct DotSlotLoad {
    const uint2* e;
    __device__ __forceinline__ unsigned key(long i) const {
        const uint2 v = e[i];
        return v.y == DOT_NOPOS ? 0u : topk_key(__uint_as_float(v.x));
    }
};

// One wave: user u's list cut back to its k best, in place and in list (= position) order; the threshold becomes the smallest key
// kept.  Every entry's rank — the entries that order before it: a larger key, or the same key earlier in the list — is counted
// against the (key, ~index) words broadcast from LDS one by one: n ceil(n / 64) compares per lane, no barrier, the four waves cut
// in parallel.
__device__ __forceinline__ void dot_cut(DotShared& s, uint2* list, int u, int k, int wave, int lane) {
    dot_wave_sync();
    const int n = (int)s.cnt[u];
    if (n <= k) return;
    unsigned long long* keys = s.keys[wave];
    uint2 e[3];
    unsigned long long mine[3];                  // (key, ~list index): a larger one orders first, no two are equal
    int rank[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int i = t * 64 + lane;
        e[t] = i < n ? list[i] : make_uint2(0u, 0u);
        mine[t] = i < n ? ((unsigned long long)topk_key(__uint_as_float(e[t].x)) << 32) | (unsigned)~i : 0ull;
        rank[t] = 0;
        if (i < n) keys[i] = mine[t];
    }
    dot_wave_sync();
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const unsigned long long kj = keys[j];
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (t * 64 < n) rank[t] += kj > mine[t];
    }
    int base = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const bool keep = t * 64 + lane < n && rank[t] < k;
        const unsigned long long b = __ballot(keep);
        if (keep) list[base + __popcll(b & ((1ull << lane) - 1ull))] = e[t];
        if (keep && rank[t] == k - 1) s.thr[u] = (unsigned)(mine[t] >> 32);
        base += __popcll(b);
    }
    if (lane == 0) s.cnt[u] = (unsigned)k;
    dot_wave_sync();
}

// CHUNK: the pool positions one workgroup walks — DIGAT_DOT_TOPK_CHUNK for the entries of this file; digat_shortlist.inc stores a slab's
// scores in shorter chunks (more workgroups for few users), the same sub-tiles through the same dot_tile: the same bits.
// The walk itself, shared with digat_qdot.inc's kernel: `product(u0)` leaves the sub-tile's scores in s.Ss behind a barrier (dot_tile here).
template <bool FUSED, int CHUNK, class Tile>
__device__ __forceinline__ void dot_chunk_walk(const DotArgs& a, DotShared& s, uint2* dot_lists, const Tile& product) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long tile = blockIdx.x % a.tiles, chunk = blockIdx.x / a.tiles;
    static_assert(CHUNK % DOT_SUB == 0, "a chunk is a whole number of sub-tiles");
    const long u0 = tile * DOT_USERS, p0 = chunk * CHUNK;
    const long pend = p0 + CHUNK < a.P ? p0 + CHUNK : a.P;
    const int cap = a.k + DOT_SUB;
    const int soft = 2 * a.k > 32 ? (2 * a.k < cap ? 2 * a.k : cap) : 32;      // cut early while that is cheap: a tighter threshold sooner
    if (FUSED) {
        if (tid < DOT_USERS) { s.cnt[tid] = 0; s.thr[tid] = 0; }
    }
    for (long q0 = p0; q0 < pend; q0 += DOT_SUB) {
        if (tid < DOT_SUB) {
            const long p = q0 + tid;
            long long id = -1;
            if (p < pend) {
                id = a.pool ? (long long)a.pool[p] : (long long)p;
                if (id < 0 || id >= a.N) id = -1;
            }
            s.id[tid] = id;
        }
        __syncthreads();
        product(u0);
        if (!FUSED) {
            for (int i = wave; i < DOT_USERS; i += 4) {
                const long g = u0 + i, p = q0 + lane;
                if (g < a.G && p < pend) a.out[g * a.P + p] = s.Ss[i][lane];
            }
        } else {
            const unsigned sub0 = (unsigned)(q0 - p0);
            const long long id = s.id[lane];
            unsigned some = 0;                                    // bit i: user i of this wave has a key above its threshold
#pragma unroll
            for (int i = 0; i < DOT_USERS / 4; ++i) {
                const int u = wave * (DOT_USERS / 4) + i;
                const unsigned key = id >= 0 ? topk_key(s.Ss[u][lane]) : 0u;
                if (__ballot(key > s.thr[u]) != 0ull && u0 + u < a.G) some |= 1u << i;
            }
            while (some) {                                        // this wave's users: nobody else touches their lists
                const int i = __ffs((int)some) - 1;
                some &= some - 1;
                const int u = wave * (DOT_USERS / 4) + i;
                if (!dot_append(a, s, dot_lists, cap, soft, u, u0 + u, sub0, lane)) {
                    dot_cut(s, dot_lists + (size_t)u * cap, u, a.k, wave, lane);
                    dot_append(a, s, dot_lists, cap, cap, u, u0 + u, sub0, lane);     // k + at most 64: fits
                }
            }
        }
        __syncthreads();
    }
    if (FUSED) {
        for (int i = 0; i < DOT_USERS / 4; ++i) {
            const int u = wave * (DOT_USERS / 4) + i;
            dot_cut(s, dot_lists + (size_t)u * cap, u, a.k, wave, lane);
        }
        __syncthreads();
        for (int x = tid; x < DOT_USERS * a.k; x += 256) {
            const int u = x / a.k, i = x - u * a.k;
            const long g = u0 + u;
            if (g < a.G)
                a.ws[(g * a.chunks + chunk) * a.k + i] = (unsigned)i < s.cnt[u] ? dot_lists[(size_t)u * cap + i] : make_uint2(0u, DOT_NOPOS);
        }
    }
}

template <bool FUSED, int CHUNK = DIGAT_DOT_TOPK_CHUNK>
__global__ void __launch_bounds__(256) dot_chunk_kernel(const DotArgs a) {
    __shared__ DotShared s;
    extern __shared__ uint2 dot_lists[];            // [DOT_USERS][k + DOT_SUB]
    dot_chunk_walk<FUSED, CHUNK>(a, s, dot_lists, [&](long u0) { dot_tile(a, s, u0); });
}

__global__ void __launch_bounds__(256) dot_topk_user_kernel(const DotArgs a) {
    __shared__ TopkShared sh;
    const long g = blockIdx.x;
    const uint2* slots = a.ws + g * a.chunks * a.k;
    const DotSlotLoad ld{slots};
    topk_select(ld, a.chunks * a.k, a.k, sh);
    topk_finish(sh, a.k, a.out_scores + g * a.k, a.out_ids + g * a.k, a.out_count + g, [&](long long slot, float& score, int64_t& id) {
        const uint2 e = slots[slot];                              // slots lie in position order
        long pos = (slot / a.k) * DIGAT_DOT_TOPK_CHUNK + (long)e.y;
        if (pos >= a.P) pos = a.P - 1;                            // cannot happen with level 1's slots: stay inside the pool
        score = __uint_as_float(e.x);
        id = a.pool ? a.pool[pos] : (int64_t)pos;
    });
}

static long dot_chunks(long pool) { return (pool + DIGAT_DOT_TOPK_CHUNK - 1) / DIGAT_DOT_TOPK_CHUNK; }
static long dot_tiles(long users) { return (users + DOT_USERS - 1) / DOT_USERS; }

static int dot_check(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d) {
    if (!users || !news || G < 0 || N < 0 || P < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (!pool && P != N) return DIGAT_ERR_ARG;
    if ((double)dot_tiles((long)G) * (double)dot_chunks((long)P) > 2147483647.0) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

extern "C" {

size_t digat_dot_topk_workspace_bytes(int64_t users, int64_t pool, int k) {
    if (users < 0 || pool < 0 || k < 1) return 0;
    return (size_t)users * (size_t)dot_chunks((long)pool) * (size_t)k * sizeof(uint2);
}

int digat_dot_topk(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t* skip,
                   int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes,
                   void* stream) {
    if (!out_scores || !out_ids || !out_count) return DIGAT_ERR_ARG;
    const size_t need = digat_dot_topk_workspace_bytes(G, P, k);
    const int rc = topk_check_args(k, skip, skip_len, dot_check(users, news, pool, G, N, P, d), need > 0, workspace);
    if (rc != DIGAT_OK) return rc;
    if (workspace_bytes < need) return DIGAT_ERR_WORKSPACE;
    if (G == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    DotArgs a{users, news, pool, (long)G, (long)N, (long)P, d, skip, skip_len, k, dot_tiles((long)G), dot_chunks((long)P), nullptr,
              (uint2*)workspace, out_scores, out_ids, out_count};
    if (P > 0) {
        const size_t lds = (size_t)DOT_USERS * (size_t)(k + DOT_SUB) * sizeof(uint2);
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)dot_chunk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess) return DIGAT_ERR_LAUNCH;
        hipLaunchKernelGGL(dot_chunk_kernel<true>, dim3((unsigned)(a.tiles * a.chunks)), dim3(256), lds, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dot_topk_user_kernel, dim3((unsigned)G), dim3(256), 0, st, a);      // P == 0: no slot, every count 0
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_dot_scores(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, float* out,
                     void* stream) {
    if (!out) return DIGAT_ERR_ARG;
    const int rc = dot_check(users, news, pool, G, N, P, d);
    if (rc != DIGAT_OK) return rc;
    if (G == 0 || P == 0) return DIGAT_OK;
    DotArgs a{users, news, pool, (long)G, (long)N, (long)P, d, nullptr, 0, 0, dot_tiles((long)G), dot_chunks((long)P), out,
              nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(dot_chunk_kernel<false>, dim3((unsigned)(a.tiles * a.chunks)), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
