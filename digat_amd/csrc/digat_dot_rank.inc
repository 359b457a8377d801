// digat_dot_rank.inc — retrieval evaluation: where in a user's whole ordered pool a given target stands (its rank), without the
// [G, P] score matrix ever reaching memory (evaluate.dot_rank, nrms.retrieval_metrics).  Included in digat_kernels.hip behind
// digat_dot_topk.inc, whose elements, order and product these are: dot_tile (every score the same bits wherever it is computed),
// topk_key, dot_skipped, DotArgs / DotShared.  rank(g, q) = the elements of user g that order before pool position q: a larger key,
// or the same key at a smaller position; -1 when q is no element of g (outside [0, P), an id outside [0, N), or skipped).
//
// Three launches, all sized by what the host knows (target_start is never read on the host):
//   dot_rank_init_kernel    one thread per target: rank -1, score NaN, key 0 — so that every output byte is written whatever
//                           target_start says.
//   dot_rank_target_kernel  one workgroup per tile of 64 users: the tile's targets (a contiguous range of target_pos), 64 at a
//                           time, take the place of a sub-tile's pool positions, and dot_tile gives every target's score against
//                           all 64 users, of which its own user's is kept.  A per-lane fmaf loop would be cheaper and the MFMA is
//                           documented as that chain; going through dot_tile makes the bits equal by construction — the padded
//                           tail and the sign of a zero included — and costs one sub-tile product per 64 targets where the
//                           counting pass does P / 64 per tile.  A target that is an element gets its key in the workspace, its
//                           score bits in out_scores and rank 0.
//   dot_rank_count_kernel   one workgroup per (tile of 64 users, chunk of DIGAT_DOT_TOPK_CHUNK positions), dot_chunk_kernel's
//                           grid; a tile without a target returns at once.  The tile's (key, position relative to the chunk) pairs
//                           are staged in LDS (RANK_CAP at a time; a tile with more re-stages them per sub-tile).  Per sub-tile:
//                           dot_tile, then wave w owns users 16 w .. + 16, one position per lane: per target of the user one ballot
//                           over "element and orders before", its popcount added to the target's partial count in LDS (one wave
//                           owns a user, so no atomics there).  The skip row is consulted only for positions that do not order
//                           behind the user's worst target AND hit a per-user Bloom filter of the row (2048 bits, two hashes,
//                           built once per workgroup: 0.2 % false positives at 50 entries, 5 % at 256), so dot_skipped — which
//                           fetches the row — runs, by that rate, for about one (user, sub-tile) pair in ten.  A ranked target is a
//                           typical element, not one of the k best, so the threshold alone prunes about half the lanes, not nearly
//                           all of them as in dot_chunk_kernel.  The chunk's partial counts go to out_rank by integer atomicAdd:
//                           sums of integers, the same in any order.
//
// target_start is clamped into [0, T] and made non-decreasing before use (rank_tile_starts): a malformed array gives wrong
// numbers, never a read or write outside the arrays.
//
// Measured on an MI355X at G = 4 096, P = 65 237, d = 400, 50-entry skip rows: 4.3 ms at one target per user, 5.8 ms at five
// (digat_dot_scores alone: 2.9 ms); at G = 64 — one tile, 32 workgroups — 1.0 ms (DESIGN section 8).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   dot_rank_init_kernel           VGPRs 7            SGPRs 14    LDS 0 B       scratch 0   occupancy 8 waves / SIMD
//   dot_rank_target_kernel         VGPRs 76 + 16 acc  SGPRs 82    LDS 43528 B   scratch 0   occupancy 3 waves / SIMD (by LDS)
//   dot_rank_count_kernel<false>   VGPRs 86 + 16 acc  SGPRs 86    LDS 53256 B   scratch 0   occupancy 3 waves / SIMD (by LDS)
//   dot_rank_count_kernel<true>    VGPRs 93 + 16 acc  SGPRs 106   LDS 69384 B   scratch 0   occupancy 2 waves / SIMD (by LDS)
//   (<true>, the variant with skip rows: four SGPRs are kept in VGPR lanes, nothing goes to scratch; its Bloom filters are the
//   16 KB that cost the third workgroup per CU.)

#define RANK_CAP 768                     // targets of a tile staged in LDS at a time: without skip rows three workgroups share a CU
#define RANK_BLOOM_WORDS 64              // 2048 bits per user

struct RankArgs {
    DotArgs dot;                         // users, news, pool, G, N, P, d, skip, skip_len, tiles, chunks: what dot_tile and dot_skipped read
    const int64_t* target_pos;           // [T] pool positions
    const int64_t* target_start;         // [G + 1]
    long T;
    int32_t* out_rank;                   // [T]
    float* out_scores;                   // [T]
    unsigned* key;                       // workspace [T]: topk_key of the target's score, 0: no element
};

template <bool SKIP>
struct RankShared {
    long ts[DOT_USERS + 1];              // the tile's users' target ranges, inside [0, T] and non-decreasing
    unsigned lo[DOT_USERS];              // the smallest key among a user's ranked targets, ~0: it has none
    uint2 tgt[RANK_CAP];                 // (key, position relative to the chunk, held inside [0, CHUNK])
    int acc[RANK_CAP];
    unsigned bloom[SKIP ? DOT_USERS : 1][RANK_BLOOM_WORDS];
};

// ts[i] = where user u0 + i's targets begin (i = 64: where the tile's end), whatever target_start holds.  Whole workgroup; ends
// behind a barrier.
__device__ __forceinline__ void rank_tile_starts(const RankArgs& r, long* ts, long u0) {
    const int tid = threadIdx.x;
    if (tid <= DOT_USERS) {
        long g = u0 + tid;
        if (g > r.dot.G) g = r.dot.G;
        long v = r.target_start[g];
        ts[tid] = v < 0 ? 0 : (v > r.T ? r.T : v);
    }
    __syncthreads();
    if (tid == 0)
        for (int i = 1; i <= DOT_USERS; ++i)
            if (ts[i] < ts[i - 1]) ts[i] = ts[i - 1];
    __syncthreads();
}

// The user of the tile that owns target t, ts[0] <= t < ts[64]: the first whose range ends beyond t.
__device__ __forceinline__ int rank_user(const long* ts, long t) {
    int lo = 0, hi = DOT_USERS - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ts[mid + 1] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned rank_hash(long long id, unsigned mul) {
    const unsigned x = (unsigned)(unsigned long long)id ^ (unsigned)((unsigned long long)id >> 32);
    return (x * mul) >> 21;              // 11 bits: one of the 2048
}
#define RANK_HASH_A 0x9E3779B1u
#define RANK_HASH_B 0x85EBCA6Bu

__global__ void __launch_bounds__(256) dot_rank_init_kernel(const RankArgs r) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < r.T) {
        r.out_rank[t] = -1;
        r.out_scores[t] = __uint_as_float(0x7fc00000u);
        r.key[t] = 0u;
    }
}

__global__ void __launch_bounds__(256) dot_rank_target_kernel(const RankArgs r) {
    __shared__ DotShared s;
    __shared__ long ts[DOT_USERS + 1];
    const DotArgs& a = r.dot;
    const int tid = threadIdx.x;
    const long u0 = (long)blockIdx.x * DOT_USERS;
    rank_tile_starts(r, ts, u0);
    const long tb = ts[0], te = ts[DOT_USERS];
    for (long b0 = tb; b0 < te; b0 += DOT_SUB) {
        const long t = b0 + tid;
        long long id = -1;
        if (tid < DOT_SUB) {
            if (t < te) {
                const long pos = r.target_pos[t];
                if (pos >= 0 && pos < a.P) {
                    id = a.pool ? (long long)a.pool[pos] : (long long)pos;
                    if (id < 0 || id >= a.N) id = -1;
                }
            }
            s.id[tid] = id;
        }
        __syncthreads();
        dot_tile(a, s, u0);
        if (tid < DOT_SUB && t < te) {
            const int u = rank_user(ts, t);
            bool elem = id >= 0;
            if (elem && a.skip) {
                const int64_t* row = a.skip + (u0 + u) * a.skip_len;
                for (int q = 0; q < a.skip_len; ++q) elem = elem && (long long)row[q] != id;
            }
            if (elem) {
                const float sc = s.Ss[u][tid];
                r.key[t] = topk_key(sc);
                r.out_scores[t] = sc;
                r.out_rank[t] = 0;
            }
        }
        __syncthreads();
    }
}

template <bool SKIP>
__global__ void __launch_bounds__(256) dot_rank_count_kernel(const RankArgs r) {
    __shared__ DotShared s;
    __shared__ RankShared<SKIP> h;
    const DotArgs& a = r.dot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long tile = blockIdx.x % a.tiles, chunk = blockIdx.x / a.tiles;
    const long u0 = tile * DOT_USERS, p0 = chunk * DIGAT_DOT_TOPK_CHUNK;
    const long pend = p0 + DIGAT_DOT_TOPK_CHUNK < a.P ? p0 + DIGAT_DOT_TOPK_CHUNK : a.P;
    rank_tile_starts(r, h.ts, u0);
    const long tb = h.ts[0], te = h.ts[DOT_USERS];
    if (te == tb) return;                                         // nobody of this tile has a target: no product
    if (tid < DOT_USERS) h.lo[tid] = ~0u;
    if (SKIP)
        for (int x = tid; x < DOT_USERS * RANK_BLOOM_WORDS; x += 256) h.bloom[x / RANK_BLOOM_WORDS][x % RANK_BLOOM_WORDS] = 0u;
    __syncthreads();
    for (long t = tb + tid; t < te; t += 256) {
        const unsigned k = r.key[t];
        if (k) atomicMin(&h.lo[rank_user(h.ts, t)], k);
    }
    if (SKIP)
        for (int x = tid; x < DOT_USERS * a.skip_len; x += 256) {
            const int u = x / a.skip_len;
            if (u0 + u < a.G) {
                const long long id = (long long)a.skip[(u0 + u) * a.skip_len + (x - u * a.skip_len)];
                const unsigned ha = rank_hash(id, RANK_HASH_A), hb = rank_hash(id, RANK_HASH_B);
                atomicOr(&h.bloom[u][ha >> 5], 1u << (ha & 31));
                atomicOr(&h.bloom[u][hb >> 5], 1u << (hb & 31));
            }
        }
    const bool once = te - tb <= RANK_CAP;                        // the usual case: the tile's targets are staged once for the chunk
    // the batch of targets [b0, b0 + n) into LDS, their partial counts zeroed
    auto stage = [&](long b0, int n) {
        for (int j = tid; j < n; j += 256) {
            const long pos = r.target_pos[b0 + j];                // ties before the chunk lose to it, ties behind it win
            h.tgt[j] = make_uint2(r.key[b0 + j], pos <= p0 ? 0u : (pos - p0 > DIGAT_DOT_TOPK_CHUNK ? (unsigned)DIGAT_DOT_TOPK_CHUNK
                                                                                                    : (unsigned)(pos - p0)));
            h.acc[j] = 0;
        }
    };
    auto flush = [&](long b0, int n) {
        for (int j = tid; j < n; j += 256)
            if (h.acc[j]) atomicAdd(&r.out_rank[b0 + j], h.acc[j]);
    };
    if (once) stage(tb, (int)(te - tb));
    __syncthreads();
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
        dot_tile(a, s, u0);
        const long long id = s.id[lane];
        const unsigned rel = (unsigned)(q0 - p0) + (unsigned)lane;
        const unsigned ha = rank_hash(id, RANK_HASH_A), hb = rank_hash(id, RANK_HASH_B);
        for (long b0 = tb; b0 < te; b0 += RANK_CAP) {
            const int n = (int)(te - b0 < RANK_CAP ? te - b0 : RANK_CAP);
            if (!once) {
                stage(b0, n);
                __syncthreads();
            }
            for (int i = 0; i < DOT_USERS / 4; ++i) {             // this wave's users: nobody else touches their targets' counts
                const int u = wave * (DOT_USERS / 4) + i;
                const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)h.lo[u]);
                if (lo == ~0u) continue;
                const long jb = (h.ts[u] > b0 ? h.ts[u] : b0) - b0, je = (h.ts[u + 1] < b0 + n ? h.ts[u + 1] : b0 + n) - b0;
                const int j0 = __builtin_amdgcn_readfirstlane((int)jb), j1 = __builtin_amdgcn_readfirstlane((int)je);
                if (j0 >= j1) continue;
                const unsigned key = id >= 0 ? topk_key(s.Ss[u][lane]) : 0u;
                bool in = key >= lo;                              // lo >= 1: an element by its id that does not order behind every target
                if (SKIP) {
                    const bool maybe = in && ((h.bloom[u][ha >> 5] >> (ha & 31)) & (h.bloom[u][hb >> 5] >> (hb & 31)) & 1u);
                    const unsigned long long pass = __ballot(maybe);
                    if (pass) {
                        const unsigned long long out = dot_skipped(a.skip + (u0 + u) * a.skip_len, a.skip_len, id, pass, lane);
                        if ((out >> lane) & 1ull) in = false;
                    }
                }
                for (int j = j0; j < j1; ++j) {
                    const uint2 tg = h.tgt[j];
                    const unsigned tk = (unsigned)__builtin_amdgcn_readfirstlane((int)tg.x);
                    const unsigned tr = (unsigned)__builtin_amdgcn_readfirstlane((int)tg.y);
                    if (tk == 0u) continue;                       // no element: its rank stays -1
                    const int c = __popcll(__ballot(in && (key > tk || (key == tk && rel < tr))));
                    if (lane == 0 && c) h.acc[j] += c;
                }
            }
            if (!once) {
                __syncthreads();
                flush(b0, n);
                __syncthreads();
            }
        }
        __syncthreads();
    }
    if (once) flush(tb, (int)(te - tb));
}

extern "C" {

size_t digat_dot_rank_workspace_bytes(int64_t users, int64_t pool, int64_t targets) {
    if (users < 0 || pool < 0 || targets < 0) return 0;
    return align_up((size_t)targets * sizeof(unsigned), 256);
}

int digat_dot_rank(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t* skip,
                   int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, int32_t* out_rank, float* out_scores,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!target_pos || !target_start || !out_rank || !out_scores || T < 0) return DIGAT_ERR_ARG;
    const size_t need = digat_dot_rank_workspace_bytes(G, P, T);
    int rc = topk_check_args(1, skip, skip_len, dot_check(users, news, pool, G, N, P, d), need > 0, workspace);
    if (rc != DIGAT_OK) return rc;
    if (T > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < need) return DIGAT_ERR_WORKSPACE;
    if (G == 0 || T == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    RankArgs r{{users, news, pool, (long)G, (long)N, (long)P, d, skip, skip_len, 0, dot_tiles((long)G), dot_chunks((long)P), nullptr, nullptr,
                nullptr, nullptr, nullptr},
               target_pos, target_start, (long)T, out_rank, out_scores, (unsigned*)workspace};
    hipLaunchKernelGGL(dot_rank_init_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, r);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(dot_rank_target_kernel, dim3((unsigned)r.dot.tiles), dim3(256), 0, st, r);
    DIGAT_CHECK_LAUNCH();
    if (P > 0) {                                                  // P == 0: no position is an element, every rank stays -1
        const dim3 grid((unsigned)(r.dot.tiles * r.dot.chunks));
        if (skip) hipLaunchKernelGGL(dot_rank_count_kernel<true>, grid, dim3(256), 0, st, r);
        else hipLaunchKernelGGL(dot_rank_count_kernel<false>, grid, dim3(256), 0, st, r);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

}  // extern "C"
