// digat_capped.inc — exposure-capped top-k: the one selection stage that works on the BATCH of lists, not on a list (the stage behind
// util.recommend(exposure_cap=) / nrms.recommend(exposure_cap=): "the k best of every reader, no story in more than c lists").  It
// is deferred acceptance — stable matching with a quota k per list and a capacity cap[id] per news — in its round-wise form
// (evaluate.capped_select_host): lists prefer entries by topk_key(score), items prefer pairs by topk_key(priority), both orders
// strict through their tie rules, so the list-optimal stable assignment is unique and any schedule of proposals reaches it.
// Included at the end of digat_kernels.hip, behind digat_topk.inc (topk_key), digat_shortlist.inc (short_bitonic) and digat_mmr.inc
// (sel_count, sel_fill).  Integer and comparison work only; the one atomic is the integer add on the round's rejection counter.
//
// The state of a call, per pair (g, slot), lives in the workspace (cap_carve): the item word, the list's rank -> slot map, and two
// bytes, rejected and demand.
//   cap_prepare_kernel    one workgroup of 256 threads per list: the element test, the item word (id << 32) | ~topk_key(priority) of
//                         every pair (CAP_NO_ELEMENT for a non-element), rejected = non-element, demand = 0; then short_bitonic over
//                         the (topk_key(score), ~slot) words in LDS and the list's order: rank r -> slot, -1 behind the elements.
//                         One stable sort of the item words — the caller's: torch.sort, as list_softmax sorts its row keys — yields
//                         the inverted index in item order: id ascending, priority key descending, ties in flat order, which is g
//                         ascending then SLOT ascending.  (The words stay in slot space for that tie rule: a list that names one id
//                         twice at equal priorities and different scores has its two pairs in slot order there, not in rank order.)
//   cap_list_kernel<W,P>  one workgroup per list, rank r held by thread r / P as its entry r % P: <1, 2> for M <= 128 (one wave, no
//                         barrier, no LDS traffic), <4, 4> up to 1024 (one barrier: the waves' alive counts) — cal_kernel's two shapes.
//                         A rank is alive when it holds an element that is not rejected; ballots give every rank the number of alive
//                         ranks in front of it, and the first k alive ranks are the list's demand.  Without emit: the demand bytes
//                         of the row.  With emit: the outputs (ids, score bits, slots in the list's order, the count, the fill).
//   cap_item_kernel       one wave per segment that can bind (more pairs than capacity; the caller lists them), four per
//                         workgroup: walks the segment's pairs in item order 64 at a time with a running count of demanded ones
//                         from ballots; from the pair behind the cap-th demanded one on (cap 0: from the start) every pair of the
//                         live part becomes rejected, and the live length is cut there, so later rounds stop where the segment
//                         was cut — inside the live part nothing is rejected, so the round's new rejections are live - cut, added to
//                         counter[round] by lane 0.  Segments are disjoint sets of pairs: no two waves write one byte.
// A round is one cap_list_kernel and one cap_item_kernel, each run to completion: no cooperative launch, no grid-wide wait, no
// workgroup that waits on another.  Rejections are permanent and a round past the fixed point changes nothing, so the host enqueues
// blocks of rounds and reads a block's counters behind it (evaluate.capped_select).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   cap_prepare_kernel      256 threads   VGPRs 24   SGPRs 48   LDS 8192 B   scratch 0   occupancy 8 waves / SIMD
//   cap_list_kernel<1, 2>    64 threads   VGPRs 16   SGPRs 50   LDS 0 B      scratch 0   occupancy 8 waves / SIMD
//   cap_list_kernel<4, 4>   256 threads   VGPRs 24   SGPRs 56   LDS 16 B     scratch 0   occupancy 8 waves / SIMD
//   cap_item_kernel         256 threads   VGPRs 18   SGPRs 29   LDS 0 B      scratch 0   occupancy 8 waves / SIMD

#define CAP_MAX_M DIGAT_CAPPED_MAX_LIST
#define CAP_NO_ELEMENT 0x7fffffffffffffffll      // the item word of a non-element: behind every news in the sort
#define CAP_KEY_NEG_INF 0x007fffffu              // topk_key(-inf); a NaN's key is 1: an element's score key lies above both

static_assert(CAP_MAX_M == 1024 && CAP_MAX_M == SHORT_MAX_K, "cap_list_kernel<4, 4> holds four ranks per thread; short_bitonic orders at most SHORT_MAX_K words");

struct CapState {
    long long* words;            // [G M] item words, slot space — the start of the workspace: the caller sorts them
    int16_t* order;              // [G M] rank -> slot of every list, -1 behind its elements
    unsigned char* rejected;     // [G M] slot space
    unsigned char* demand;       // [G M] slot space
};

static size_t cap_round256(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t cap_state_bytes(long G, int M) {
    const size_t n = (size_t)G * (size_t)M;
    return cap_round256(n * 8) + cap_round256(n * 2) + 2 * cap_round256(n);
}

static CapState cap_carve(void* workspace, long G, int M) {
    const size_t n = (size_t)G * (size_t)M;
    unsigned char* p = (unsigned char*)workspace;
    CapState s;
    s.words = (long long*)p;
    p += cap_round256(n * 8);
    s.order = (int16_t*)p;
    p += cap_round256(n * 2);
    s.rejected = p;
    p += cap_round256(n);
    s.demand = p;
    return s;
}

struct CapPrepArgs {
    const int64_t* ids;
    const float* scores;
    const float* priority;       // NULL: the scores
    const int32_t* count;
    int M;
    long P;
    CapState st;
};

__global__ void __launch_bounds__(256) cap_prepare_kernel(const CapPrepArgs a) {
    __shared__ unsigned long long w[CAP_MAX_M];      // (score key, ~slot): a larger word orders first; 0: no element
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = sel_count(a.count, g, a.M);
    int n2 = 2;
    while (n2 < a.M) n2 <<= 1;
    for (int j = tid; j < n2; j += 256) {
        unsigned long long lw = 0ull;
        if (j < a.M) {
            long long iw = CAP_NO_ELEMENT;
            if (j < cnt) {
                const long long id = (long long)a.ids[g * a.M + j];
                const float s = a.scores[g * a.M + j];
                const unsigned ks = topk_key(s), kp = a.priority ? topk_key(a.priority[g * a.M + j]) : ks;
                if (id >= 0 && id < a.P && ks > CAP_KEY_NEG_INF && kp != 1u) {      // neither NaN nor -inf; the priority no NaN
                    iw = (id << 32) | (long long)(unsigned)~kp;
                    lw = ((unsigned long long)ks << 32) | (unsigned)~j;
                }
            }
            a.st.words[g * a.M + j] = iw;
            a.st.rejected[g * a.M + j] = lw == 0ull;
            a.st.demand[g * a.M + j] = 0;
        }
        w[j] = lw;
    }
    __syncthreads();
    short_bitonic(w, n2, [](unsigned long long x, unsigned long long y) { return x > y; });
    for (int r = tid; r < a.M; r += 256) a.st.order[g * a.M + r] = w[r] ? (int16_t)(~(unsigned)w[r] & (CAP_MAX_M - 1)) : (int16_t)-1;
}

struct CapListArgs {
    CapState st;
    int M, k, emit;
    const int64_t* ids;          // the four below and the outputs: with emit only
    const float* scores;
    int64_t* out_ids;
    float* out_scores;
    int32_t* out_count;
    int32_t* out_slots;
};

template <int WAVES, int PPL>
__global__ void __launch_bounds__(64 * WAVES) cap_list_kernel(const CapListArgs a) {
    __shared__ int wave_alive[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const long row = g * a.M;

    int slot[PPL];
    bool alive[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
        const int r = tid * PPL + h;
        slot[h] = r < a.M ? (int)a.st.order[row + r] : -1;
        alive[h] = slot[h] >= 0 && slot[h] < a.M && a.st.rejected[row + slot[h]] == 0;
    }
    // alive ranks in front of this thread's first: the lower lanes' (ballots), then the lower waves'
    const unsigned long long below = (1ull << lane) - 1ull;
    int before = 0, total = 0;
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
        const unsigned long long b = __ballot(alive[h]);
        before += __popcll(b & below);
        total += __popcll(b);
    }
    if (WAVES > 1) {
        if (lane == 0) wave_alive[wave] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) {
            const int t = wave_alive[v];
            before += v < wave ? t : 0;
            total += t;
        }
    }
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
        const bool wanted = alive[h] && before < a.k;          // the first k alive ranks: the list's demand
        if (!a.emit) {
            if (slot[h] >= 0 && slot[h] < a.M) a.st.demand[row + slot[h]] = wanted;
        } else if (wanted) {
            a.out_ids[g * a.k + before] = a.ids[row + slot[h]];
            a.out_scores[g * a.k + before] = a.scores[row + slot[h]];
            a.out_slots[g * a.k + before] = slot[h];
        }
        before += alive[h];
    }
    if (a.emit) {
        const int held = total < a.k ? total : a.k;
        sel_fill(a.out_scores, a.out_ids, g, a.k, held, tid, 64 * WAVES);
        for (int x = held + tid; x < a.k; x += 64 * WAVES) a.out_slots[g * a.k + x] = -1;
        if (tid == 0) a.out_count[g] = held;
    }
}

struct CapItemArgs {
    const int32_t* perm;         // [G M] the pairs (g M + slot) in item order
    const int32_t* seg_begin;    // [n_seg] where a binding-capable segment starts in perm
    const int32_t* seg_cap;      // [n_seg] its news' capacity
    int32_t* seg_live;           // [n_seg] its live length: every pair behind it is rejected
    long n_seg;
    long pairs;                  // G M
    CapState st;
    int32_t* counter;            // the round's
};

__global__ void __launch_bounds__(256) cap_item_kernel(const CapItemArgs a) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.n_seg) return;                        // a whole wave
    const long begin = a.seg_begin[s];
    const int cap = a.seg_cap[s];
    int live = a.seg_live[s];
    if (begin < 0 || live < 0 || begin + live > a.pairs) return;     // a malformed segment table: nothing is read or written
    const unsigned long long below = (1ull << lane) - 1ull;
    int cut = cap > 0 ? live : 0;
    int seen = 0;
    for (int base = 0; base < live && cap > 0; base += 64) {
        const int i = base + lane;
        bool d = false;
        if (i < live) {
            const unsigned f = (unsigned)a.perm[begin + i];
            d = (long)f < a.pairs && a.st.demand[f] != 0;
        }
        const unsigned long long b = __ballot(d);
        const int c = __popcll(b);
        if (seen + c >= cap) {                       // the cap-th demanded pair stands in this chunk: behind it the segment is cut
            const unsigned long long hit = __ballot(d && __popcll(b & below) == cap - seen - 1);
            cut = base + __ffsll((long long)hit);
            break;
        }
        seen += c;
    }
    for (int i = cut + lane; i < live; i += 64) {
        const unsigned f = (unsigned)a.perm[begin + i];
        if ((long)f < a.pairs) a.st.rejected[f] = 1;
    }
    if (lane == 0 && cut < live) {
        a.seg_live[s] = cut;
        atomicAdd(a.counter, live - cut);
    }
}

static void cap_launch_list(const CapListArgs& a, long G, hipStream_t st) {
    if (a.M <= 128)
        hipLaunchKernelGGL((cap_list_kernel<1, 2>), dim3((unsigned)G), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((cap_list_kernel<4, 4>), dim3((unsigned)G), dim3(256), 0, st, a);
}

static int cap_check_lists(int64_t G, int M, const void* workspace, size_t workspace_bytes) {
    if (G < 0 || ((uintptr_t)workspace & 7)) return DIGAT_ERR_ARG;
    if (M < 1 || M > CAP_MAX_M || G > 0x7fffffffL || G * (int64_t)M > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (G > 0 && !workspace) return DIGAT_ERR_ARG;
    if (G > 0 && workspace_bytes < cap_state_bytes((long)G, M)) return DIGAT_ERR_WORKSPACE;
    return DIGAT_OK;
}

extern "C" {

size_t digat_capped_select_workspace_bytes(int64_t lists, int m) {
    if (lists <= 0 || m < 1 || m > CAP_MAX_M) return 0;
    return cap_state_bytes((long)lists, m);
}

int digat_capped_prepare(const int64_t* ids, const float* scores, const float* priority, const int32_t* count, int64_t G, int M, int64_t P,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!ids || !scores || P < 0) return DIGAT_ERR_ARG;
    const int bad = cap_check_lists(G, M, workspace, workspace_bytes);
    if (bad) return bad;
    if (P > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    CapPrepArgs a{ids, scores, priority, count, M, (long)P, cap_carve(workspace, (long)G, M)};
    hipLaunchKernelGGL(cap_prepare_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_capped_rounds(int64_t G, int M, int k, const int32_t* perm, const int32_t* seg_begin, const int32_t* seg_cap, int32_t* seg_live,
                        int64_t n_seg, int32_t* counter, int rounds, void* workspace, size_t workspace_bytes, void* stream) {
    if (!counter || n_seg < 0 || rounds < 0 || (n_seg > 0 && (!perm || !seg_begin || !seg_cap || !seg_live))) return DIGAT_ERR_ARG;
    const int bad = cap_check_lists(G, M, workspace, workspace_bytes);
    if (bad) return bad;
    if (k < 1 || k > TOPK_MAX_K || n_seg > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    const CapState st = cap_carve(workspace, (long)G, M);
    CapListArgs la{st, M, k, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int r = 0; r < rounds; ++r) {
        cap_launch_list(la, (long)G, (hipStream_t)stream);
        DIGAT_CHECK_LAUNCH();
        if (n_seg == 0) continue;                    // nothing can bind: the round rejects nothing, its counter stays 0
        CapItemArgs ia{perm, seg_begin, seg_cap, seg_live, (long)n_seg, (long)G * M, st, counter + r};
        hipLaunchKernelGGL(cap_item_kernel, dim3((unsigned)((n_seg + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ia);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

int digat_capped_emit(const int64_t* ids, const float* scores, int64_t G, int M, int k, int64_t* out_ids, float* out_scores,
                      int32_t* out_count, int32_t* out_slots, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ids || !scores || !out_ids || !out_scores || !out_count || !out_slots) return DIGAT_ERR_ARG;
    const int bad = cap_check_lists(G, M, workspace, workspace_bytes);
    if (bad) return bad;
    if (k < 1 || k > TOPK_MAX_K) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    CapListArgs la{cap_carve(workspace, (long)G, M), M, k, 1, ids, scores, out_ids, out_scores, out_count, out_slots};
    cap_launch_list(la, (long)G, (hipStream_t)stream);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
