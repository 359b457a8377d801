// digat_rerank.inc — the joint re-rank: diversity (maximal marginal relevance), calibration (the category mix of the reader's history)
// and a cap per category in ONE greedy pass over a shortlist of up to DIGAT_RERANK_MAX_LIST = 1024 entries per user — the last stage
// behind util.recommend(rerank=) / nrms.recommend(rerank=), and plain MMR beyond the 128 entries digat_mmr_select stops at.  Included at
// the end of digat_kernels.hip, behind digat_topk.inc (topk_key), digat_dot_topk.inc (dot_load4), digat_list_softmax.inc (the LSM_*
// tile sizes: the similarity below is lsm_score_stage's product, restated with the picked row where the user row stands),
// digat_mmr.inc (sel_count, sel_fill, and for the short route mmr_gram) and digat_calibrate.inc (cal_target, cal_gain, cal_finish:
// the target row, a step's gains and the kl epilogue are cal_kernel's own functions, called here, not copied — every kernel's
// resource line is what it was with the code written out, down to the raw VGPR count).  One piece stays written out in
// rr_gram_kernel, the one-wave winner: as a function it cost a scalar j and about 1 % (digat_mmr.inc has the details).
//
// rr_kernel, one workgroup of 256 threads per list, list position p = slab * 256 + tid held by thread tid as its slot `slab` (four slabs):
// a thread keeps its slots' score, fl(w_rel s), gain category (-1: no element; 64: uncategorised), raw category, the step they were
// picked at, the cap counter and pen in registers, every loop over the slabs unrolled.  There is NO Gram: a step forms the one row of
// it that the step's winner needs.  A step:
//   gains    lane c < C of EVERY wave takes the two float64 logarithms of category c and keeps fl(w_cal gain32_c) — the same bits in every
//            wave, never exchanged; a slot fetches its category's with one ds_bpermute (cal_kernel's).
//   winner   value = fl(fl(rel - fl(w_div pen)) + red), a term whose weight is zero not formed at all (rr_value: contraction off, never an
//            fma); a slot's 32-bit key and its position packed as key << 32 | (1023 - p), so that the largest word is the largest key at
//            the LOWEST position — with this layout thread order does not imply position order; a thread's max, the wave's butterfly
//            over the 64-bit words, one double-buffered LDS slot per wave and one barrier; every thread reads all four.
//   update   the winner's two categories come from LDS (written once, before the loop): lane c's n_c += 1, the cap counters.
//   row      when w_div != 0 and another step follows: the winner's vector goes into LDS (channels from d on: zeros) and every slab below
//            count is scored against it as lsm_score_stage scores a list against its user: 128-byte lines staged through the padded
//            tile (stride 36 floats), eight threads a line, the next block's loads in flight under the arithmetic, one fp32 fmaf chain
//            per lane over ascending channels, the tail k-step padded with zeros: digat_dot_scores' bits.  pen = fmaxf(pen, that) at
//            elements.  A slot that is no element has a null row: zeros are staged, nothing is dereferenced.  Slabs at or beyond count
//            are skipped.
// The outputs are written once, behind the loop; kl is cal_kernel's (wave 0, one logarithm pair per category, a butterfly).  No atomics,
// no workspace: the same bits from run to run and in any batch.
//
// rr_gram_kernel, M <= 128 (chosen by M alone): mmr_kernel's layout — the list's Gram in LDS by mmr_gram (shared with digat_mmr.inc and
// digat_listq.inc, not copied), then wave 0 runs the same step on positions lane and lane + 64 with no workgroup barrier, the penalty read
// from the Gram's row.  mmr_gram's product and the chain above both have digat_dot_scores' bits, so the two routes pick the same entries
// (tests/test_hip_rerank.py: the same lists at M = 128 and inside M = 129).  On an MI355X at d = 400 a step of 4 096 lists of 128 costs
// 14 us at k = 100 (70 us at k = 10, the Gram's share larger) against 162 us (154 us) through rr_kernel (tools/kbench.py rerank; DESIGN
// section 8 has every case, the losing ones included).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   rr_kernel        VGPRs 131   SGPRs 106 (26 kept in VGPR lanes)   LDS 52288 B   scratch 0   occupancy 3 waves / SIMD (registers and LDS)
//   rr_gram_kernel   VGPRs 60 + AGPRs 64 (mmr_gram's 2 x 8 accumulator tiles)   SGPRs 97   LDS 2048 B static + 4 Mp max(Mp + 4, DOT_LD)
//                    dynamic (67 584 B at M = 128)   scratch 0   occupancy 4 waves / SIMD (by registers; by LDS two workgroups per CU at M = 128)
//
// Measured on an MI355X at d = 400, C = 17 (tools/kbench.py rerank, legs alternated, medians of five rounds): 4 096 lists of 1 024 take
// 11.0 ms at k = 10 and 121 ms at k = 100 — 1.1 to 1.2 ms per step, one gather of the list's rows per step — against 62 / 493 ms for
// gather + bmm Gram + torch rounds and 28 / 270 ms for rows gathered once + a batched matrix-vector product per step.  64 lists of 1 024
// (64 workgroups on 256 CUs) take 1.43 / 15.4 ms and LOSE long MMR (w_cal = 0) to the stock Gram leg (1.19 / 9.8 ms), which pays for its
// bmm once.

#define RR_MAX_M DIGAT_RERANK_MAX_LIST
#define RR_MAX_C DIGAT_CALIBRATE_MAX_CATEGORIES

static_assert(RR_MAX_M == LSM_MAX_M && LSM_SLABS == 4, "rr_kernel holds a list as four slots per thread");
static_assert(RR_MAX_C == 64, "lane c of a wave owns category c");

struct RrArgs {
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
    const float* target;
    int C;
    float w_rel, w_div, w_cal;
    double alpha;
    int k;
    int64_t* out_ids;
    float* out_scores;
    int32_t* out_count;
    float* out_kl;
};

// fl(fl(rel - fl(w_div pen)) + red); a term whose weight is zero is not formed.  Every operation rounded: never an fma.
__device__ __forceinline__ float rr_value(float rel, float w_div, float pen, float red, bool div, bool cal) {
#pragma clang fp contract(off)
    float v = rel;
    if (div) {
        const float dp = w_div * pen;
        v = rel - dp;
    }
    if (cal) v = v + red;
    return v;
}

__global__ void __launch_bounds__(256) rr_kernel(const RrArgs a) {
    __shared__ float4 su4[LSM_MAX_D / 4];                         // the picked row
    __shared__ float4 tile4[LSM_SLAB * LSM_LD / 4];               // a slab's staged block
    __shared__ long long lid[RR_MAX_M];                           // vectors row of every list position, -1: no element
    __shared__ signed char lcat[RR_MAX_M];                        // gain category of every position
    __shared__ int lraw[RR_MAX_M];                                // raw category (the cap's)
    __shared__ unsigned long long xbest[2][4];                    // a wave's winner of the step, double-buffered: one barrier per step
    float* const su = (float*)su4;
    float* const T = (float*)tile4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;                  // this thread stages rows r0 + 32 h, channels c4 .. c4 + 3
    const long g = blockIdx.x;
    const int cnt = sel_count(a.count, g, a.M);
    const bool div = a.w_div != 0.f, cal = a.w_cal != 0.f;
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.vectors) & 15) == 0;

    float s[LSM_SLABS], rel[LSM_SLABS], pen[LSM_SLABS];
    int cat[LSM_SLABS], raw[LSM_SLABS], picked[LSM_SLABS], same[LSM_SLABS];
#pragma unroll
    for (int b = 0; b < LSM_SLABS; ++b) {
        const int pos = b * LSM_SLAB + tid;
        s[b] = 0.f;
        pen[b] = 0.f;
        cat[b] = -1;
        raw[b] = 0;
        picked[b] = -1;
        same[b] = 0;
        long long id = -1;
        if (pos < cnt) {
            id = (long long)a.ids[g * a.M + pos];
            if (id < 0 || id >= a.N) id = -1;
        }
        if (id >= 0) {
            s[b] = a.scores[g * a.M + pos];
            cat[b] = RR_MAX_C;
            if (a.category) {
                raw[b] = a.category[id];
                if (raw[b] >= 0 && raw[b] < a.C) cat[b] = raw[b];
            }
        }
        rel[b] = cal_mul(a.w_rel, s[b]);
        lid[pos] = id;
        lcat[pos] = (signed char)cat[b];
        lraw[pos] = raw[b];
    }
    // lane c of every wave: category c of this list (no target: C = 0, every p_c is 0)
    const double p = cal_target(a.target, g, a.C, lane);
    const double oma = 1.0 - a.alpha;
    const double ap = a.alpha * p;
    int n = 0;
    __syncthreads();

    int t = 0;
    for (; t < a.k; ++t) {
        const float mg = cal ? cal_gain(a.w_cal, p, oma, ap, n, t) : 0.f;
        unsigned long long best = 0ull;
#pragma unroll
        for (int b = 0; b < LSM_SLABS; ++b) {
            const float got = __shfl(mg, cat[b] & 63, 64);        // every lane takes part; the value counts for a categorised element only
            const float red = cat[b] >= 0 && cat[b] < RR_MAX_C ? got : 0.f;
            const bool eligible = cat[b] >= 0 && picked[b] < 0 && (a.q == 0 || same[b] < a.q);
            const unsigned key = eligible ? topk_key(rr_value(rel[b], a.w_div, pen[b], red, div, cal)) : 0u;
            const unsigned long long word = ((unsigned long long)key << 32) | (unsigned)(RR_MAX_M - 1 - (b * LSM_SLAB + tid));
            if (key != 0u && word > best) best = word;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)best, o, 64);
            best = other > best ? other : best;
        }
        const int xb = t & 1;
        if (lane == 0) xbest[xb][wave] = best;
        __syncthreads();
        {
            const unsigned long long b0 = xbest[xb][0], b1 = xbest[xb][1], b2 = xbest[xb][2], b3 = xbest[xb][3];
            const unsigned long long m01 = b0 > b1 ? b0 : b1, m23 = b2 > b3 ? b2 : b3;
            best = m01 > m23 ? m01 : m23;
        }
        if (best == 0ull) break;                                  // nothing eligible: the same answer in every thread of the workgroup
        const int j = RR_MAX_M - 1 - (int)(unsigned)(best & 0xffffffffull);       // an element: j < cnt <= M
        const int cj = lcat[j], rj = lraw[j];
#pragma unroll
        for (int b = 0; b < LSM_SLABS; ++b) {
            if (j == b * LSM_SLAB + tid) picked[b] = t;
            if (a.q > 0) same[b] += cat[b] >= 0 && raw[b] == rj;
        }
        n += lane == cj;                                          // an uncategorised winner (RR_MAX_C) is no lane's
        if (!div || t + 1 >= a.k) continue;                       // workgroup-uniform

        // ---- the winner's row of the Gram: lsm_score_stage with the picked row where the user row stands
        const float* const prow = a.vectors + lid[j] * a.d;
        __syncthreads();                                          // the step before is done with su
        for (int c = tid; c < LSM_MAX_D; c += 256) su[c] = c < a.d ? prow[c] : 0.f;
#pragma unroll
        for (int b = 0; b < LSM_SLABS; ++b) {
            const int j0 = b * LSM_SLAB;
            if (j0 >= cnt) continue;                              // workgroup-uniform: a slab beyond count is skipped
            const float* row[8];
            float4 rv[8];
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const long long rid = lid[j0 + r0 + 32 * h];
                row[h] = rid >= 0 ? a.vectors + rid * a.d : nullptr;
                rv[h] = dot_load4(row[h], c4, a.d, vec);
            }
            __syncthreads();                                      // su is written; the slab before is done with the tile
            float acc = 0.f;
            for (int kb = 0; kb < a.d; kb += LSM_KB) {
#pragma unroll
                for (int h = 0; h < 8; ++h) *(float4*)&T[(r0 + 32 * h) * LSM_LD + c4] = rv[h];
                __syncthreads();
                if (kb + LSM_KB < a.d) {
#pragma unroll
                    for (int h = 0; h < 8; ++h) rv[h] = dot_load4(row[h], kb + LSM_KB + c4, a.d, vec);
                }
#pragma unroll
                for (int q = 0; q < LSM_KB / 4; ++q) {
                    if (kb + 4 * q < a.d) {                       // workgroup-uniform: dot_tile's k-steps, the last one padded with zeros
                        const float4 v = *(const float4*)&T[tid * LSM_LD + 4 * q];
                        const float4 w = su4[(kb >> 2) + q];
                        acc = fmaf(v.x, w.x, acc);
                        acc = fmaf(v.y, w.y, acc);
                        acc = fmaf(v.z, w.z, acc);
                        acc = fmaf(v.w, w.w, acc);
                    }
                }
                __syncthreads();
            }
            pen[b] = fmaxf(pen[b], cat[b] >= 0 ? acc : 0.f);
        }
    }

#pragma unroll
    for (int b = 0; b < LSM_SLABS; ++b) {
        if (picked[b] >= 0) {
            a.out_scores[g * a.k + picked[b]] = s[b];
            a.out_ids[g * a.k + picked[b]] = (int64_t)lid[b * LSM_SLAB + tid];
        }
    }
    sel_fill(a.out_scores, a.out_ids, g, a.k, t, tid, 256);
    if (wave == 0) cal_finish(p, oma, ap, n, t, lane, g, a.out_count, a.out_kl);
}

// The route of short lists, M <= 128: mmr_kernel's layout.  All four waves form the list's Gram in LDS (mmr_gram — the product digat_mmr.inc
// and digat_listq.inc share, digat_dot_scores' bits as the chain above), then wave 0 alone runs the steps, positions lane and lane + 64
// per lane, with no workgroup barrier inside the loop: the step above with the penalty read from the Gram's row.  The same values in the
// same order, so the same picks; which route runs depends on M alone.
__global__ void __launch_bounds__(256) rr_gram_kernel(const RrArgs a, const int ld) {
    extern __shared__ float4 rr_lds[];               // the staged rows [Mu][DOT_LD], then the Gram [Mu][ld]
    __shared__ long long lid[MMR_MAX_M];
    __shared__ int lcat[MMR_MAX_M], lraw[MMR_MAX_M];
    float* const L = (float*)rr_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int cnt = sel_count(a.count, g, a.M);
    const bool div = a.w_div != 0.f, cal = a.w_cal != 0.f;
    const int T = (cnt + 15) >> 4;                   // 16-row tiles of this list's Gram: <= 8, and 16 T <= ld - 4
    if (tid < MMR_MAX_M) {
        long long id = -1;
        if (tid < cnt) {
            id = (long long)a.ids[g * a.M + tid];
            if (id < 0 || id >= a.N) id = -1;
        }
        lid[tid] = id;
    }
    __syncthreads();
    if (div) mmr_gram(L, lid, a.vectors, a.d, T, ld);         // workgroup-uniform
    if (wave != 0) return;

    float s[2], rel[2], pen[2];
    long long id[2];
    int cat[2], raw[2], picked[2], same[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pos = lane + 64 * h;
        id[h] = lid[pos];
        s[h] = 0.f;
        pen[h] = 0.f;
        cat[h] = -1;
        raw[h] = 0;
        picked[h] = -1;
        same[h] = 0;
        if (id[h] >= 0) {                            // then pos < cnt <= M
            s[h] = a.scores[g * a.M + pos];
            cat[h] = RR_MAX_C;
            if (a.category) {
                raw[h] = a.category[id[h]];
                if (raw[h] >= 0 && raw[h] < a.C) cat[h] = raw[h];
            }
        }
        rel[h] = cal_mul(a.w_rel, s[h]);
        lcat[pos] = cat[h];
        lraw[pos] = raw[h];
    }
    dot_wave_sync();
    const double p = cal_target(a.target, g, a.C, lane);
    const double oma = 1.0 - a.alpha;
    const double ap = a.alpha * p;
    int n = 0;
    int t = 0;
    for (; t < a.k; ++t) {
        const float mg = cal ? cal_gain(a.w_cal, p, oma, ap, n, t) : 0.f;
        unsigned key[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float got = __shfl(mg, cat[h] & 63, 64);
            const float red = cat[h] >= 0 && cat[h] < RR_MAX_C ? got : 0.f;
            const bool eligible = cat[h] >= 0 && picked[h] < 0 && (a.q == 0 || same[h] < a.q);
            key[h] = eligible ? topk_key(rr_value(rel[h], a.w_div, pen[h], red, div, cal)) : 0u;
        }
        unsigned best = key[0] > key[1] ? key[0] : key[1];         // the one-wave winner, written out as in mmr_kernel (digat_mmr.inc says why)
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
        const int cj = lcat[j], rj = lraw[j];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (a.q > 0) same[h] += cat[h] >= 0 && raw[h] == rj;
            if (div) pen[h] = fmaxf(pen[h], cat[h] >= 0 ? L[j * ld + lane + 64 * h] : 0.f);
        }
        n += lane == cj;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (picked[h] >= 0) {
            a.out_scores[g * a.k + picked[h]] = s[h];
            a.out_ids[g * a.k + picked[h]] = (int64_t)id[h];
        }
    }
    sel_fill(a.out_scores, a.out_ids, g, a.k, t, lane, 64);
    cal_finish(p, oma, ap, n, t, lane, g, a.out_count, a.out_kl);
}

extern "C" {

size_t digat_rerank_select_workspace_bytes(int64_t lists, int m, int k) {
    (void)lists; (void)m; (void)k;
    return 0;                                        // a list's state lives in registers and LDS; the Gram is never formed
}

int digat_rerank_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const float* vectors, int64_t N, int d,
                        const int32_t* category, int max_per_category, const float* target, int C, float w_rel, float w_div, float w_cal,
                        double alpha, int k, int64_t* out_ids, float* out_scores, int32_t* out_count, float* out_kl, void* workspace,
                        size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!ids || !scores || !out_ids || !out_scores || !out_count || !out_kl || G < 0 || N < 0 || max_per_category < 0) return DIGAT_ERR_ARG;
    if (!(w_rel >= 0.f && w_rel < INFINITY) || !(w_div >= 0.f && w_div < INFINITY) || !(w_cal >= 0.f && w_cal < INFINITY)) return DIGAT_ERR_ARG;
    if (!(alpha > 0.0 && alpha < 1.0)) return DIGAT_ERR_ARG;
    if ((w_div != 0.f && !vectors) || ((w_cal != 0.f || max_per_category > 0 || target) && !category) || (w_cal != 0.f && !target)) return DIGAT_ERR_ARG;
    if (k < 1 || k > TOPK_MAX_K || M < 1 || M > RR_MAX_M || G > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (w_div != 0.f && (d < 1 || d > LSM_MAX_D)) return DIGAT_ERR_SHAPE;
    if (target && (C < 1 || C > RR_MAX_C)) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    RrArgs a{ids, scores, count, (long)G, M, vectors, (long)N, d, category, max_per_category, target, target ? C : 0, w_rel, w_div, w_cal,
             alpha, k, out_ids, out_scores, out_count, out_kl};
    if (M <= MMR_MAX_M) {                            // by M alone: the Gram of a short list fits LDS
        const int Mp = (M + 15) / 16 * 16;
        const size_t lds = (size_t)Mp * (size_t)(Mp + 4 > DOT_LD ? Mp + 4 : DOT_LD) * sizeof(float);
        if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)rr_gram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return DIGAT_ERR_LAUNCH;
        hipLaunchKernelGGL(rr_gram_kernel, dim3((unsigned)G), dim3(256), lds, (hipStream_t)stream, a, Mp + 4);
    } else {
        hipLaunchKernelGGL(rr_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
