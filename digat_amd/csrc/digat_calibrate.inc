// digat_calibrate.inc — calibrated top-k: a greedy re-rank of a shortlist per user that trades the model's score against the KL
// divergence between the category mix of the user's history (target [G, C]) and the list's (the last stage behind
// util.recommend(calibration=) / nrms.recommend(calibration=): "the k best whose categories look like what this reader reads").
// Included at the end of digat_kernels.hip, behind digat_topk.inc (topk_key: a step's winner is ordered as digat_topk_segments
// orders).  No Gram, so a list of DIGAT_CALIBRATE_MAX_LIST = 1024 entries is taken whole where digat_mmr_select stops at 128.
//
// cal_kernel<WAVES, PPL>, one workgroup of WAVES waves per list, list position p held by thread p / PPL as its entry p % PPL: the
// lowest (wave, lane) that holds a step's largest key holds its lowest position.  A thread keeps its positions' score, category
// (-1: no element; CAL_MAX_C: uncategorised) and the step they were picked at in registers, the loops over PPL unrolled.
//   <1, 2>  M <= 128: one wave, no barrier and no LDS inside the loop (mmr_kernel's greedy phase)
//   <4, 4>  M <= 1024: four waves, one workgroup barrier per step: a wave's winner (key, position, category) goes through a
//           double-buffered LDS slot and every thread reads all four
// A step: lane c < C of EVERY wave computes the two float64 logarithms of category c and keeps fl(mu * gain32_c) — the same bits in
// every wave, so the gains are never exchanged through LDS: a position fetches its category's gain with one ds_bpermute; then the
// PPL keys, the wave max over the 32-bit keys, a ballot for the lowest lane that holds it, and lane c's n_c += 1 for the winner's
// category.  value = fl(fl(lam * s) + fl(mu * gain32)) and q~ = fl(fl(fl((1 - alpha) n) / T) + fl(alpha p)) are written with
// contraction switched off (cal_value, cal_q): never an fma.  The outputs are written once, behind the loop, and kl is one more
// logarithm pair per category, summed over the wave by a butterfly (a fixed order: the same bits from run to run and in any batch).
// No atomics, no workspace.  The count clamp and the fill of unused slots are digat_mmr.inc's (sel_count, sel_fill); the target row,
// a step's gains and the kl epilogue are __device__ functions below (cal_target, cal_gain, cal_finish) that digat_rerank.inc calls too.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   cal_kernel<1, 2>   64 threads   VGPRs 52   SGPRs 57   LDS 0 B    scratch 0   occupancy 8 waves / SIMD
//   cal_kernel<4, 4>  256 threads   VGPRs 67   SGPRs 66   LDS 96 B   scratch 0   occupancy 7 waves / SIMD

#define CAL_MAX_M DIGAT_CALIBRATE_MAX_LIST
#define CAL_MAX_C DIGAT_CALIBRATE_MAX_CATEGORIES

static_assert(CAL_MAX_M == 1024, "cal_kernel<4, 4> holds a list as four positions per thread of four waves");
static_assert(CAL_MAX_C == 64, "lane c of a wave owns category c");

struct CalArgs {
    const int64_t* ids;
    const float* scores;
    const int32_t* count;
    long G;
    int M;
    const int32_t* category;
    long N;
    const float* target;
    int C;
    float lam, mu;
    double alpha;
    int k;
    int64_t* out_ids;
    float* out_scores;
    int32_t* out_count;
    float* out_kl;
};

// lam * s + mg with the product and the sum rounded: never an fma.
__device__ __forceinline__ float cal_value(float lam, float s, float mg) {
#pragma clang fp contract(off)
    const float rel = lam * s;
    return rel + mg;
}

__device__ __forceinline__ float cal_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}

// q~_c(n) at list length T: ((1 - alpha) n) / T + alpha p_c, four rounded float64 operations (ap = fl(alpha p_c) is the list's).
__device__ __forceinline__ double cal_q(double oma, int n, double T, double ap) {
#pragma clang fp contract(off)
    const double num = oma * (double)n;
    const double share = num / T;
    return share + ap;
}

// The calibration pieces of a list, shared with rr_kernel and rr_gram_kernel (digat_rerank.inc).  Lane c of a wave owns category c.
// p_c of list g: the target where it is finite and > 0, else 0 (lanes from C on: 0).
__device__ __forceinline__ double cal_target(const float* target, const long g, const int C, const int lane) {
    double p = 0.0;
    if (lane < C) {
        const float tv = target[g * C + lane];
        if (tv > 0.f && tv < INFINITY) p = (double)tv;       // a NaN fails both comparisons
    }
    return p;
}

// fl(w * gain32_c) of step t with n_c = n picked: the two float64 logarithms of the lane's category; 0 where p_c = 0.
__device__ __forceinline__ float cal_gain(const float w, const double p, const double oma, const double ap, const int n, const int t) {
    if (!(p > 0.0)) return 0.f;
    const double T = (double)(t + 1);
    const double q0 = cal_q(oma, n, T, ap), q1 = cal_q(oma, n + 1, T, ap);
    const double gain = p * (log(q1) - log(q0));
    return cal_mul(w, (float)gain);
}

// Behind the loop, one whole wave: kl of the finished list of t picks — one more logarithm pair per category, summed by a butterfly
// (a fixed order) — and lane 0 writes it with the count.
__device__ __forceinline__ void cal_finish(const double p, const double oma, const double ap, const int n, const int t, const int lane,
                                           const long g, int32_t* out_count, float* out_kl) {
    double term = 0.0;
    if (p > 0.0) term = p * (log(p) - log(cal_q(oma, n, (double)(t > 1 ? t : 1), ap)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if (lane == 0) {
        out_count[g] = t;
        out_kl[g] = (float)term;
    }
}

template <int WAVES, int PPL>
__global__ void __launch_bounds__(64 * WAVES) cal_kernel(const CalArgs a) {
    __shared__ unsigned xkey[2][WAVES];              // a wave's winner of the step, double-buffered: one barrier per step
    __shared__ int xpos[2][WAVES], xcat[2][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int cnt = sel_count(a.count, g, a.M);

    float s[PPL];
    int cat[PPL], picked[PPL];
#pragma unroll
    for (int h = 0; h < PPL; ++h) {
        const int pos = tid * PPL + h;
        s[h] = 0.f;
        cat[h] = -1;
        picked[h] = -1;
        if (pos < cnt) {
            const long long id = (long long)a.ids[g * a.M + pos];
            if (id >= 0 && id < a.N) {
                s[h] = a.scores[g * a.M + pos];
                const int c = a.category[id];
                cat[h] = c >= 0 && c < a.C ? c : CAL_MAX_C;
            }
        }
    }
    // lane c of every wave: category c of this list
    const double p = cal_target(a.target, g, a.C, lane);
    const double oma = 1.0 - a.alpha;
    const double ap = a.alpha * p;
    int n = 0;

    int t = 0;
    for (; t < a.k; ++t) {
        const float mg = cal_gain(a.mu, p, oma, ap, n, t);
        unsigned bkey = 0u;
        int bpos = 0, bcat = 0;
#pragma unroll
        for (int h = 0; h < PPL; ++h) {
            const float got = __shfl(mg, cat[h] & 63, 64);   // every lane takes part; the value counts for a categorised element only
            const float gain = cat[h] >= 0 && cat[h] < CAL_MAX_C ? got : 0.f;
            const unsigned key = cat[h] >= 0 && picked[h] < 0 ? topk_key(cal_value(a.lam, s[h], gain)) : 0u;
            if (key > bkey) {                        // equal keys: the lower position stays
                bkey = key;
                bpos = tid * PPL + h;
                bcat = cat[h];
            }
        }
        unsigned best = bkey;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)best, o, 64);
            best = other > best ? other : best;
        }
        const unsigned long long holds = __ballot(bkey == best);
        const int src = __ffsll((long long)holds) - 1;       // best == 0: every lane holds it, lane 0 answers
        int j = __shfl(bpos, src, 64), cj = __shfl(bcat, src, 64);
        if (WAVES > 1) {
            const int b = t & 1;
            if (lane == 0) {
                xkey[b][wave] = best;
                xpos[b][wave] = j;
                xcat[b][wave] = cj;
            }
            __syncthreads();
            best = xkey[b][0];
            j = xpos[b][0];
            cj = xcat[b][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                const unsigned kw = xkey[b][w];
                if (kw > best) {                     // equal keys: the lower wave holds the lower position
                    best = kw;
                    j = xpos[b][w];
                    cj = xcat[b][w];
                }
            }
        }
        if (best == 0u) break;                       // nothing eligible: the same answer in every thread of the workgroup
#pragma unroll
        for (int h = 0; h < PPL; ++h)
            if (j == tid * PPL + h) picked[h] = t;
        n += lane == cj;                             // an uncategorised winner (CAL_MAX_C) is no lane's
    }

#pragma unroll
    for (int h = 0; h < PPL; ++h) {
        if (picked[h] >= 0) {
            a.out_scores[g * a.k + picked[h]] = s[h];
            a.out_ids[g * a.k + picked[h]] = a.ids[g * a.M + tid * PPL + h];
        }
    }
    sel_fill(a.out_scores, a.out_ids, g, a.k, t, tid, 64 * WAVES);
    if (wave == 0) cal_finish(p, oma, ap, n, t, lane, g, a.out_count, a.out_kl);
}

extern "C" {

size_t digat_calibrated_select_workspace_bytes(int64_t lists, int m, int c, int k) {
    (void)lists; (void)m; (void)c; (void)k;
    return 0;                                        // a list's whole state lives in registers and 96 bytes of LDS
}

int digat_calibrated_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const int32_t* category,
                            int64_t N, const float* target, int C, float lam, float mu, double alpha, int k, int64_t* out_ids,
                            float* out_scores, int32_t* out_count, float* out_kl, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!ids || !scores || !category || !target || !out_ids || !out_scores || !out_count || !out_kl || G < 0 || N < 0) return DIGAT_ERR_ARG;
    if (!(lam >= 0.f && lam <= 1.f) || !(alpha > 0.0 && alpha < 1.0)) return DIGAT_ERR_ARG;
    if (k < 1 || k > TOPK_MAX_K || M < 1 || M > CAL_MAX_M || C < 1 || C > CAL_MAX_C || G > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    CalArgs a{ids, scores, count, (long)G, M, category, (long)N, target, C, lam, mu, alpha, k, out_ids, out_scores, out_count, out_kl};
    if (M <= 128)
        hipLaunchKernelGGL((cal_kernel<1, 2>), dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((cal_kernel<4, 4>), dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
