// digat_list_plrank.inc — the PL-Rank policy gradient of a position-weighted metric over a user's OWN list of news: the lists are scored
// once, the Plackett-Luce slates are drawn from those scores inside the kernel that scored them, the metric of every slate is taken,
// and the backward is the PL-Rank-2 estimator of the gradient of the EXPECTED metric (Oosterhuis, "Computationally Efficient
// Optimization of Plackett-Luce Ranking Models", SIGIR 2021; "Learning-to-Rank at the Speed of Sampling", 2022) — evaluate.list_plrank,
// evaluate.plrank_scores, nrms.plrank_step, nrms.fit_policy(estimator="plrank").  Included in digat_kernels.hip behind digat_list_pl.inc:
// lists, elements, live positions, a_j = fl((double)score_j inv_t), w_j = exp(max(a_j - a_max, -700)) and Z_t are digat_list_pl.inc's, to
// the letter (lsm_score_stage, pl_stage_list, pl_cut_slate, pl_z_stage); the draw is digat_pl_sample.inc's pl_draw_slate, the function
// pl_sample_kernel calls; the two ends behind the coefficient are lpw_users_kernel and lsm_rows_kernel, as in digat_list_pl_bwd.
//
// The metric of a slate is a sum over positions, R(y) = sum_t theta_t rho_{y_t}: gain [G, M] f32 (rho; a NaN, an infinity or a negative
// value counts as 0), discount [k] f64 (theta; finite, >= 0), list_weight [G] f64 (NULL: 1).  For one slate of length n with picks
// p_0 .. p_{n-1}:  r_t = fl(theta_t rho_{p_t});  PR_t = sum_{x = t}^{n-1} r_x, PR_n = 0;  A_t = sum_{u < t} theta_u / Z_u;
// B_t = sum_{u < t} PR_u / Z_u.  The per-slate coefficient, a_max and the clamp held constant:
//   c(j)   = w_j (rho_j A_n - B_n)                          j live, not in the slate
//   c(p_t) = PR_{t+1} + w_{p_t} (rho_{p_t} A_{t+1} - B_{t+1})
//   c(j)   = 0                                              j not live
//   slate_value = PR_0
// Each position is credited only with the reward that comes after it, and an item's own reward enters through its conditional
// expectation (w_j theta_u rho_j / Z_u at every step u it was still in the list), not through the event of being drawn: the mean of c
// over the policy's slates is the exact gradient of E[R] in a, with no baseline (tests/test_plrank_cpu.py enumerates every slate).
// Per list, for S slates, with f = fl(fl(inv_t list_weight[g]) grad_value[g]):
//   value[g]   = fl(list_weight[g] fl((sum_s slate_value[g, s]) / S))
//   coef[g, j] = fl32(fl(f fl((sum_s c_s(j)) / S))), exactly 0 at every slot that is not live
// An empty slate adds nothing and still counts in S.  value is the sample mean of the metric; its backward is the ESTIMATOR above, not
// the derivative of that sample mean (which is 0: the picks are constants).
//
// One workgroup of 256 threads per list; the list's S slates run inside it in ascending s: no floating-point atomics, no [G, S, M]
// workspace, the same bits from two calls, for a list alone or in a batch and — the draw being a function of (seed, stream,
// first_sample + s, position) — from a call split by first_sample (slate_value and picks; value and coef are sums over a call's S).
//   plr_fwd_kernel         lsm_score_stage, PlShared laid over the dead tile as in lpl_fwd_kernel, then plr_slates.
//   plr_scores_fwd_kernel  its twin from GIVEN scores (pl_stage_list): models whose score is no inner product, and the no-graph use.
//   plr_slates             per slate: pl_draw_slate (picks_in NULL; the picks are written out) or pl_cut_slate; thread t < n forms r_t;
//                          thread 0 adds them from the END of the slate (PR_0 as the coefficient kernel forms it) and keeps the sum
//                          over s.  The forward needs no Z_t: pl_z_stage is not run here.
//   plr_coef_kernel        lpl_coef_kernel's frame: sh.a from the saved scores, then per non-empty slate pl_cut_slate + pl_z_stage;
//                          thread t < n: r_t and fl(theta_t / Z_t); thread 0: the PR suffix; thread t < n: fl(PR_t / Z_t); thread 0 the
//                          prefix A, thread 64 (another wave) the prefix B — serial chains of at most 128 additions each; every thread
//                          adds fl(w_j fl(fl(rho_j A_n) - B_n)) for its four positions to fp64 registers (sh.w holds 0 at the picked and
//                          the dead positions); thread t < n adds fl(PR_{t+1} + fl(w_pick fl(fl(rho A_{t+1}) - B_{t+1}))) to an LDS
//                          accumulator (a slate's positions are distinct: one writer per slot, slates apart by barriers).  One float32
//                          rounding at the end.  A list whose grad_value is 0 writes zeros and runs no slate.
//   backward               plr_coef_kernel -> workspace [G, M]; lpw_users_kernel with a NULL per-list factor -> d_users; lsm_rows_kernel
//                          with the caller's sorted entry keys -> d_rows: digat_list_pl_bwd's chain.
// Everything in fp64 under `#pragma clang fp contract(off)`.
//
// The bound evaluate.plrank_bound states for coef against evaluate.plrank_host (numpy float64, math.fsum), derived.  u = 2^-53, n = the
// list's live positions, first order, relative to a term's size.  Device and twin form a, a_max, a - a_max, the clamp, r_t and f with the
// same roundings on the same inputs.
//   w_j            exp correct to 1 ulp on either side:                                                    4
//   Z_t            digat_pl_sample.inc: the twin's fsum against at most n positive additions:               n + 4
//   theta_t / Z_t  one division on either side:                                                            n + 6
//   A              at most k positive terms in slate order, (k - 1); the twin's fsum, 1:                   n + k + 6     of A
//   PR_t           r_t agree; at most k positive additions from the end, (k - 1); the twin's fsum, 1:      k             of PR_t
//   PR_t / Z_t     k + (n + 4) + one division on either side:                                              n + k + 6
//   B              at most k positive terms, the twin's fsum:                                              n + 2k + 6    of B
//   rho_j A        one product on either side:                                                             n + k + 8     of rho A
//   rho_j A - B    the difference rounded on either side, 2 of |rho A - B| <= rho A + B:                   n + 2k + 10   of rho A + B
//   w (rho A - B)  w's 4 and one product on either side:                                                   n + 2k + 16   of w (rho A + B)
//   PR_{t+1} + ..  PR's k <= n + 2k + 16; the sum rounded on either side, 2:                               n + 2k + 18   of PR + w (rho A + B)
//   sum over s     a slot's terms go to the register chain or the LDS chain: at most S - 1 additions of at most u times the absolute
//                  sum each, the last addition 1, the twin's fsum 1:                                       S + 1
//   / S and f      a division and a product on either side:                                                4
// Together (n + 2k + S + 23) u Abs with Abs(g, j) = |f| sum_s (PR_{t+1} 1[j = p_t in slate s] + w_j (rho_j A + B)) / S — rho_j A - B
// cancels within a slate and the terms across slates, so the error is relative to the ABSOLUTE sum, as in digat_list_pl.inc.  One
// float32 rounding, or float32's subnormal spacing:
//   |coef - twin| <= 2^-24 |coef| + (n + 2k + S + 24) 2^-53 Abs + 2^-149                               (24: 23 and the second order)
// slate_value: r_t agree, at most k positive additions against the twin's fsum: k u; value: the sum over s (S + 1) u, the division and
// the product on either side 4 u:  |value - twin| <= (k + S + 6) 2^-53 |value|  (6: 5 and the second order); slate_value carries the
// same bound.  Both hold while Z_t, theta_t / Z_t and the products stay normal float64 numbers (|a - a_max| clamps at 700).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup, scratch 0 everywhere:
//   plr_fwd_kernel          VGPRs 84   SGPRs 105   LDS 57344 B   occupancy 2 waves / SIMD (by LDS: lpl_fwd_kernel's 40 960 B and the
//                           16 384 B of PlRec beside it, within 64 KB; two workgroups of 56 KB fit a CU's 160 KB)
//   plr_scores_fwd_kernel   VGPRs 57   SGPRs 105   LDS 37424 B   occupancy 4 waves / SIMD (by LDS: PlShared and PlRec, pl_sample_kernel's;
//                           four workgroups a CU)
//   plr_coef_kernel         VGPRs 88   SGPRs 101   LDS 35384 B   occupancy 4 waves / SIMD (by LDS: PlShared, the picked sums, PlrSums;
//                           four workgroups a CU)
// The kernels whose stages this file shares keep their lines, restated from the same build as VGPRs / SGPRs / LDS / waves per SIMD:
// pl_sample_kernel (its draw now pl_draw_slate) 32 / 64 / 37424 / 4, pl_log_prob_kernel 30 / 53 / 21040 / 7, lpl_fwd_kernel
// 84 / 89 / 40960 / 4, lpl_coef_kernel 74 / 84 / 29232 / 5.
//
// Seen on an MI355X over the sweep of tests/test_hip_plrank.py: the worst |coef - twin| is 0.993 of the bound (G = 65, M = 257, k = 128) —
// the float32 rounding alone —, value 0.167 and slate_value 0.116 of theirs.
// Measured on an MI355X at d = 400 (tools/kbench.py plrank; legs alternated in one process, medians of five rounds; forward | forward +
// backward, ms) against what a sampled-slate step was made of before — list_softmax's forward, pl_sample, the slates' nDCG by a gather,
// leave-one-out weights, list_pl — and against the stock torch composition (bmm scores, rand + topk slates, evaluate._pl_stock):
//   4 096 x 1 024, k = 10, S = 1:  1.63 | 4.05  against 2.68 | 4.45 and 5.25 | 19.95;   S = 8:  3.32 | 5.86 against 3.89 | 5.72 and 6.18 | 19.55
//   4 096 x 128,   k = 10, S = 1:  0.39 | 1.19  against 0.63 | 1.39 and 0.81 | 2.71;    S = 8:  0.82 | 1.66 against 1.09 | 1.86 and 1.05 | 3.71
//   64 x 1 024,    k = 10, S = 1:  0.26 | 0.92  against 0.61 | 1.24 and 0.34 | 1.44;    S = 8:  0.45 | 1.15 against 0.67 | 1.38 and 0.37 | 1.53
//   64 x 128,      k = 10, S = 1:  0.12 | 0.67  against 0.37 | 0.97 and 0.34 | 1.45;    S = 8:  0.17 | 0.71 against 0.42 | 0.99 and 0.37 | 1.50
// The forward wins against the three launches it replaces in all sixteen cases (1.17x - 3.1x); with the backward it wins 1.08x - 1.56x in
// fifteen and LOSES one, 4 096 x 1 024 at k = 10, S = 8 (5.86 against 5.72 ms): the S draws of a list — a 1 024-record sort each — run one
// after the other in a workgroup that holds two waves per SIMD, where pl_sample spreads them over G S workgroups at four.  For the same
// reason the forward loses to the launch-bound stock composition at 64 x 1 024, S = 8 (0.45 - 0.46 against 0.37 ms).  An S-parallel draw
// was not built.  tools/kbench.py policy (planted-signal corpus, NRMS at d = 64, random titles, 300 steps of 64 lists, both legs warmed by
// three untimed steps): fit_policy(estimator="plrank") 2.7 ms a step against REINFORCE's 4.3 in the same run (fit_ranker 2.6, the click
// softmax 2.5); the nDCG@10 of the steps' own slates 0.1599 -> 0.2180 against 0.1564 -> 0.1805; held-out clicks do not move (nDCG@10 0.1548
// against 0.1518; plrank - REINFORCE +0.0029 [-0.0051, +0.0109]); the variance of d_users over 64 values of first_sample at 4 samples,
// summed over coordinates: 1.93e-3 against 6.68e-3 for REINFORCE with the leave-one-out baseline, 0.289 of it (DESIGN section 8).

struct PlrArgs {
    LsmArgs l;                           // plr_fwd_kernel: users, rows, ids, count, G, P, M, d; scores out
    PlArgs p;                            // scores (in), count, M, k, inv_t, seed, first_sample, S, streams, picks_in (NULL: draw), out_picks
    const float* gain;                   // [G, M]
    const double* discount;              // [k]
    const double* list_weight;           // [G]; NULL: 1
    const double* grad_value;            // [G]
    double* slate_value;                 // [G, S]
    double* value;                       // [G]
    float* coef;                         // [G, M]
};

struct PlrSums {
    double r[PL_MAX_K], pr[PL_MAX_K + 1], qa[PL_MAX_K], qb[PL_MAX_K], A[PL_MAX_K], B[PL_MAX_K];
};

static_assert(LSM_SLAB * LSM_LD * sizeof(float) + LSM_MAX_D * sizeof(float) + LSM_SLAB * sizeof(long long) + PL_MAX_M * sizeof(PlRec) <= 65536,
              "plr_fwd_kernel's static LDS");

// slate_value's gain: a NaN, an infinity or a negative value counts as 0.
__device__ __forceinline__ double plr_gain(float x) { return x - x == 0.f && x > 0.f ? (double)x : 0.0; }

// The slates of list g under sh.a (the whole workgroup, behind sh.a's stores): picks (drawn, or cut from picks_in), slate_value and value.
__device__ __forceinline__ void plr_slates(const PlrArgs& a, long g, PlShared& sh, PlRec* rec) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const unsigned stream = a.p.streams ? (unsigned)a.p.streams[g] : (unsigned)g;
    double total = 0.0;                              // thread 0's
    for (long s = 0; s < a.p.S; ++s) {
        const size_t row = (size_t)g * (size_t)a.p.S + (size_t)s;
        int n_out;
        if (a.p.picks_in) {
            n_out = pl_cut_slate(a.p, row, sh);      // its first barrier stands behind sh.a
        } else {                                     // a thread reads its own sh.a; the slate before left rec and sh.cut behind a barrier
            n_out = pl_draw_slate(sh, rec, a.p.M, a.p.k, a.p.seed, stream, a.p.first_sample + s);
            if (tid < a.p.k) a.p.out_picks[row * a.p.k + tid] = sh.pick[tid];
        }
        if (tid < n_out) sh.v[tid] = a.discount[tid] * plr_gain(a.gain[(size_t)g * a.p.M + sh.pick[tid]]);      // sh.pick[tid]: this thread's own
        __syncthreads();
        if (tid == 0) {
            double pr = 0.0;
            for (int t = n_out - 1; t >= 0; --t) pr = pr + sh.v[t];
            a.slate_value[row] = pr;
            total = total + pr;
        }
        // the next slate's first write to sh.v stands behind the barriers of its cut or its draw
    }
    if (tid == 0) a.value[g] = (a.list_weight ? a.list_weight[g] : 1.0) * (total / (double)a.p.S);
}

__global__ void __launch_bounds__(256) plr_fwd_kernel(const PlrArgs a) {
    __shared__ float4 su4[LSM_MAX_D / 4];
    __shared__ float4 tile4[LSM_SLAB * LSM_LD / 4];
    __shared__ long long sid[LSM_SLAB];
    __shared__ PlRec rec[PL_MAX_M];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = lsm_count(a.l, g);
    float sc[LSM_SLABS];
    bool el[LSM_SLABS];
    lsm_score_stage(a.l, g, cnt, su4, tile4, sid, sc, el);              // its last read of the tile is behind a barrier
    PlShared& sh = *reinterpret_cast<PlShared*>(tile4);
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const float x = sc[s];
        sh.a[s * LSM_SLAB + tid] = el[s] && x - x == 0.f ? pl_mul((double)x, a.p.inv_t) : -INFINITY;      // pl_stage_list's rule
    }
    plr_slates(a, g, sh, rec);
}

__global__ void __launch_bounds__(256) plr_scores_fwd_kernel(const PlrArgs a) {
    __shared__ PlShared sh;
    __shared__ PlRec rec[PL_MAX_M];
    const long g = blockIdx.x;
    pl_stage_list(a.p, g, sh);
    plr_slates(a, g, sh, rec);
}

__global__ void __launch_bounds__(256) plr_coef_kernel(const PlrArgs a) {
#pragma clang fp contract(off)
    __shared__ PlShared sh;
    __shared__ PlrSums q;
    __shared__ double picked[PL_MAX_M];              // the picked positions' own terms, summed over the slates
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const double gv = a.grad_value[g];
    if (gv == 0.0) {                                 // workgroup-uniform: a zero weight moves nothing
        for (int j = tid; j < a.p.M; j += 256) a.coef[(size_t)g * a.p.M + j] = 0.f;
        return;
    }
    pl_stage_list(a.p, g, sh);
    double acc[4], rho[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int j = tid + 256 * h;
        acc[h] = 0.0;
        picked[j] = 0.0;
        rho[h] = j < a.p.M ? plr_gain(a.gain[(size_t)g * a.p.M + j]) : 0.0;
    }
    for (long s = 0; s < a.p.S; ++s) {
        const size_t row = (size_t)g * (size_t)a.p.S + (size_t)s;
        const int n_out = pl_cut_slate(a.p, row, sh);
        if (n_out == 0) continue;                    // workgroup-uniform: an empty slate adds nothing
        pl_z_stage(sh, n_out);
        double rp = 0.0;                             // rho of this thread's pick
        if (tid < n_out) {
            const double th = a.discount[tid];
            rp = plr_gain(a.gain[(size_t)g * a.p.M + sh.pick[tid]]);
            q.r[tid] = th * rp;
            q.qa[tid] = th / sh.z[tid];
        }
        __syncthreads();
        if (tid == 0) {
            double pr = 0.0;
            q.pr[n_out] = 0.0;
            for (int t = n_out - 1; t >= 0; --t) {
                pr = pr + q.r[t];
                q.pr[t] = pr;                        // PR_t
            }
        }
        __syncthreads();
        if (tid < n_out) q.qb[tid] = q.pr[tid] / sh.z[tid];
        __syncthreads();
        if (tid == 0) {
            double A = 0.0;
            for (int t = 0; t < n_out; ++t) {
                A = A + q.qa[t];
                q.A[t] = A;                          // A_{t+1}
            }
        }
        if (tid == 64) {
            double B = 0.0;
            for (int t = 0; t < n_out; ++t) {
                B = B + q.qb[t];
                q.B[t] = B;                          // B_{t+1}
            }
        }
        __syncthreads();
        const double An = q.A[n_out - 1], Bn = q.B[n_out - 1];
#pragma unroll
        for (int h = 0; h < 4; ++h) acc[h] = acc[h] + sh.w[tid + 256 * h] * (rho[h] * An - Bn);
        if (tid < n_out) {
            const int p = sh.pick[tid];
            picked[p] = picked[p] + (q.pr[tid + 1] + sh.wpick[tid] * (rp * q.A[tid] - q.B[tid]));
        }
        // the next slate's first writes to sh.w, sh.wpick and q stand behind pl_cut_slate's barriers; sh.pick[tid] is this thread's own
    }
    __syncthreads();
    const double f = (a.p.inv_t * (a.list_weight ? a.list_weight[g] : 1.0)) * gv;
    const double Sd = (double)a.p.S;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int j = tid + 256 * h;
        if (j < a.p.M) a.coef[(size_t)g * a.p.M + j] = sh.a[j] > -INFINITY ? (float)(f * ((acc[h] + picked[j]) / Sd)) : 0.f;
    }
}

// picks may be NULL in a forward: the slates are drawn and written to out_picks.
static int plr_check(const void* picks, const void* out_picks, bool forward, const float* gain, const double* discount, const double* list_weight,
                     int64_t G, int M, int k, double inv_t, int64_t S, int64_t first_sample, const int64_t* streams) {
    if ((!picks && !(forward && out_picks)) || !gain || !discount || G < 0) return DIGAT_ERR_ARG;
    if (((uintptr_t)picks & 3) || ((uintptr_t)out_picks & 3) || ((uintptr_t)gain & 3) || ((uintptr_t)discount & 7) || ((uintptr_t)list_weight & 7) ||
        ((uintptr_t)streams & 7))
        return DIGAT_ERR_ARG;
    if (!(inv_t > 0.0) || !(inv_t * 3.4028234663852886e38 < INFINITY)) return DIGAT_ERR_ARG;       // a NaN fails the first comparison
    if (k < 1 || k > PL_MAX_K || M < 1 || M > PL_MAX_M || S < 1 || G * (int64_t)M > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (first_sample < 0 || first_sample > DIGAT_PL_MAX_SAMPLE || S > DIGAT_PL_MAX_SAMPLE - first_sample) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

static PlrArgs plr_args(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t S, const int32_t* picks,
                        const float* gain, const double* discount, const double* list_weight) {
    PlrArgs a{};
    a.l.count = count; a.l.G = (long)G; a.l.M = M;
    a.p.scores = scores; a.p.count = count; a.p.M = M; a.p.k = k; a.p.inv_t = inv_t; a.p.S = (long)S; a.p.picks_in = picks;
    a.gain = gain; a.discount = discount; a.list_weight = list_weight;
    return a;
}

extern "C" {

size_t digat_list_plrank_workspace_bytes(int64_t lists, int m) { return digat_list_softmax_workspace_bytes(lists, m); }

int digat_list_plrank_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                          const float* gain, const double* discount, const double* list_weight, const int32_t* picks, int64_t samples, int k,
                          double inv_t, uint32_t seed, int64_t first_sample, const int64_t* streams, int32_t* out_picks,
                          double* out_slate_value, double* out_value, float* out_scores, void* stream) {
    if (!out_slate_value || !out_value || !out_scores || ((uintptr_t)out_slate_value & 7) || ((uintptr_t)out_value & 7) || ((uintptr_t)out_scores & 3))
        return DIGAT_ERR_ARG;
    int rc = lpl_list_check(users, rows, ids, count, P, d);
    if (rc == DIGAT_OK) rc = plr_check(picks, out_picks, true, gain, discount, list_weight, G, M, k, inv_t, samples, first_sample, streams);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    PlrArgs a = plr_args(nullptr, count, G, M, k, inv_t, samples, picks, gain, discount, list_weight);
    a.l.users = users; a.l.rows = rows; a.l.ids = ids; a.l.P = (long)P; a.l.d = d; a.l.scores = out_scores;
    a.p.seed = seed; a.p.first_sample = (long)first_sample; a.p.streams = streams; a.p.out_picks = out_picks;
    a.slate_value = out_slate_value; a.value = out_value;
    hipLaunchKernelGGL(plr_fwd_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_plrank_scores_fwd(const float* scores, const int32_t* count, int64_t G, int M, const float* gain, const double* discount,
                            const double* list_weight, const int32_t* picks, int64_t samples, int k, double inv_t, uint32_t seed,
                            int64_t first_sample, const int64_t* streams, int32_t* out_picks, double* out_slate_value, double* out_value,
                            void* stream) {
    if (!scores || !out_slate_value || !out_value || ((uintptr_t)scores & 3) || ((uintptr_t)count & 3) || ((uintptr_t)out_slate_value & 7) ||
        ((uintptr_t)out_value & 7))
        return DIGAT_ERR_ARG;
    const int rc = plr_check(picks, out_picks, true, gain, discount, list_weight, G, M, k, inv_t, samples, first_sample, streams);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    PlrArgs a = plr_args(scores, count, G, M, k, inv_t, samples, picks, gain, discount, list_weight);
    a.p.seed = seed; a.p.first_sample = (long)first_sample; a.p.streams = streams; a.p.out_picks = out_picks;
    a.slate_value = out_slate_value; a.value = out_value;
    hipLaunchKernelGGL(plr_scores_fwd_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_plrank_scores_bwd(const float* scores, const int32_t* count, int64_t G, int M, const float* gain, const double* discount,
                            const double* list_weight, const int32_t* picks, int64_t samples, int k, double inv_t, const double* grad_value,
                            float* out_grad, void* stream) {
    if (!scores || !grad_value || !out_grad) return DIGAT_ERR_ARG;
    if (((uintptr_t)scores & 3) || ((uintptr_t)count & 3) || ((uintptr_t)grad_value & 7) || ((uintptr_t)out_grad & 3)) return DIGAT_ERR_ARG;
    const int rc = plr_check(picks, nullptr, false, gain, discount, list_weight, G, M, k, inv_t, samples, 0, nullptr);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    PlrArgs a = plr_args(scores, count, G, M, k, inv_t, samples, picks, gain, discount, list_weight);
    a.grad_value = grad_value; a.coef = out_grad;
    hipLaunchKernelGGL(plr_coef_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_list_plrank_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                          const float* scores, const float* gain, const double* discount, const double* list_weight, const int32_t* picks,
                          int64_t samples, int k, double inv_t, const double* grad_value, const int64_t* entry_keys, int64_t E,
                          float* d_users, float* d_rows, void* workspace, size_t workspace_bytes, void* stream) {
    if (!scores || !grad_value || !d_users || ((uintptr_t)scores & 3) || ((uintptr_t)grad_value & 7) || ((uintptr_t)d_users & 3) ||
        ((uintptr_t)d_rows & 3) || ((uintptr_t)entry_keys & 7))
        return DIGAT_ERR_ARG;
    int rc = lpl_list_check(users, rows, ids, count, P, d);
    if (rc == DIGAT_OK) rc = plr_check(picks, nullptr, false, gain, discount, list_weight, G, M, k, inv_t, samples, 0, nullptr);
    if (rc != DIGAT_OK) return rc;
    if (d_rows && (E < 0 || E > G * (int64_t)M || (E > 0 && !entry_keys))) return DIGAT_ERR_ARG;
    if (G > 0 && (!workspace || (((uintptr_t)workspace) & 3))) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_list_plrank_workspace_bytes(G, M)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    PlrArgs a = plr_args(scores, count, G, M, k, inv_t, samples, picks, gain, discount, list_weight);
    a.grad_value = grad_value; a.coef = (float*)workspace;
    LpwArgs b{};                                                      // the gather and the rows kernel, from the coefficients as they stand
    b.l.users = users; b.l.rows = rows; b.l.ids = ids; b.l.count = count;
    b.l.G = (long)G; b.l.P = (long)P; b.l.M = M; b.l.d = d;
    b.l.keys = entry_keys; b.l.E = G > 0 ? (long)E : 0;
    b.l.coef = (float*)workspace; b.l.d_users = d_users; b.l.d_rows = d_rows;
    b.lambda = (float*)workspace;
    if (G > 0) {
        hipLaunchKernelGGL(plr_coef_kernel, dim3((unsigned)G), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(lpw_users_kernel, dim3((unsigned)G), dim3(256), 0, st, b);
        DIGAT_CHECK_LAUNCH();
    }
    if (d_rows && P > 0) {                                            // G == 0: no entry, every row zero
        hipLaunchKernelGGL(lsm_rows_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, b.l);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

}  // extern "C"
