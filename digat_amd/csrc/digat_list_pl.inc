// digat_list_pl.inc — the differentiable Plackett-Luce slate likelihood over a user's OWN list of news: the log-probability of GIVEN
// slates under softmax(scale <user, news> / T) and its gradients in users and rows (evaluate.list_pl, evaluate.pl_scores,
// nrms.policy_step: learning from a log, on-policy policy gradient, ListMLE).  Included in digat_kernels.hip behind
// digat_pl_sample.inc, whose probability stage it runs (pl_cut_slate, pl_z_stage, pl_prob_stage: the bits of digat_pl_log_prob), and
// behind digat_list_softmax.inc / digat_list_pairwise.inc, whose two ends it reuses: lsm_score_stage in front, lpw_users_kernel
// (lsm_gather_users) and lsm_rows_kernel behind.
// users [G, d], rows [P, d], ids [G, M] int64, count [G] int32 (NULL: M), picks [G, S, k] int32 positions into the list, inv_t (f64).
//   Slot (g, j) is an ELEMENT exactly as in digat_list_softmax_fwd; score(g, j) = digat_dot_scores' bits; out_scores = the score at
//   elements, NaN elsewhere.  A position is LIVE when it is an element and its score is finite.  a_j = fl((double)score_j inv_t);
//   inv_t = fl(scale fl(1 / T)) is formed once by the caller.  From there on logp [G, S] f64 and step_logp [G, S, k] f32 are
//   digat_pl_log_prob's on a: a slate ends in front of its first entry that is negative, >= M, not live or repeated; w_j =
//   exp(max(a_j - a_max, -700)); Z_t = the sum of w over the live positions not picked before step t; step[t] = d_t - log Z_t.
// The gradient, a_max and the clamp held constant (exact while no live entry sits on the clamp).  With H_t = sum_{u < t} 1 / Z_u
// and n the slate's length:
//   dlogp / da_j = - w_j H_n              j live and not in the slate
//   dlogp / da_j = 1 - w_j H_{t+1}        j = pick(t)
//   dlogp / da_j = 0                      j not live
//   coef(g, j) = fl32(inv_t sum_s grad_logp[g, s] dlogp_s / da_j), exactly 0 at every slot that is not live.
//   d_users[g] = sum_j coef(g, j) rows[id_j], d_rows[p] = sum_{ids[g, j] = p} coef(g, j) users[g]: digat_list_softmax_bwd's two sums.
//
// One workgroup of 256 threads per list; the list's S slates run inside it in ascending s, so the order of every sum is fixed by
// (M, d, count, ids, the slates) alone: no floating-point atomics, no [G, S, M] workspace, the same bits from two calls and for a list
// alone or in a batch.
//   lpl_fwd_kernel   lsm_score_stage, then PlShared laid OVER the staged tile (dead once scoring ends; 21 040 of its 36 864 bytes):
//                    sh.a from the scores in registers by pl_stage_list's rule, then per slate pl_cut_slate + pl_prob_stage.
//   lpl_coef_kernel  sh.a from the saved scores (pl_stage_list), then per slate — skipped when it is empty or its grad_logp is 0 —
//                    pl_cut_slate + pl_z_stage; thread 0 builds H_{t+1} = fl(H_t + fl(1 / Z_t)), a serial prefix of at most 128
//                    reciprocals; every thread adds -fl(g fl(w_j H_n)) for its four positions to fp64 registers (sh.w holds 0 at the
//                    picked and the dead positions); thread t < n adds the picked position's own term fl(g fl(1 - fl(w_pick H_{t+1})))
//                    to an LDS accumulator (a slate's positions are distinct: one writer per slot, slates apart by barriers).
//                    The picked term is taken directly and not as -g w H_n + g (1 + w (H_n - H_{t+1})): the same number without
//                    the cancelling pair, at the same cost.  At the end coef = fl32(inv_t (registers + LDS)).
//                    Everything under `#pragma clang fp contract(off)`.
//   backward         lpl_coef_kernel -> workspace [G, M]; lpw_users_kernel with no per-list factor (grad_loss NULL: lambda is the
//                    coefficient) -> d_users; lsm_rows_kernel with the caller's sorted entry keys -> d_rows.
//
// The bound evaluate.list_pl_bound states for coef against evaluate.list_pl_host (numpy float64, math.fsum), derived.  u = 2^-53,
// n = the list's live positions, first order, relative to a term's size.  Device and twin form a, a_max, a - a_max and the clamp with
// the same roundings; logp and step_logp therefore carry digat_pl_sample.inc's pl_bound unchanged.  For coef:
//   w_j          exp correct to 1 ulp on either side:                                                   4
//   Z_t          digat_pl_sample.inc: the twin's fsum against at most n positive additions:              n + 4
//   1 / Z_t      one division on either side:                                                           n + 6
//   H            the device adds at most k positive terms in slate order, (k - 1); the twin's fsum, 1:     n + k + 6
//   g w H_n      two products on either side:                              4 + (n + k + 6) + 4 =         n + k + 14    of |g| w H_n
//   g (1 - w H)  x = w H: n + k + 12 of x; the difference and the product, 2 each side, of (1 + x):     n + k + 16    of |g| (1 + w H)
//   sum over s   a slot's terms go to the register chain (not picked) or the LDS chain (picked): at most S - 1 additions of at
//                most u times the absolute sum each, the last addition 1, the twin's fsum 1:            S + 1
//   inv_t        one product on either side:                                                            2
// Together (n + k + S + 19) u A with A(g, j) = |inv_t| sum_s |g_s| (1[j in slate s] + w_j H_n(s)) — the terms cancel across slates
// and, in a picked position, within one, so the error is relative to the ABSOLUTE sum, as lambda's is in digat_list_pairwise.inc; S
// stands in it because the slates are added one after the other.  One float32 rounding, or float32's subnormal spacing:
//   |coef - twin| <= 2^-24 |coef| + (n + k + S + 20) 2^-53 A + 2^-149                                  (20: 19 and the second order)
// Seen on an MI355X over the sweep of tests/test_hip_list_pl.py: the worst |coef - twin| is 0.987 of this bound (G = 65, M = 257,
// k = 128) — the float32 rounding alone; the float64 terms lie nine orders of magnitude below it.  logp: 0.093 of pl_bound.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   lpl_fwd_kernel     VGPRs 84   SGPRs 89   LDS 40960 B   scratch 0   occupancy 4 waves / SIMD (by LDS: the staged tile, PlShared laid over it)
//   lpl_coef_kernel    VGPRs 74   SGPRs 84   LDS 29232 B   scratch 0   occupancy 5 waves / SIMD (by LDS: PlShared and the picked sums)
// The kernels whose stages this file shares keep their lines: lsm_fwd_kernel 86 / 71 / 41248 / 3, lsm_users_kernel 52 / 58 / 20768 / 7,
// lpw_fwd_kernel 115 / 78 / 40992 / 3, lpw_users_kernel (grad_loss may now be NULL) 50 / 56 / 20736 / 7, pl_sample_kernel
// 32 / 64 / 37424 / 4, pl_log_prob_kernel (its cut now pl_cut_slate, its stage now pl_z_stage + the steps) 30 / 53 / 21040 / 7.
//
// Measured on an MI355X at d = 400 against index_select + bmm + a gather of the picks + the tail's logsumexp + a flipped logcumsumexp
// under autograd in fp32, chunked to 1 GiB of forward intermediates (tools/kbench.py list-pl; forward | forward + backward, ms):
// 4 096 lists of 1 024: 1.10 | 3.48 (k = 10, S = 1) to 1.41 | 4.31 (k = 100, S = 8) against 5.44 | 18.8 to 7.89 | 19.8, at a peak of
// 221 - 246 MiB beyond the inputs against 2.0 - 2.1 GiB; 4 096 x 128: 0.20 | 0.84 to 0.55 | 1.70 against 0.81 | 2.35 to 3.07 | 4.87.
// 64 lists — 64 workgroups on 256 CUs — do not lose, because the stock composition is launch-bound there (0.44 | 0.96 ms at any
// shape), but barely win with the backward at M = 1 024: 0.21 - 0.30 | 0.69 - 0.87 ms (the narrowest: k = 100, S = 8, 0.872 against
// 0.969); 64 x 128: 0.08 - 0.15 | 0.38 - 0.55 against 0.44 | 0.89.  The S slates of a list run one after the other in its workgroup:
// an S-parallel grid was not built.  tools/kbench.py policy (planted-signal corpus, NRMS at d = 64, random titles, 300 steps of 64
// lists): nrms.fit_policy 10.9 ms a step against fit_ranker's 2.5 and the click softmax's 2.4; it raises the nDCG@10 of its own
// sampled training slates (0.1585 -> 0.1922) and does not move held-out clicks (nDCG@10 0.1539 against 0.1569 and 0.1600; every
// paired interval holds 0).  nrms.fit_from_logs: 4.7 ms a step, the graph-free first scoring pass 1.1 ms (23 %) of it; on the log it
// trained on, clipped IPS 0.34 -> 0.61, while its own slates earn 0.4830 -> 0.4903: mostly the log fitted (DESIGN section 8).

struct LplArgs {
    LsmArgs l;                           // users, rows, ids, count, G, P, M, d; scores out
    PlArgs p;                            // scores (backward in), count, M, k, inv_t, S, picks_in, out_logp, out_step
    const double* grad_logp;             // [G, S]
    float* coef;                         // [G, M]
};

static_assert(LSM_MAX_M == PL_MAX_M && LSM_SLABS == 4, "a thread's four scoring slots are its four positions of PlShared");
static_assert(sizeof(PlShared) <= LSM_SLAB * LSM_LD * sizeof(float), "PlShared lives in the staged tile");

__global__ void __launch_bounds__(256) lpl_fwd_kernel(const LplArgs a) {
    __shared__ float4 su4[LSM_MAX_D / 4];
    __shared__ float4 tile4[LSM_SLAB * LSM_LD / 4];
    __shared__ long long sid[LSM_SLAB];
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
    for (long s = 0; s < a.p.S; ++s) {
        const size_t row = (size_t)g * (size_t)a.p.S + (size_t)s;
        const int n_out = pl_cut_slate(a.p, row, sh);                   // its first barrier stands behind sh.a
        pl_prob_stage(sh, a.p.k, n_out, a.p.out_logp + row, a.p.out_step + row * a.p.k);
    }
}

__global__ void __launch_bounds__(256) lpl_coef_kernel(const LplArgs a) {
#pragma clang fp contract(off)
    __shared__ PlShared sh;
    __shared__ double picked[PL_MAX_M];              // the picked positions' own terms, summed over the slates
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    pl_stage_list(a.p, g, sh);
    double acc[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        acc[h] = 0.0;
        picked[tid + 256 * h] = 0.0;
    }
    for (long s = 0; s < a.p.S; ++s) {
        const size_t row = (size_t)g * (size_t)a.p.S + (size_t)s;
        const double gs = a.grad_logp[row];
        const int n_out = pl_cut_slate(a.p, row, sh);
        if (n_out == 0 || gs == 0.0) continue;       // workgroup-uniform: an empty slate has logp 0, a zero weight moves nothing
        pl_z_stage(sh, n_out);
        if (tid == 0) {
            double H = 0.0;
            for (int t = 0; t < n_out; ++t) {
                H = H + 1.0 / sh.z[t];
                sh.v[t] = H;                         // H_{t+1}
            }
        }
        __syncthreads();
        const double Hn = sh.v[n_out - 1];
#pragma unroll
        for (int h = 0; h < 4; ++h) acc[h] = acc[h] - gs * (sh.w[tid + 256 * h] * Hn);
        if (tid < n_out) {
            const int p = sh.pick[tid];
            picked[p] = picked[p] + gs * (1.0 - sh.wpick[tid] * sh.v[tid]);
        }
        // the next slate's first writes to sh.w, sh.wpick and sh.v stand behind pl_cut_slate's barriers; sh.pick[tid] is this thread's own
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int j = tid + 256 * h;
        if (j < a.p.M) a.coef[(size_t)g * a.p.M + j] = sh.a[j] > -INFINITY ? (float)(a.p.inv_t * (acc[h] + picked[j])) : 0.f;
    }
}

static int lpl_pl_check(const void* picks, int64_t G, int M, int k, double inv_t, int64_t S) {
    if (!picks || ((uintptr_t)picks & 3) || G < 0) return DIGAT_ERR_ARG;
    if (!(inv_t > 0.0) || !(inv_t * 3.4028234663852886e38 < INFINITY)) return DIGAT_ERR_ARG;       // a NaN fails the first comparison
    if (k < 1 || k > PL_MAX_K || M < 1 || M > PL_MAX_M || S < 1 || G * (int64_t)M > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

static int lpl_list_check(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t P, int d) {
    if (!users || (!rows && P > 0) || !ids || P < 0) return DIGAT_ERR_ARG;
    if (((uintptr_t)users & 3) || ((uintptr_t)rows & 3) || ((uintptr_t)ids & 7) || ((uintptr_t)count & 3)) return DIGAT_ERR_ARG;
    if (d < 1 || d > LSM_MAX_D || P > 0x80000000L) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

static LplArgs lpl_args(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t S, const int32_t* picks) {
    LplArgs a{};
    a.l.count = count; a.l.G = (long)G; a.l.M = M;
    a.p.scores = scores; a.p.count = count; a.p.M = M; a.p.k = k; a.p.inv_t = inv_t; a.p.S = (long)S; a.p.picks_in = picks;
    return a;
}

extern "C" {

size_t digat_list_pl_workspace_bytes(int64_t lists, int m) { return digat_list_softmax_workspace_bytes(lists, m); }

int digat_list_pl_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                      const int32_t* picks, int64_t samples, int k, double inv_t, double* out_logp, float* out_step, float* out_scores,
                      void* stream) {
    if (!out_logp || !out_step || !out_scores || ((uintptr_t)out_logp & 7) || ((uintptr_t)out_step & 3) || ((uintptr_t)out_scores & 3))
        return DIGAT_ERR_ARG;
    int rc = lpl_list_check(users, rows, ids, count, P, d);
    if (rc == DIGAT_OK) rc = lpl_pl_check(picks, G, M, k, inv_t, samples);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    LplArgs a = lpl_args(nullptr, count, G, M, k, inv_t, samples, picks);
    a.l.users = users; a.l.rows = rows; a.l.ids = ids; a.l.P = (long)P; a.l.d = d; a.l.scores = out_scores;
    a.p.out_logp = out_logp; a.p.out_step = out_step;
    hipLaunchKernelGGL(lpl_fwd_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_pl_scores_bwd(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples,
                        const int32_t* picks, const double* grad_logp, float* out_grad, void* stream) {
    if (!scores || !grad_logp || !out_grad) return DIGAT_ERR_ARG;
    if (((uintptr_t)scores & 3) || ((uintptr_t)count & 3) || ((uintptr_t)grad_logp & 7) || ((uintptr_t)out_grad & 3)) return DIGAT_ERR_ARG;
    const int rc = lpl_pl_check(picks, G, M, k, inv_t, samples);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    LplArgs a = lpl_args(scores, count, G, M, k, inv_t, samples, picks);
    a.grad_logp = grad_logp; a.coef = out_grad;
    hipLaunchKernelGGL(lpl_coef_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_list_pl_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                      const float* scores, const int32_t* picks, int64_t samples, int k, double inv_t, const double* grad_logp,
                      const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!scores || !grad_logp || !d_users || ((uintptr_t)scores & 3) || ((uintptr_t)grad_logp & 7) || ((uintptr_t)d_users & 3) ||
        ((uintptr_t)d_rows & 3) || ((uintptr_t)entry_keys & 7))
        return DIGAT_ERR_ARG;
    int rc = lpl_list_check(users, rows, ids, count, P, d);
    if (rc == DIGAT_OK) rc = lpl_pl_check(picks, G, M, k, inv_t, samples);
    if (rc != DIGAT_OK) return rc;
    if (d_rows && (E < 0 || E > G * (int64_t)M || (E > 0 && !entry_keys))) return DIGAT_ERR_ARG;
    if (G > 0 && (!workspace || (((uintptr_t)workspace) & 3))) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_list_pl_workspace_bytes(G, M)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LplArgs a = lpl_args(scores, count, G, M, k, inv_t, samples, picks);
    a.grad_logp = grad_logp; a.coef = (float*)workspace;
    LpwArgs b{};                                                      // the gather and the rows kernel, from the coefficients as they stand
    b.l.users = users; b.l.rows = rows; b.l.ids = ids; b.l.count = count;
    b.l.G = (long)G; b.l.P = (long)P; b.l.M = M; b.l.d = d;
    b.l.keys = entry_keys; b.l.E = G > 0 ? (long)E : 0;
    b.l.coef = (float*)workspace; b.l.d_users = d_users; b.l.d_rows = d_rows;
    b.lambda = (float*)workspace;
    if (G > 0) {
        hipLaunchKernelGGL(lpl_coef_kernel, dim3((unsigned)G), dim3(256), 0, st, a);
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
