// digat_list_pairwise.inc — the pairwise nDCG loss (LambdaRank / LambdaLoss) over a user's OWN list of news, and its gradients, without
// a [G, M, M] tensor ever reaching memory (evaluate.list_pairwise, evaluate.pairwise_scores, nrms.rank_step).  Included in
// digat_kernels.hip behind digat_list_softmax.inc, whose two ends it reuses: lsm_score_stage (the gather-dot scoring of a list) in front,
// lsm_gather_users and lsm_rows_kernel (the deterministic backward from a [G, M] coefficient array) behind.
// users [G, d], rows [P, d], ids [G, M] int64, count [G] int32 (NULL: M), gain [G, M] f32, discount [M] f64, scale.
//   Slot (g, j) is an ELEMENT exactly as in digat_list_softmax_fwd: j < clamp(count[g], 0, M) and 0 <= ids[g, j] < P; a repeated id is
//   two elements.  score(g, j) = the fp32 fmaf chain — digat_dot_scores' bits —, x = fl32(scale * score), widened to double.
//   digat_list_pairwise_scores_fwd takes the scores as given: a slot is an element when j < clamp(count[g], 0, M) and its score is no NaN.
//   An element is LABELLED when its gain is finite and >= 0 (NaN, +-inf, negative: no label) and its x is no NaN (a chain that
//   overflowed to inf - inf; the scores entry, fed the fused entry's scores, sees the same slots).  Anything else takes part in
//   nothing: no rank, no pair, gradient exactly 0.  n = the labelled elements of the list.
//   r_i = the labelled elements that order before i under (x descending, slot ascending), t_i = the same under (gain descending, slot
//   ascending): integers.  D(r) = discount[r], READ from the caller's table (evaluate.ndcg_discount: numpy's 1 / log2(2 + r), zero from
//   r = k on when truncated) — the kernel takes no logarithm for it, so the device and the numpy twin hold the same discount bits.
//   idcg = sum gain_i D(t_i), dcg = sum gain_i D(r_i); the list is VALID when idcg > 0; ndcg = dcg / idcg (0 when invalid).
//   For every ordered pair (i, j) of labelled elements with gain_i > gain_j:  w_ij = ((gain_i - gain_j) |D(r_i) - D(r_j)|) / idcg, in
//   that operation order in fp64 — a constant: no gradient flows through the ranks.  With t = x_i - x_j,
//   sp(t) = max(-t, 0) + log1p(exp(-|t|)), sg(t) = 1 / (1 + exp(t)):
//   loss[g]      = sum_pairs w_ij sp(t)                                                                  (0 when invalid)
//   lambda[g, i] = scale ( - sum_{j: gain_i > gain_j} w_ij sg(x_i - x_j) + sum_{j: gain_j > gain_i} w_ji sg(x_j - x_i) ), rounded to fp32
//                  once; exactly 0 at every slot that is no labelled element of a valid list.
//   Every output byte is written whatever count holds.
// Backward, given grad_loss [G] and the forward's lambda: coef(g, j) = fl32(grad_loss[g] lambda[g, j]) -> workspace [G, M];
//   d_users and d_rows are digat_list_softmax_bwd's two sums over coef, in its order.
//
// Forward, one launch, one workgroup of 256 threads per list, lanes own slots tid + 256 s:
//   lpw_fwd_kernel     lsm_score_stage, then the pair stage in the LDS of the staged tile.
//   lpw_scores_kernel  the pair stage on given scores.
//   lpw_pair_stage     LDS: one 16-byte record per slot — x (fp32), gain (fp32; NaN marks "not labelled": every compare with it is
//                      false, so such a slot drops out of the counts and of the pairs by itself), D(r) (fp64) —, 16 KB at M = 1 024.
//                      (1) r and t by counting: a thread walks j ascending for each of its slots; every lane of a wave reads the same
//                      record (an LDS broadcast read), two compares and two integer adds per record.  (2) D(r_i) from the table into
//                      the record; idcg and dcg: a lane adds its slots in ascending order, then lsm_block_sum.  (3) the pair loop: a
//                      thread walks j ascending for each of its slots and accumulates its own lambda and, from the side with the
//                      larger gain, the pair's share of the loss, in fp64 registers: every unordered pair is visited from both sides —
//                      twice the arithmetic, no atomics.  One exp serves sp and sg: e = exp(-|t|), sg = (t >= 0 ? e : 1) / (1 + e).
//                      A pair with w == 0 (equal gains: never reached; both ranks past a truncation) pays no exp.  The loss: per slot
//                      in j order, the thread's slots in ascending order, then lsm_block_sum.
//                      What was tried for click labels (almost all pairs negative against negative): the per-lane skip above, alone.
//                      A wave whose 64 slots are all negatives does arithmetic only at the list's few positives; a wave that holds a
//                      positive walks the whole list for that lane.  Compacting the labelled elements by gain class first was NOT
//                      tried; tools/kbench.py list-pairwise measures both kinds of gains.
// Backward, two launches (one when d_rows is NULL):
//   lpw_users_kernel   coef -> workspace and LDS, then lsm_gather_users (a list whose coefficients are all zero is not gathered);
//                      the "small kernel that writes coef" lives in front of the gather, as in lsm_users_kernel: one launch fewer.
//   lsm_rows_kernel    as it is, through LsmArgs and the caller's sorted entry_keys.
// No floating-point atomics; the order of every sum is fixed by M, count, ids and gain alone; a list's outputs depend on that list alone.
//
// Error against the contract evaluated exactly on the same bits (evaluate.list_pairwise_host: numpy float64, math.fsum).  Device and
// twin share x, gain, the table and the ranks, hence t = x_i - x_j, gain_i - gain_j, |D - D| and their product bit for bit (the same
// fp64 operations in the same order).  In units of 2^-53, relative, first order:
//   idcg, dcg     n products of one rounding each and a sum of positive terms of depth <= n - 1:   n        (twin: product + fsum: 2)
//   w             idcg's error and the quotient's rounding:                                          n + 1    (twin: 3)
//   sp            exp 2 (the sibling file's 2^-52 per library call), carried through log1p <= 2, log1p 2, the sum 1:   7   (twin: 7)
//   sg            exp 2, 1 + e: 1 + 2, the quotient 1:                                               6        (twin: 6)
//   w sp, w sg    one product:                                                                       1        (twin: 1)
//   the sum       loss: a slot's pairs in j order <= n - 1, the thread's four slots 3, the butterfly 6, the waves 3: n + 11;
//                 lambda: one sequence over j, <= n - 1, and the product with scale 1: n              (twin: fsum 1, scale 1)
// loss: (n + 1) + 7 + 1 + (n + 11) = 2 n + 20 on the device, 12 in the twin: 2 n + 32 = c(n).  lambda: 2 n + 8 and 12: below c(n).
// ndcg = dcg / idcg: 2 n + 1 and 5: below c(n).  loss and ndcg are sums of positive terms, so the error is relative to the value;
// lambda's two halves cancel, so it is relative to the ABSOLUTE sum A_i = scale sum_j w sg.  Each is rounded to fp32 once, u = 2^-24
// relative — or, below fp32's normal range (a lambda of e^-300 flushes to a subnormal or to zero), 2^-150 absolute:
//   |loss - twin|     <= u |loss| + c(n) 2^-53 loss (1 + u) + 2^-149
//   |ndcg - twin|     <= u ndcg + c(n) 2^-53 ndcg (1 + u) + 2^-149
//   |lambda_i - twin| <= u |lambda_i| + c(n) 2^-53 A_i (1 + u) + 2^-149                 c(n) = 2 n + 32
// The subnormal term stands beside the relative ones because fp32 has no relative accuracy there.  evaluate.list_pairwise_bound is this formula;
// tests/test_hip_list_pairwise.py holds the kernels to it.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   lpw_fwd_kernel     VGPRs 115  SGPRs 78   LDS 40992 B   scratch 0   occupancy 3 waves / SIMD (by LDS: the staged tile, reused by the pair stage)
//   lpw_scores_kernel  VGPRs 116  SGPRs 69   LDS 16416 B   scratch 0   occupancy 4 waves / SIMD
//   lpw_users_kernel   VGPRs 50   SGPRs 56   LDS 20736 B   scratch 0   occupancy 7 waves / SIMD
// and digat_list_softmax.inc's two kernels before and after their scoring stage and gather became __device__ functions shared with this file:
//   lsm_fwd_kernel     before VGPRs 78   SGPRs 82   LDS 41248 B   scratch 0   occupancy 3      after VGPRs 86   SGPRs 71   LDS 41248 B   scratch 0   occupancy 3
//   lsm_users_kernel   before VGPRs 52   SGPRs 58   LDS 20768 B   scratch 0   occupancy 7      after VGPRs 52   SGPRs 58   LDS 20768 B   scratch 0   occupancy 7
//
// Measured on an MI355X at d = 400 against index_select + bmm + argsort ranks + the [g, M, M] differences + softplus under autograd in
// fp32, chunked to 1 GiB intermediates (tools/kbench.py list-pairwise): 4 096 lists of 1 024: forward 9.5 ms (click gains) / 21.3 ms
// (all-distinct gains) against 94, forward + backward 11.6 / 23.2 ms against 137 at a peak of 212 MiB beyond the inputs against
// 4.5 GiB; 4 096 x 128: 0.72 / 0.84 and 1.38 / 1.44 ms against 2.2 and 4.2.  64 lists of 1 024 — 64 workgroups on 256 CUs, a million
// pair visits each — lose: 1.87 / 2.78 ms forward against 1.66, 2.53 / 3.40 ms with the backward against 2.45 (DESIGN section 8).

static_assert(LSM_SLABS == 4, "lpw_pair_stage's depth count takes four slots per thread");

struct LpwArgs {
    LsmArgs l;                           // users, rows, ids, count, G, P, M, d, scale; loss, valid, scores out; grad_loss, keys, coef, d_users, d_rows
    const float* in_scores;              // [G, M]  lpw_scores_kernel
    const float* gain;                   // [G, M]
    const double* discount;              // [M]
    float* ndcg;                         // [G]     forward out
    float* lambda;                       // [G, M]  forward out, backward in
};

struct __align__(16) LpwSlot {
    float x, gain;                       // gain NaN: the slot is no labelled element
    double D;                            // discount[r]
};

static_assert(sizeof(LpwSlot) == 16 && LSM_MAX_M * sizeof(LpwSlot) <= LSM_SLAB * LSM_LD * sizeof(float), "the pair stage lives in the staged tile");

// Whole workgroup.  sc[s] / el[s]: the score and the element flag of the thread's slot s LSM_SLAB + tid; P = LSM_MAX_M records of LDS that
// nobody else is using any more; red = four doubles.  Writes loss, ndcg, valid and lambda of list g.
__device__ __forceinline__ void lpw_pair_stage(const LpwArgs& a, long g, const float (&sc)[LSM_SLABS], const bool (&el)[LSM_SLABS], LpwSlot* P,
                                               double* red) {
#pragma clang fp contract(off)                                        // no fused multiply-add: the two forward kernels round alike
    const int tid = threadIdx.x, M = a.l.M;
    const float qnan = __uint_as_float(0x7fc00000u);
    float xf[LSM_SLABS], gf[LSM_SLABS];
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int i = s * LSM_SLAB + tid;
        xf[s] = 0.f;
        gf[s] = qnan;
        if (i < M && el[s]) {
            const float x = a.l.scale * sc[s], gn = a.gain[g * M + i];
            if (x == x && gn >= 0.f && gn - gn == 0.f) {              // labelled: x no NaN, the gain finite and not negative
                xf[s] = x;
                gf[s] = gn;
            }
        }
        P[i].x = xf[s];
        P[i].gain = gf[s];
        P[i].D = 0.0;
    }
    __syncthreads();

    // (1) ranks by counting
    int r[LSM_SLABS], t[LSM_SLABS];
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        r[s] = 0;
        t[s] = 0;
        if (s * LSM_SLAB >= M) continue;                              // workgroup-uniform
        const int i = s * LSM_SLAB + tid;
        const float xi = xf[s], gi = gf[s];
        for (int j = 0; j < M; ++j) {
            const float2 e = *(const float2*)&P[j];                   // the same record in every lane
            const bool lab = e.y == e.y, first = j < i;
            r[s] += (lab && (e.x > xi || (e.x == xi && first))) ? 1 : 0;
            t[s] += (e.y > gi || (e.y == gi && first)) ? 1 : 0;        // a NaN gain, here or there, counts nowhere
        }
    }
    // (2) D(r) into the records, idcg and dcg
    double Di[LSM_SLABS], si = 0.0, sd = 0.0;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        Di[s] = 0.0;
        if (gf[s] == gf[s]) {                                         // labelled: r, t < n <= M
            Di[s] = a.discount[r[s]];
            si += (double)gf[s] * a.discount[t[s]];
            sd += (double)gf[s] * Di[s];
            P[s * LSM_SLAB + tid].D = Di[s];
        }
    }
    const double idcg = lsm_block_sum(si, red), dcg = lsm_block_sum(sd, red);     // behind barriers: the records are complete
    const bool valid = idcg > 0.0;
    // (3) the pairs
    double loss = 0.0;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int i = s * LSM_SLAB + tid;
        double lam = 0.0, ls = 0.0;
        if (valid && s * LSM_SLAB < M) {                              // workgroup-uniform
            const float gi = gf[s];
            const double xi = (double)xf[s], gid = (double)gi, Dr = Di[s];
            for (int j = 0; j < M; ++j) {
                const LpwSlot e = P[j];
                const bool up = gi > e.gain, down = e.gain > gi;      // both false where either slot is not labelled
                if (up || down) {
                    const double hi = up ? gid : (double)e.gain, lo = up ? (double)e.gain : gid;
                    const double w = ((hi - lo) * fabs(up ? Dr - e.D : e.D - Dr)) / idcg;
                    if (w != 0.0) {
                        const double tt = up ? xi - (double)e.x : (double)e.x - xi;
                        const double ex = exp(-fabs(tt));
                        const double sg = (tt >= 0.0 ? ex : 1.0) / (1.0 + ex);
                        if (up) {
                            lam -= w * sg;
                            ls += w * (fmax(-tt, 0.0) + log1p(ex));
                        } else {
                            lam += w * sg;
                        }
                    }
                }
            }
        }
        loss += ls;
        if (i < M) a.lambda[g * M + i] = valid && gf[s] == gf[s] ? (float)((double)a.l.scale * lam) : 0.f;
    }
    loss = lsm_block_sum(loss, red);
    if (tid == 0) {
        a.l.loss[g] = valid ? (float)loss : 0.f;
        a.ndcg[g] = valid ? (float)(dcg / idcg) : 0.f;
        a.l.valid[g] = valid ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) lpw_fwd_kernel(const LpwArgs a) {
    __shared__ float4 su4[LSM_MAX_D / 4];
    __shared__ float4 tile4[LSM_SLAB * LSM_LD / 4];
    __shared__ long long sid[LSM_SLAB];
    __shared__ double red[4];
    const long g = blockIdx.x;
    const int cnt = lsm_count(a.l, g);
    float sc[LSM_SLABS];
    bool el[LSM_SLABS];
    lsm_score_stage(a.l, g, cnt, su4, tile4, sid, sc, el);              // its last read of the tile is behind a barrier
    lpw_pair_stage(a, g, sc, el, (LpwSlot*)tile4, red);
}

__global__ void __launch_bounds__(256) lpw_scores_kernel(const LpwArgs a) {
    __shared__ LpwSlot P[LSM_MAX_M];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = lsm_count(a.l, g);
    float sc[LSM_SLABS];
    bool el[LSM_SLABS];
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j = s * LSM_SLAB + tid;
        sc[s] = j < cnt ? a.in_scores[g * a.l.M + j] : 0.f;
        el[s] = j < cnt && sc[s] == sc[s];
    }
    lpw_pair_stage(a, g, sc, el, P, red);
}

__global__ void __launch_bounds__(256) lpw_users_kernel(const LpwArgs a) {
    __shared__ long long sid[LSM_MAX_M];
    __shared__ float scoef[LSM_MAX_M];
    __shared__ float part[4][LSM_MAX_D];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = lsm_count(a.l, g);
    const float gl = a.l.grad_loss ? a.l.grad_loss[g] : 1.f;          // NULL: lambda is the coefficient itself (digat_list_pl.inc)
    bool live = false;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j = s * LSM_SLAB + tid;
        const long long id = j < a.l.M ? lsm_id(a.l, g, j, cnt) : -1;
        float lam = 0.f;
        if (id >= 0) lam = a.lambda[g * a.l.M + j];
        const float cf = lam != 0.f ? gl * lam : 0.f;                 // a zero lambda stays a zero whatever grad_loss holds
        sid[j] = id;
        scoef[j] = cf;
        live = live || cf != 0.f;
        if (j < a.l.M) a.l.coef[g * a.l.M + j] = cf;
    }
    const bool any = __syncthreads_or(live ? 1 : 0) != 0;             // the barrier behind sid and scoef
    lsm_gather_users(a.l, g, cnt, any, sid, scoef, part);
}

static int lpw_check(const float* gain, const double* discount, int64_t G, int M) {
    if (!gain || !discount || G < 0) return DIGAT_ERR_ARG;
    if (M < 1 || M > LSM_MAX_M || G * (int64_t)M > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

extern "C" {

size_t digat_list_pairwise_workspace_bytes(int64_t lists, int m) { return digat_list_softmax_workspace_bytes(lists, m); }

int digat_list_pairwise_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* gain,
                            const double* discount, int64_t G, int64_t P, int M, int d, float scale, float* out_loss, float* out_ndcg,
                            int32_t* out_valid, float* out_scores, float* out_lambda, void* stream) {
    if (!users || (!rows && P > 0) || !ids || !out_loss || !out_ndcg || !out_valid || !out_scores || !out_lambda || P < 0) return DIGAT_ERR_ARG;
    const int rc = lpw_check(gain, discount, G, M);
    if (rc != DIGAT_OK) return rc;
    if (d < 1 || d > LSM_MAX_D || P > 0x80000000L) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    LpwArgs a{};
    a.l.users = users; a.l.rows = rows; a.l.ids = ids; a.l.count = count;
    a.l.G = (long)G; a.l.P = (long)P; a.l.M = M; a.l.d = d; a.l.scale = scale;
    a.l.loss = out_loss; a.l.valid = out_valid; a.l.scores = out_scores;
    a.gain = gain; a.discount = discount; a.ndcg = out_ndcg; a.lambda = out_lambda;
    hipLaunchKernelGGL(lpw_fwd_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_list_pairwise_scores_fwd(const float* scores, const int32_t* count, const float* gain, const double* discount, int64_t G, int M,
                                   float scale, float* out_loss, float* out_ndcg, int32_t* out_valid, float* out_lambda, void* stream) {
    if (!scores || !out_loss || !out_ndcg || !out_valid || !out_lambda) return DIGAT_ERR_ARG;
    const int rc = lpw_check(gain, discount, G, M);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    LpwArgs a{};
    a.l.count = count; a.l.G = (long)G; a.l.M = M; a.l.scale = scale;
    a.l.loss = out_loss; a.l.valid = out_valid;
    a.in_scores = scores; a.gain = gain; a.discount = discount; a.ndcg = out_ndcg; a.lambda = out_lambda;
    hipLaunchKernelGGL(lpw_scores_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_list_pairwise_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                            const float* lambda, const float* grad_loss, const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!users || (!rows && P > 0) || !ids || !lambda || !grad_loss || !d_users || G < 0 || P < 0) return DIGAT_ERR_ARG;
    if (M < 1 || M > LSM_MAX_M || d < 1 || d > LSM_MAX_D || G * (int64_t)M > 0x7fffffffL || P > 0x80000000L) return DIGAT_ERR_SHAPE;
    if (d_rows && (E < 0 || E > G * (int64_t)M || (E > 0 && !entry_keys))) return DIGAT_ERR_ARG;
    if (G > 0 && (!workspace || (((uintptr_t)workspace) & 3))) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_list_pairwise_workspace_bytes(G, M)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LpwArgs a{};
    a.l.users = users; a.l.rows = rows; a.l.ids = ids; a.l.count = count;
    a.l.G = (long)G; a.l.P = (long)P; a.l.M = M; a.l.d = d;
    a.l.grad_loss = grad_loss; a.l.keys = entry_keys; a.l.E = G > 0 ? (long)E : 0;
    a.l.coef = (float*)workspace; a.l.d_users = d_users; a.l.d_rows = d_rows;
    a.lambda = const_cast<float*>(lambda);
    if (G > 0) {
        hipLaunchKernelGGL(lpw_users_kernel, dim3((unsigned)G), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    if (d_rows && P > 0) {                                            // G == 0: no entry, every row zero
        hipLaunchKernelGGL(lsm_rows_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, a.l);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

}  // extern "C"
