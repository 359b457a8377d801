// digat_pl_expect.inc — the control variate of a doubly robust off-policy value: for every logged slate and every step t, the
// expectation of a per-item value under the TARGET's conditional distribution over the items still on the list,
//   m_t = sum_{j left at t} w_j v_j / sum_{j left at t} w_j
// (evaluate.pl_expect; util.slate_step_values, evaluate.off_policy_steps, util.off_policy_report).  Included in digat_kernels.hip
// behind digat_pl_sample.inc, whose stages it runs unchanged: pl_stage_list, pl_cut_slate, pl_prob_stage (pl_z_stage inside it).
//
// pl_expect_kernel, one workgroup of 256 threads per (list g, slate s), as pl_log_prob_kernel:
//   the list, the cut and the probability are pl_log_prob_kernel's own calls on the same LDS image: out_logp and out_step are
//           digat_pl_log_prob's bit for bit and out_len[g, s] is what pl_cut_slate returns.
//   values  v_p = (double)values[g][p] where that float is finite, else 0; read from global memory, never staged.
//   behind pl_z_stage sh.w holds the unpicked weights (the picked slots 0) and sh.wpick / sh.z the picked weights and Z_t:
//           R_v = the sum of fl(w_p v_p) over a thread's four positions in ascending order, wave_sum_f64's butterfly, the four
//           waves ((0 + 1) + 2) + 3 — the order of R in pl_z_stage; thread t < n_out keeps fl(wpick_t v_pick(t)) in LDS and writes
//           out_value[t], the float32 value it used; thread 0 walks back from the end of the slate, N_t = fl(N_{t+1} +
//           fl(wpick_t v_pick(t))) with N_{n_out} = R_v: the suffix sum beside Z_t, again with no subtraction; thread t:
//           out_mean[t] = fl(N_t / Z_t).  At and beyond the slate's length out_mean and out_value are 0.
// All of it under `#pragma clang fp contract(off)`: never an fma.  Every order of addition depends on (M, count, the slate) alone;
// no atomics, no workspace, nothing read back.  Extra LDS beside PlShared: one double[PL_MAX_K].
//
// The bound evaluate.pl_expect_bound states, derived.  u = 2^-53; n the live positions of the list; B_t = sum_{left} w_j |v_j|,
// A_t = B_t / Z_t >= |m_t|.  digat_pl_sample.inc: the arguments of exp agree bit for bit on both sides and exp is correct to 1 ulp
// on either: the weights differ by at most 4u relatively.  A float32 value is exact in float64 on both sides.  Each side rounds a
// product once: the products differ by at most (4 + 2) u w_j |v_j|.  The twin's numerator is the correctly rounded sum (fsum):
// u B_t; the device adds at most n non-zero signed terms (a position that is not live adds an exact 0), each addition at most u of
// a partial sum whose magnitude never exceeds B_t: (n - 1) u B_t.  The numerators differ by at most (n + 6) u B_t.
// digat_pl_sample.inc again: the two Z_t differ by at most (n + 4) u Z_t.  With N / Z - N' / Z' = (N - N') / Z + N' (1 / Z - 1 / Z')
// the exact quotients differ by at most (n + 6) u A_t + (n + 4) u |m_t| <= (2n + 10) u A_t; each side then rounds the division,
// u |m_t| on either: 2^-52 |m_t|.  The terms of second order are below (2n + 10) (n + 6) u^2 A_t < 2^-31 u A_t at n <= 1024; the
// constant that is stated is c = 12:   (2n + 12) 2^-53 A_t + 2^-52 |m_t|.
// Its domain: every non-zero product w_j |v_j| is a normal float64 (>= 2^-1022).  A weight is at least e^-700, so |v_j| >= 2^-12 or
// v_j = 0 is enough whatever the spread; below that a product on the clamp is rounded absolutely (2^-1075), not relatively.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup, scratch 0:
//   pl_expect_kernel     VGPRs 35   SGPRs 64   LDS 22064 B   occupancy 7 waves / SIMD (by LDS, as pl_log_prob_kernel: 21040 + 1024)
// pl_log_prob_kernel, pl_sample_kernel, lpl_fwd_kernel and lpl_coef_kernel keep their lines and their code: PlArgs is untouched (four
// more pointers at its end moved lpl_coef_kernel, which embeds it, from 74 to 94 VGPRs), so the values and the three further outputs
// travel as a second kernel argument, PlExpectArgs, which pl_launch passes on behind PlArgs.

struct PlExpectArgs {             // pl_expect_kernel's second argument: PlArgs and every kernel that takes it alone stay as they are
    const float* values;         // [G, M]
    double* out_mean;            // [G, S, k]
    float* out_value;            // [G, S, k]
    int32_t* out_len;            // [G, S]
};

// fl(w v) with v = (double)x where the float x is finite, else 0.
__device__ __forceinline__ double pl_weighted(double w, float x) {
#pragma clang fp contract(off)
    const double v = x - x == 0.f ? (double)x : 0.0;
    return w * v;
}

__global__ void __launch_bounds__(256) pl_expect_kernel(const PlArgs a, const PlExpectArgs e) {
#pragma clang fp contract(off)
    __shared__ PlShared sh;
    __shared__ double num[PL_MAX_K];                 // fl(wpick_t v_pick(t)), then N_t
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = a.g0 + blockIdx.x, s = a.s0 + blockIdx.y;
    const size_t row = (size_t)g * (size_t)a.S + (size_t)s;
    pl_stage_list(a, g, sh);
    const int n_out = pl_cut_slate(a, row, sh);
    pl_prob_stage(sh, a.k, n_out, a.out_logp + row, a.out_step + row * a.k);
    // sh.w, sh.wpick and sh.z stand behind pl_z_stage's last barrier; sh.part was last read in front of it
    const float* values = e.values + (size_t)g * a.M;
    double r = 0.0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int p = tid + 256 * h;
        const double term = p < a.M ? pl_weighted(sh.w[p], values[p]) : 0.0;       // no read beyond the row
        r = h == 0 ? term : r + term;
    }
    r = wave_sum_f64(r);
    if (lane == 0) sh.part[wave] = r;
    if (tid < a.k) {
        float x = 0.f;
        if (tid < n_out) {
            const float xp = values[sh.pick[tid]];                                 // a slate's entries are live: inside the row
            x = xp - xp == 0.f ? xp : 0.f;
            num[tid] = pl_weighted(sh.wpick[tid], x);
        }
        e.out_value[row * a.k + tid] = x;
    }
    if (tid == 0) e.out_len[row] = n_out;
    __syncthreads();
    if (tid == 0) {
        double nt = ((sh.part[0] + sh.part[1]) + sh.part[2]) + sh.part[3];
        for (int t = n_out - 1; t >= 0; --t) {
            nt = nt + num[t];
            num[t] = nt;
        }
    }
    __syncthreads();
    if (tid < a.k) e.out_mean[row * a.k + tid] = tid < n_out ? num[tid] / sh.z[tid] : 0.0;
}

extern "C" {

int digat_pl_expect(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples, const int32_t* picks,
                    const float* values, double* out_logp, float* out_step, double* out_mean, float* out_value, int32_t* out_len,
                    void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!picks || !values || !out_mean || !out_value || !out_len) return DIGAT_ERR_ARG;
    if (((uintptr_t)picks & 3) || ((uintptr_t)count & 3) || ((uintptr_t)values & 3) || ((uintptr_t)out_mean & 7) || ((uintptr_t)out_value & 3) ||
        ((uintptr_t)out_len & 3))
        return DIGAT_ERR_ARG;
    const int rc = pl_check(scores, G, M, k, inv_t, samples, 0, out_logp, out_step);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    const PlArgs a{scores, count, 0, M, k, inv_t, 0u, 0, 0, (long)samples, nullptr, picks, nullptr, nullptr, out_logp, out_step};
    return pl_launch(pl_expect_kernel, a, G, samples, (hipStream_t)stream, PlExpectArgs{values, out_mean, out_value, out_len});
}

}  // extern "C"
