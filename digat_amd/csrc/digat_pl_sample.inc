// digat_pl_sample.inc — stochastic lists: Plackett-Luce slates drawn from a user's own list with the probability of what was drawn
// (evaluate.pl_sample / pl_log_prob; util.sample_lists, util.slate_log_prob, recommend(sample=): exploration, logs with propensities,
// off-policy evaluation).  Included at the end of digat_kernels.hip, behind digat_eval.inc (wave_sum_f64), the dropout hash (hash32:
// a draw's word is digat_bootstrap.inc's construction) and digat_shortlist.inc (short_bitonic: the one sorting network of the library).
//
// pl_sample_kernel, one workgroup of 256 threads per (list g, sample s); a thread holds the positions tid, tid + 256, tid + 512,
// tid + 768.  Position p is LIVE when p < clamp(count[g], 0, M) and scores[g][p] is finite.
//   keys    a_p = fl((double)x_p * inv_t) goes to LDS (-inf: not live); the word of (stream, sample, position) is hashed,
//           u = (w + 0.5) 2^-32 (exact), key = fl(a_p + (-log(-log(u)))): two float64 logarithms per position.  The key's bits are
//           mapped to an unsigned word that orders as the doubles do (never 0 for a finite key) and stored beside the position.
//   order   short_bitonic over the next power of two >= M of (key word, position) records, 16 bytes each: key descending, equal
//           keys by ascending position (shortlist_segment_kernel's tie rule); records that are no live position carry key 0 and
//           sink to the end.  The slate is the first n_out = min(k, live) records.  Keys and order are pl_draw_slate, the ONE
//           __device__ function this kernel and digat_list_plrank.inc's forward kernels call: the same draw from the same scores.
//   pl_prob_stage, the probability of a slate in LDS — the ONE __device__ function pl_sample_kernel and pl_log_prob_kernel both
//           call, on the same LDS image, so digat_pl_log_prob on the sampler's picks returns the sampler's bits:
//           a_max by a max butterfly (exact in any order); w_p = exp(max(fl(a_p - a_max), -700)) for every position (0: not live);
//           the picked weights move to a side array and their slots become 0; R = the sum of what is left: a thread's four
//           positions in ascending order, wave_sum_f64's butterfly, the four waves ((0 + 1) + 2) + 3; thread 0 then adds the picked
//           weights back from the END of the slate, Z_t = fl(Z_{t+1} + w_pick(t)) with Z_{n_out} = R: a suffix sum with no
//           subtraction, so no cancellation; thread t: step[t] = fl(d_t - log(Z_t)) with d_t = max(fl(a_pick(t) - a_max), -700);
//           thread 0 adds the steps in slate order.  All of it under `#pragma clang fp contract(off)`: never an fma.
// pl_log_prob_kernel stages the same a_p, reads the slate from `picks` and cuts it at the first entry that is negative, out of
// range, not live or a repeat of an earlier one, then calls pl_prob_stage.
// Determinism: a draw depends on (seed, stream, sample, position) alone and every order of addition on (M, count, the slate) —
// not on G, the grid, first_sample or the other lists.  No atomics, no workspace.
//
// The bound evaluate.pl_bound states, derived.  With u = 2^-53: both sides form fl(x inv_t), fl(a - a_max) and the clamp with the
// same roundings, so the arguments of exp agree bit for bit.  exp is correct to 1 ulp on either side: the weights differ by at most
// 4u relatively.  The twin's Z_t is the correctly rounded sum (fsum: u); the device adds at most n positive terms, each addition
// at most u of a partial sum that never exceeds Z_t: (n - 1) u.  So the two Z_t differ by at most (n + 4) u Z_t and their exact
// logarithms by (n + 4) u (1 + O(nu)); log is correct to 1 ulp on either side: 4u |log Z_t|.  Before the last rounding the steps
// differ by at most (n + 4) u + 4u |log Z_t| <= (n + 16) u (1 + |log Z_t|) — the form the issue expects, with room to spare.  One
// term comes on top of it: each side ROUNDS d_t - log Z_t to float64, and two numbers that close may round to neighbours, 2u |v|
// apart (d_t reaches 700 where log Z_t is near 0, so (n + 16) u does not cover it).  step_logp is compared as float32: one rounding
// of 2^-24 |v| on either side, 2^-23 |v| together.  logp: the twin adds the float64 steps exactly, the device in slate order,
// k - 1 additions of at most u sum |v| each, plus the twin's own rounding: (k + 1) u sum |v| on top of the summed step bounds.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup, scratch 0:
//   pl_sample_kernel     VGPRs 32   SGPRs 64   LDS 37424 B   occupancy 4 waves / SIMD (by LDS: four 36.5 KB workgroups per CU)
//   pl_log_prob_kernel   VGPRs 30   SGPRs 53   LDS 21040 B   occupancy 7 waves / SIMD (by LDS)
// shortlist_segment_kernel, whose network became short_bitonic, keeps its line: 32 / 76 / 19560, occupancy 8.

#define PL_MAX_M DIGAT_PL_MAX_LIST
#define PL_MAX_K DIGAT_PL_MAX_K
#define PL_CLAMP DIGAT_PL_CLAMP

static_assert(PL_MAX_M == 1024 && PL_MAX_M == SHORT_MAX_K, "a thread holds four positions; short_bitonic orders at most SHORT_MAX_K records");
static_assert(PL_MAX_K == TOPK_MAX_K && PL_MAX_K <= 256, "thread t owns step t of a slate");
static_assert(DIGAT_PL_MAX_SAMPLE == (1 << 22), "a sample shares the low counter word with a 10-bit position");
constexpr long PL_GRID_X = 1L << 23;             // lists per launch (gridDim.x)
constexpr long PL_GRID_Y = 65535;                // samples per launch (gridDim.y)

struct PlRec {
    unsigned long long key;      // the float64 key as an ordered word; 0: no live position
    unsigned long long pos;
};

struct PlShared {
    double a[PL_MAX_M];          // fl(x inv_t); -inf: not live
    double w[PL_MAX_M];          // exp(max(a - a_max, -700)); 0: not live, or moved to wpick
    double wpick[PL_MAX_K], d[PL_MAX_K], z[PL_MAX_K], v[PL_MAX_K];
    double part[4];
    int pick[PL_MAX_K];
    int cut[4];
};

struct PlArgs {
    const float* scores;
    const int32_t* count;
    long g0;                     // first list of this launch
    int M, k;
    double inv_t;
    unsigned seed;
    long s0, first_sample;       // first sample of this launch; the caller's first_sample
    long S;                      // samples of the call: the row length of the outputs
    const int64_t* streams;
    const int32_t* picks_in;     // pl_log_prob_kernel
    int32_t* out_picks;
    int32_t* out_n;
    double* out_logp;
    float* out_step;
};

__device__ __forceinline__ double pl_mul(double x, double y) {
#pragma clang fp contract(off)
    return x * y;
}

__device__ __forceinline__ double pl_add(double x, double y) {
#pragma clang fp contract(off)
    return x + y;
}

// fl(a - a_max), held at -700 from below: the argument of a weight's exp and the first term of a step.
__device__ __forceinline__ double pl_rel(double a, double amax) {
#pragma clang fp contract(off)
    const double d = a - amax;
    return d > PL_CLAMP ? d : PL_CLAMP;
}

// A float64 as a word that orders as the doubles do; finite keys never map to 0.
__device__ __forceinline__ unsigned long long pl_ordered(double key) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(key);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// sh.a[0 .. 1024) of list g: the whole workgroup; a barrier follows in the caller.
__device__ __forceinline__ void pl_stage_list(const PlArgs& a, long g, PlShared& sh) {
    int cnt = a.count ? a.count[g] : a.M;
    cnt = cnt < 0 ? 0 : (cnt > a.M ? a.M : cnt);
    for (int p = threadIdx.x; p < PL_MAX_M; p += 256) {
        double ap = -INFINITY;
        if (p < cnt) {
            const float x = a.scores[(size_t)g * a.M + p];
            if (x - x == 0.f) ap = pl_mul((double)x, a.inv_t);       // finite: an infinity and a NaN fail the comparison
        }
        sh.a[p] = ap;
    }
}

// The weights and the suffix sums of the slate sh.pick[0 .. n_out) — live, distinct positions — under sh.a: behind it sh.w holds the
// weights with the picked slots at 0, sh.wpick / sh.d / sh.z [0 .. n_out) the picked weights, d_t and Z_t.  Called by the whole
// workgroup behind a barrier that made sh.a and sh.pick visible; ends behind a barrier.  pl_prob_stage's first half, and all that
// digat_list_pl.inc's lpl_coef_kernel needs of it.
__device__ __forceinline__ void pl_z_stage(PlShared& sh, int n_out) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m = -INFINITY;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const double ap = sh.a[tid + 256 * h];
        m = ap > m ? ap : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if (lane == 0) sh.part[wave] = m;
    __syncthreads();
    double amax = sh.part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) amax = sh.part[w] > amax ? sh.part[w] : amax;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const double ap = sh.a[tid + 256 * h];
        sh.w[tid + 256 * h] = ap > -INFINITY ? exp(pl_rel(ap, amax)) : 0.0;
    }
    __syncthreads();                                 // the weights stand; part[] has been read by every thread
    if (tid < n_out) {
        const int p = sh.pick[tid];
        sh.wpick[tid] = sh.w[p];
        sh.d[tid] = pl_rel(sh.a[p], amax);
    }
    __syncthreads();
    if (tid < n_out) sh.w[sh.pick[tid]] = 0.0;       // distinct positions: one writer per slot
    __syncthreads();
    double r = sh.w[tid];
#pragma unroll
    for (int h = 1; h < 4; ++h) r = r + sh.w[tid + 256 * h];
    r = wave_sum_f64(r);
    if (lane == 0) sh.part[wave] = r;
    __syncthreads();
    if (tid == 0) {
        double z = ((sh.part[0] + sh.part[1]) + sh.part[2]) + sh.part[3];
        for (int t = n_out - 1; t >= 0; --t) {
            z = z + sh.wpick[t];
            sh.z[t] = z;
        }
    }
    __syncthreads();
}

// The probability of the slate sh.pick[0 .. n_out) under sh.a: out_step[0 .. k) and *out_logp.  Called as pl_z_stage is.
__device__ __forceinline__ void pl_prob_stage(PlShared& sh, int k, int n_out, double* out_logp, float* out_step) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    pl_z_stage(sh, n_out);
    if (tid < k) {
        double v = 0.0;
        if (tid < n_out) v = sh.d[tid] - log(sh.z[tid]);
        sh.v[tid] = v;
        out_step[tid] = (float)v;
    }
    __syncthreads();
    if (tid == 0) {
        double lp = 0.0;
        for (int t = 0; t < n_out; ++t) lp = lp + sh.v[t];
        *out_logp = lp;
    }
}

// One Plackett-Luce draw under sh.a: the Gumbel keys of (seed, stream, sample, position) into rec, the live count, short_bitonic, and
// the slate — the first n_out = min(k, live) records — into sh.pick[0 .. k), -1 from n_out on.  Returns n_out.  The ONE __device__
// function pl_sample_kernel and digat_list_plrank.inc's forward kernels both call.  The whole workgroup; a thread reads the sh.a slots
// it stored itself (p = tid + 256 h); ends with sh.pick[tid] written by thread tid alone: a barrier follows in the caller.
__device__ __forceinline__ int pl_draw_slate(PlShared& sh, PlRec* rec, int M, int k, unsigned seed, unsigned stream, long sample) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n2 = 2;
    while (n2 < M) n2 <<= 1;
    const unsigned inner = hash32(seed + stream);
    const unsigned low0 = (unsigned)sample << 10;
    int live = 0;
    for (int p = tid; p < n2; p += 256) {
        const double ap = sh.a[p];                  // this thread's own store
        unsigned long long key = 0ull;
        if (ap > -INFINITY) {
            const unsigned w = hash32((low0 | (unsigned)p) * 0x9E3779B9U + inner);
            const double u = ((double)w + 0.5) * 0x1p-32;            // exact: 33 significant bits
            key = pl_ordered(pl_add(ap, -log(-log(u))));
            ++live;
        }
        rec[p] = PlRec{key, (unsigned long long)p};
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) live += __shfl_xor(live, o, 64);
    if (lane == 0) sh.cut[wave] = live;
    __syncthreads();
    live = sh.cut[0] + sh.cut[1] + sh.cut[2] + sh.cut[3];
    const int n_out = live < k ? live : k;
    short_bitonic(rec, n2, [](const PlRec& x, const PlRec& y) { return x.key > y.key || (x.key == y.key && x.pos < y.pos); });
    if (tid < k) sh.pick[tid] = tid < n_out ? (int)rec[tid].pos : -1;
    return n_out;
}

__global__ void __launch_bounds__(256) pl_sample_kernel(const PlArgs a) {
    __shared__ PlShared sh;
    __shared__ PlRec rec[PL_MAX_M];
    const int tid = threadIdx.x;
    const long g = a.g0 + blockIdx.x, s = a.s0 + blockIdx.y;
    pl_stage_list(a, g, sh);
    const unsigned stream = a.streams ? (unsigned)a.streams[g] : (unsigned)g;
    const int n_out = pl_draw_slate(sh, rec, a.M, a.k, a.seed, stream, a.first_sample + s);
    const size_t row = (size_t)g * (size_t)a.S + (size_t)s;
    if (tid < a.k) a.out_picks[row * a.k + tid] = sh.pick[tid];
    if (tid == 0 && s == 0) a.out_n[g] = n_out;
    __syncthreads();
    pl_prob_stage(sh, a.k, n_out, a.out_logp + row, a.out_step + row * a.k);
}

// Row `row` of a.picks_in into sh.pick, cut in front of its first entry that is negative, out of range, not live or a repeat of an
// earlier one: the slate's length.  The whole workgroup; its first barrier also makes sh.a visible.  pl_log_prob_kernel's rule, and
// through this function digat_list_pl.inc's.
__device__ __forceinline__ int pl_cut_slate(const PlArgs& a, size_t row, PlShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int p = -1;
    if (tid < a.k) {
        p = a.picks_in[row * a.k + tid];
        sh.pick[tid] = p;
    }
    __syncthreads();
    bool bad = tid < a.k && (p < 0 || p >= a.M || !(sh.a[p] > -INFINITY));
    if (tid < a.k && !bad)
        for (int j = 0; j < tid; ++j) bad = bad || sh.pick[j] == p;  // a repeat of an earlier entry
    const unsigned long long b = __ballot(bad);
    if (lane == 0) sh.cut[wave] = b ? 64 * wave + __ffsll((long long)b) - 1 : PL_MAX_M;
    __syncthreads();
    int n_out = a.k;                                 // the slate ends in front of the first bad entry
#pragma unroll
    for (int w = 0; w < 4; ++w) n_out = sh.cut[w] < n_out ? sh.cut[w] : n_out;
    return n_out;
}

__global__ void __launch_bounds__(256) pl_log_prob_kernel(const PlArgs a) {
    __shared__ PlShared sh;
    const long g = a.g0 + blockIdx.x, s = a.s0 + blockIdx.y;
    const size_t row = (size_t)g * (size_t)a.S + (size_t)s;
    pl_stage_list(a, g, sh);
    const int n_out = pl_cut_slate(a, row, sh);
    pl_prob_stage(sh, a.k, n_out, a.out_logp + row, a.out_step + row * a.k);
}

static int pl_check(const float* scores, int64_t G, int M, int k, double inv_t, int64_t samples, int64_t first_sample,
                    const void* o1, const void* o2) {
    if (!scores || !o1 || !o2 || G < 0) return DIGAT_ERR_ARG;
    if (!(inv_t > 0.0) || !(inv_t * 3.4028234663852886e38 < INFINITY)) return DIGAT_ERR_ARG;       // a NaN fails the first comparison
    if (((uintptr_t)scores & 3) || ((uintptr_t)o1 & 7) || ((uintptr_t)o2 & 3)) return DIGAT_ERR_ARG;
    if (k < 1 || k > PL_MAX_K || M < 1 || M > PL_MAX_M || G > 0x7fffffffL) return DIGAT_ERR_SHAPE;
    if (samples < 1 || first_sample < 0 || first_sample > DIGAT_PL_MAX_SAMPLE || samples > DIGAT_PL_MAX_SAMPLE - first_sample) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

// One launch per (at most PL_GRID_X lists, at most PL_GRID_Y samples); `more`: a kernel's arguments behind PlArgs (digat_pl_expect.inc).
template <class Kernel, class... More>
static int pl_launch(Kernel kernel, PlArgs a, int64_t G, int64_t S, hipStream_t st, More... more) {
    for (long g0 = 0; g0 < (long)G; g0 += PL_GRID_X)
        for (long s0 = 0; s0 < (long)S; s0 += PL_GRID_Y) {
            const long gs = (long)G - g0 < PL_GRID_X ? (long)G - g0 : PL_GRID_X, ss = (long)S - s0 < PL_GRID_Y ? (long)S - s0 : PL_GRID_Y;
            a.g0 = g0;
            a.s0 = s0;
            hipLaunchKernelGGL(kernel, dim3((unsigned)gs, (unsigned)ss), dim3(256), 0, st, a, more...);
            DIGAT_CHECK_LAUNCH();
        }
    return DIGAT_OK;
}

extern "C" {

size_t digat_pl_sample_workspace_bytes(int64_t lists, int m, int k, int64_t samples) {
    (void)lists; (void)m; (void)k; (void)samples;
    return 0;                                        // a slate's whole state lives in LDS
}

int digat_pl_sample(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, uint32_t seed, int64_t samples,
                    int64_t first_sample, const int64_t* streams, int32_t* out_picks, int32_t* out_n, double* out_logp, float* out_step,
                    void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!out_picks || !out_n || ((uintptr_t)out_picks & 3) || ((uintptr_t)out_n & 3) || ((uintptr_t)count & 3) || ((uintptr_t)streams & 7))
        return DIGAT_ERR_ARG;
    const int rc = pl_check(scores, G, M, k, inv_t, samples, first_sample, out_logp, out_step);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    const PlArgs a{scores, count, 0, M, k, inv_t, seed, 0, (long)first_sample, (long)samples, streams, nullptr, out_picks, out_n, out_logp, out_step};
    return pl_launch(pl_sample_kernel, a, G, samples, (hipStream_t)stream);
}

int digat_pl_log_prob(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples, const int32_t* picks,
                      double* out_logp, float* out_step, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!picks || ((uintptr_t)picks & 3) || ((uintptr_t)count & 3)) return DIGAT_ERR_ARG;
    const int rc = pl_check(scores, G, M, k, inv_t, samples, 0, out_logp, out_step);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    const PlArgs a{scores, count, 0, M, k, inv_t, 0u, 0, 0, (long)samples, nullptr, picks, nullptr, nullptr, out_logp, out_step};
    return pl_launch(pl_log_prob_kernel, a, G, samples, (hipStream_t)stream);
}

}  // extern "C"
