// digat_bootstrap.inc — bootstrap resampling of per-unit metric rows (the sums behind evaluate.metric_intervals / compare_metrics:
// percentile intervals and paired differences of every mean this library reports).  Included at the end of digat_kernels.hip, behind
// digat_eval.inc (wave_sum_f64) and the dropout hash (hash32: a draw's word is drop_keep's construction, the seed used as given).
//
// Replicate r = first_replicate + b makes n draws; draw j has the 64-bit counter e = r n + j, the word
//   w = hash32((uint32)e * 0x9E3779B9 + hash32(seed + (uint32)(e >> 32)))
// and the unit idx = (w n) >> 32 (a 64-bit product: idx < n for every w); sums[b, :] = sum over j of values[idx_j, :].  One index per
// draw serves every column — what makes a comparison of two models' columns a paired one.
//
// bootstrap_sums_kernel<C>, one workgroup (4 waves) per (slice of BOOT_SLICE draws, replicate): thread t takes the slice's draws
//   t, t + 256, t + 512, ... in this order, hashes each, loads the row (8 C contiguous bytes: 16-byte loads where C is even and the
//   table 16-byte aligned, else 8-byte ones — the loads change no bit) and adds it into C double accumulators in registers; a draw
//   beyond n adds nothing.  Then per column the butterfly of wave_sum_f64 (both partners add the same two numbers), the four waves'
//   sums through LDS, and thread c adds them ((0 + 1) + 2) + 3 and writes column c: to sums[b, c] when n has one slice, else to the
//   workspace's partial [b, slice, c].
// bootstrap_finish_kernel (more than one slice only), one thread per (replicate, column): the slices' partials added in ascending order.
//
// Determinism: which thread takes a draw, and every order of addition, are fixed by j and n alone — not by B, first_replicate, C, the
// grid or the other columns —; no float atomics.  So a column's sums depend on that column, n, seed and the replicate only: a call
// split by first_replicate, or its columns split over two calls, gives the same bits.
//
// segment_sums_f64_kernel, one thread per (unit, column): the unit's rows added left to right (start clamped to [0, rows]: no read
// leaves the table whatever the device array holds).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup, AGPRs 0, scratch 0,
// no dynamic LDS:
//   bootstrap_sums_kernel<C>   VGPRs 22 / 30 / 40 / 28 (C = 1 .. 4), 62 / 40 / 64 / 48 (5 .. 8), 72 / 62 / 68 / 70 / 68 / 70 / 72 / 71 (9 .. 16)
//                              SGPRs 28 - 33   LDS 512 B static   occupancy 8 waves / SIMD (7 at C = 9 and 11 .. 16)
//   bootstrap_finish_kernel, segment_sums_f64_kernel   VGPRs 13   SGPRs 27   LDS 0   occupancy 8

constexpr int BOOT_SLICE = DIGAT_BOOTSTRAP_SLICE;
constexpr int BOOT_MAX_C = DIGAT_BOOTSTRAP_MAX_COLUMNS;
constexpr long BOOT_GRID_Y = 65535;              // replicates per launch (gridDim.y)
constexpr long BOOT_LAUNCH_WG = 1L << 23;        // ... and workgroups per launch

template <int C>
__global__ void __launch_bounds__(256) bootstrap_sums_kernel(const double* __restrict__ values, unsigned n, long long first, unsigned seed,
                                                             int wide, double* __restrict__ out) {
    __shared__ double part[4][BOOT_MAX_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long e0 = (unsigned long long)(first + (long long)blockIdx.y) * n;
    const unsigned j0 = blockIdx.x * (unsigned)BOOT_SLICE;              // < n < 2^31
    const unsigned j1 = n - j0 > (unsigned)BOOT_SLICE ? j0 + (unsigned)BOOT_SLICE : n;
    double acc[C];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (unsigned j = j0 + tid; j < j1; j += 256) {
        const unsigned long long e = e0 + j;
        const unsigned w = hash32((unsigned)e * 0x9E3779B9U + hash32(seed + (unsigned)(e >> 32)));
        const size_t idx = (size_t)(((unsigned long long)w * n) >> 32);     // < n
        const double* const row = values + idx * C;
        if ((C & 1) == 0 && wide) {
            const double2* const row2 = (const double2*)row;
#pragma unroll
            for (int k = 0; k < C / 2; ++k) {
                const double2 v = row2[k];
                acc[2 * k] += v.x;
                acc[2 * k + 1] += v.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) acc[k] += row[k];
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < C)
        out[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// sums[b, c] = partial[b, 0, c] + partial[b, 1, c] + ... in this order; `total` = replicates of this launch x C
__global__ void __launch_bounds__(256) bootstrap_finish_kernel(const double* __restrict__ partial, int S, int C, long total,
                                                               double* __restrict__ sums) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long b = i / C;
    const int c = (int)(i - b * C);
    const double* p = partial + (size_t)b * S * C + c;
    double a = p[0];
    for (int s = 1; s < S; ++s) a += p[(size_t)s * C];
    sums[i] = a;
}

__global__ void __launch_bounds__(256) segment_sums_f64_kernel(const double* __restrict__ values, long rows, int C,
                                                               const int64_t* __restrict__ start, long total, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long u = i / C;
    const int c = (int)(i - u * C);
    long a = start[u], b = start[u + 1];
    a = a < 0 ? 0 : (a > rows ? rows : a);
    b = b < 0 ? 0 : (b > rows ? rows : b);
    double s = 0.0;
    for (long r = a; r < b; ++r) s += values[(size_t)r * C + c];
    out[i] = s;
}

static inline long boot_slices(int64_t n) { return (long)((n + BOOT_SLICE - 1) / BOOT_SLICE); }

static int boot_check(int64_t n, int c, int64_t B, int64_t r0) {
    if (n < 1 || c < 1 || B < 0 || r0 < 0) return DIGAT_ERR_ARG;
    if (n > 0x7fffffffLL || c > BOOT_MAX_C || r0 > (1LL << 31) || B > (1LL << 31) - r0) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

template <int C>
static void boot_launch(dim3 grid, hipStream_t st, const double* values, unsigned n, long long first, unsigned seed, int wide, double* out) {
    hipLaunchKernelGGL(bootstrap_sums_kernel<C>, grid, dim3(256), 0, st, values, n, first, seed, wide, out);
}

extern "C" {

size_t digat_bootstrap_workspace_bytes(int64_t n, int c, int64_t B) {
    if (boot_check(n, c, B, 0) != DIGAT_OK) return 0;
    const long S = boot_slices(n);
    return S == 1 ? 0 : (size_t)B * (size_t)S * (size_t)c * sizeof(double);
}

int digat_bootstrap_sums(const double* values, int64_t n, int c, int64_t B, int64_t first_replicate, uint32_t seed, double* sums,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!values || !sums || ((uintptr_t)values & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7)) return DIGAT_ERR_ARG;
    const int rc = boot_check(n, c, B, first_replicate);
    if (rc != DIGAT_OK) return rc;
    const size_t need = digat_bootstrap_workspace_bytes(n, c, B);
    if (need && (!workspace || workspace_bytes < need)) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const long S = boot_slices(n);                                   // <= 2^31 / BOOT_SLICE
    long per = BOOT_LAUNCH_WG / S;
    per = per < 1 ? 1 : (per > BOOT_GRID_Y ? BOOT_GRID_Y : per);
    const int wide = ((uintptr_t)values & 15) == 0;
    for (int64_t b0 = 0; b0 < B; b0 += per) {
        const long nb = (long)(B - b0 < per ? B - b0 : per);
        double* const out = S == 1 ? sums + (size_t)b0 * c : (double*)workspace + (size_t)b0 * S * c;
        const dim3 grid((unsigned)S, (unsigned)nb);
        const long long first = first_replicate + b0;
        switch (c) {
#define BOOT_CASE(C) case C: boot_launch<C>(grid, st, values, (unsigned)n, first, seed, wide, out); break;
            BOOT_CASE(1) BOOT_CASE(2) BOOT_CASE(3) BOOT_CASE(4) BOOT_CASE(5) BOOT_CASE(6) BOOT_CASE(7) BOOT_CASE(8)
            BOOT_CASE(9) BOOT_CASE(10) BOOT_CASE(11) BOOT_CASE(12) BOOT_CASE(13) BOOT_CASE(14) BOOT_CASE(15) BOOT_CASE(16)
#undef BOOT_CASE
        }
        DIGAT_CHECK_LAUNCH();
        if (S > 1) {
            const long total = nb * c;
            hipLaunchKernelGGL(bootstrap_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                               (const double*)out, (int)S, c, total, sums + (size_t)b0 * c);
            DIGAT_CHECK_LAUNCH();
        }
    }
    return DIGAT_OK;
}

int digat_segment_sums_f64(const double* values, int64_t rows, int columns, const int64_t* start, int64_t units, double* out,
                           void* stream) {
    if (!start || !out || rows < 0 || columns < 1 || units < 0 || (rows > 0 && !values)) return DIGAT_ERR_ARG;
    if (((uintptr_t)values & 7) || ((uintptr_t)out & 7) || ((uintptr_t)start & 7)) return DIGAT_ERR_ARG;
    if (columns > (1 << 20) || units > (1LL << 38) / columns) return DIGAT_ERR_SHAPE;          // units x columns / 256 workgroups < 2^31
    if (units == 0) return DIGAT_OK;
    const long total = (long)units * columns;
    hipLaunchKernelGGL(segment_sums_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values,
                       (long)rows, columns, start, total, out);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
