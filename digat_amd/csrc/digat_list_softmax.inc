// digat_list_softmax.inc — listwise distillation: the softmax of a user's OWN list of news held against a target distribution given
// as scores, and its gradients, without a [G, M, d] copy of the gathered rows ever reaching memory (evaluate.list_softmax,
// nrms.distil_step).  Included in digat_kernels.hip behind digat_pool_softmax.inc; dot_load4 is digat_dot_topk.inc's.
// users [G, d], rows [P, d], ids [G, M] int64, count [G] int32 (NULL: M), teacher [G, M], scale, temperature > 0.
//   Slot (g, j) is an ELEMENT when j < clamp(count[g], 0, M) and 0 <= ids[g, j] < P; a repeated id in one list is two elements.
//   score(g, j) = the fp32 fmaf chain over c = 0 .. d-1 from 0 — digat_dot_scores' bits (digat_dot_topk.inc) —, x = fl(scale * score).
//   tau = teacher / temperature where the slot is an element and teacher is finite; any other element (-inf, +inf, NaN) has target
//   mass 0.  q = softmax(tau) over the elements with mass, p = softmax(x) over all elements.
//   lse[g]  = log sum exp x                                       (-inf without elements)
//   loss[g] = KL(q || p) = lse_x - lse_tau + sum_j q_j (tau_j - x_j)    (0, with valid[g] = 0, without an element or without mass)
//   out_scores [G, M] = the score bits at elements, NaN elsewhere.  Every output byte is written whatever count holds.
// Backward, given grad_loss [G] and the forward's lse and out_scores (nothing is recomputed but the gathers):
//   coef(g, j) = grad_loss[g] scale (p_j - q_j) on elements of valid lists, exactly 0 elsewhere        -> workspace [G, M]
//   d_users[g, :] = sum_j coef(g, j) rows[id_j, :]          d_rows[p, :] = sum over the elements with ids[g, j] == p of coef(g, j) users[g, :]
//
// Forward, one launch:
//   lsm_fwd_kernel     one workgroup of 256 threads per list, lanes own slots tid, tid + 256, ..  The user row goes into LDS.  Per slab
//                      of 256 slots the rows are staged in blocks of LSM_KB = 32 channels — whole 128-byte lines per row, eight
//                      threads a line, the next block's loads in flight under the arithmetic — into an LDS tile of stride 36 floats
//                      (a lane reads its own row 16 bytes at a time: 9 l mod 16 is a different bank quad for each lane of a
//                      ds_read_b128 group of 16; a write pass is eight lanes, one row's 32 consecutive dwords), and every lane
//                      carries its slot's accumulator across the blocks: the chain above, on the vector unit.  Then, in fp64:
//                      the maxima of x and tau (always subtracted), sum exp(x - max), sum exp(tau - max) and
//                      sum exp(tau - max) (tau - x): a lane adds its slots in ascending order, the wave's butterfly (lane l +
//                      lane l ^ 32, ^ 16, .. ^ 1: psm_chunk_kernel's), then the waves 0 + 1 + 2 + 3; lse and loss rounded once.
// Backward, two launches (one when d_rows is NULL):
//   lsm_users_kernel   one workgroup per list: lse_tau again from teacher, coef -> workspace and LDS, then the gather: wave w takes the
//                      elements j = w, w + 4, .. in ascending order, lane l the channels l, l + 64, ..; the four waves' sums are added
//                      in wave order.
//   lsm_rows_kernel    one wave per row p of rows: entry_keys [E] int64 holds, sorted, id (G M) + (g M + j) of every element; the wave
//                      finds the lower bound of p (G M) by bisection and walks to the next row's, adding coef(g, j) users[g, :] in
//                      ascending (g, j).  Every row is written, zeros included.  The keys are distinct, so any correct sort gives the
//                      same array: the caller sorts (evaluate.list_softmax: torch.sort in the forward, the ids carry no gradient).  A
//                      key outside its row's range is never followed.
// No floating-point atomics: every sum's order is fixed by M, d, count and ids alone, so two calls give the same bits, and a list's
// outputs depend on that list alone.
//
// Error of lse and loss against an exact evaluation on the same fp32 scores, scale and temperature being the floats the entry
// receives (u = 2^-24, n <= M elements): tau, the exponentials, the sums, the logarithms and the quotient are fp64 — n + 8 operations
// deep at most, each below 2^-52 relative, on terms no larger than 1 + max|tau - x|: at M = 1 024 below
// 2^-40 (1 + max|x| + max|tau|) altogether.  What remains is fp32's: x = fl(scale * score) carries one rounding, u |x|.  It moves
// lse by at most sum_j p_j u |x_j| <= u max|x|, and loss, whose derivative in x_j is p_j - q_j, by at most
// u max|x| sum_j |p_j - q_j| <= u max|x| min(2, sqrt(2 loss)) (Pinsker).  Both are rounded once, u |lse| and u |loss|.  Altogether
//   |lse - exact|  <= u (max|x| + |lse|) + e64
//   |loss - exact| <= u (max|x| min(2, sqrt(2 loss)) + |loss|) + 2 e64           e64 = 2^-40 (1 + max|x| + max|tau|)
// At M = 1 024, |x|, |tau| <= 30: lse within 1.8e-6 + 6e-8 |lse|; loss within 6e-8 loss + 1.8e-6 min(2, sqrt(2 loss)), which is below
// 2e-6 up to loss = 0.6 and below 1e-5 loss from loss = 0.36 on — both inside the project's output tolerance (atol 2e-6, rtol 1e-5).
// evaluate.list_softmax_bound is this formula; tests/test_hip_list_softmax.py holds the kernels to it.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
//   lsm_fwd_kernel     VGPRs 86   SGPRs 71   LDS 41248 B   scratch 0   occupancy 3 waves / SIMD (by LDS: the staged tile)
//   lsm_users_kernel   VGPRs 52   SGPRs 58   LDS 20768 B   scratch 0   occupancy 7 waves / SIMD
//   lsm_rows_kernel    VGPRs 43   SGPRs 75   LDS 0 B   scratch 0   occupancy 8 waves / SIMD
//
// Measured on an MI355X at d = 400 against index_select + bmm + log_softmax + KL under autograd (tools/kbench.py list-softmax): 4 096
// lists of 1 024: forward 0.97 ms against 4.09, forward + backward 3.04 ms against 13.8 at a peak of 196 MiB of device memory beyond
// the inputs against 12.5 GiB; 4 096 x 128: 0.21 / 0.85 ms against 0.67 / 2.12.  64 lists — 64 workgroups on 256 CUs — lose: 64 x 1 024
// 0.19 / 0.71 ms against 0.14 / 0.47, 64 x 128 0.055 / 0.46 ms against 0.14 / 0.40 (DESIGN section 8).

#define LSM_MAX_D DIGAT_LIST_SOFTMAX_MAX_D       // the user row in LDS; eight channel registers per lane in the backward
#define LSM_MAX_M DIGAT_SHORTLIST_MAX_K
#define LSM_SLAB 256                     // slots scored at a time: one per thread
#define LSM_SLABS (LSM_MAX_M / LSM_SLAB)
#define LSM_KB 32                        // channels per staged block: one 128-byte line per row
#define LSM_LD (LSM_KB + 4)
#define LSM_DREGS (LSM_MAX_D / 64)

static_assert(LSM_MAX_M % LSM_SLAB == 0 && LSM_SLAB == 256, "a slab is one slot per thread of the workgroup");

struct LsmArgs {
    const float* users;
    const float* rows;
    const int64_t* ids;
    const int32_t* count;
    const float* teacher;
    long G, P;
    int M, d;
    float scale, temperature;
    float* loss;                         // [G]     forward out
    float* lse;                          // [G]     forward out, backward in
    int32_t* valid;                      // [G]     forward out
    float* scores;                       // [G, M]  forward out, backward in
    const float* grad_loss;              // [G]
    const int64_t* keys;                 // [E]
    long E;
    float* coef;                         // workspace [G, M]
    float* d_users;                      // [G, d]
    float* d_rows;                       // [P, d]
};

__device__ __forceinline__ int lsm_count(const LsmArgs& a, long g) {
    const int c = a.count ? a.count[g] : a.M;
    return c < 0 ? 0 : (c > a.M ? a.M : c);
}

// The news row of slot j of list g, -1 where the slot is no element.
__device__ __forceinline__ long long lsm_id(const LsmArgs& a, long g, int j, int cnt) {
    if (j >= cnt) return -1;
    const long long id = (long long)a.ids[g * a.M + j];
    return id < 0 || id >= a.P ? -1 : id;
}

// Whole workgroup, red = four doubles of LDS; every thread ends with the same bits, behind a barrier.
__device__ __forceinline__ double lsm_block_max(double v, double* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

__device__ __forceinline__ double lsm_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// What is subtracted before exp: the maximum, or 0 where that is not finite (no element; an infinite score shows in the result).
__device__ __forceinline__ double lsm_ref(double m) { return m - m == 0.0 ? m : 0.0; }

// The thread's slots of list g: x and tau in fp64 (-inf where the slot is no element / has no mass), from given score bits.
__device__ __forceinline__ void lsm_slots(const LsmArgs& a, long g, const float (&sc)[LSM_SLABS], const bool (&el)[LSM_SLABS],
                                          double (&x)[LSM_SLABS], double (&tau)[LSM_SLABS], bool (&ms)[LSM_SLABS]) {
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j = s * LSM_SLAB + (int)threadIdx.x;
        x[s] = -INFINITY;
        tau[s] = -INFINITY;
        ms[s] = false;
        if (el[s]) {
            x[s] = (double)(a.scale * sc[s]);
            const float t = a.teacher[g * a.M + j];
            ms[s] = t - t == 0.f;                                 // finite
            if (ms[s]) tau[s] = (double)t / (double)a.temperature;
        }
    }
}

// The scoring stage of a forward kernel (lsm_fwd_kernel; digat_list_pairwise.inc's lpw_fwd_kernel): the whole workgroup scores list g —
// sc[s] = the chain of slot s LSM_SLAB + tid, el[s] = whether that slot is an element — and writes a.scores.  su4, tile4 and sid are the
// caller's LDS: the user row, the staged tile and a slab's rows; the tile is free again behind the caller's next barrier.
__device__ __forceinline__ void lsm_score_stage(const LsmArgs& a, long g, int cnt, float4* su4, float4* tile4, long long* sid,
                                                float (&sc)[LSM_SLABS], bool (&el)[LSM_SLABS]) {
    float* const su = (float*)su4;
    float* const T = (float*)tile4;
    const int tid = threadIdx.x;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;                  // this thread stages rows r0 + 32 h, channels c4 .. c4 + 3
    const bool vec = (a.d & 3) == 0 && (((uintptr_t)a.rows) & 15) == 0;
    for (int c = tid; c < LSM_MAX_D; c += 256) su[c] = c < a.d ? a.users[g * a.d + c] : 0.f;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j0 = s * LSM_SLAB, j = j0 + tid;
        sc[s] = 0.f;
        el[s] = false;
        if (j0 >= a.M) continue;                                  // workgroup-uniform
        const long long id = lsm_id(a, g, j, cnt);
        el[s] = id >= 0;
        if (j0 < cnt) {                                           // workgroup-uniform: the slab holds slots in use
            __syncthreads();                                      // the slab before is done with sid; su is written
            sid[tid] = id;
            __syncthreads();
            const float* row[8];
            float4 rv[8];
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const long long rid = sid[r0 + 32 * h];
                row[h] = rid >= 0 ? a.rows + rid * a.d : nullptr;
                rv[h] = dot_load4(row[h], c4, a.d, vec);
            }
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
            sc[s] = acc;
        }
        if (j < a.M) a.scores[g * a.M + j] = el[s] ? sc[s] : __uint_as_float(0x7fc00000u);
    }
}

__global__ void __launch_bounds__(256) lsm_fwd_kernel(const LsmArgs a) {
    __shared__ float4 su4[LSM_MAX_D / 4];
    __shared__ float4 tile4[LSM_SLAB * LSM_LD / 4];
    __shared__ long long sid[LSM_SLAB];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = lsm_count(a, g);
    float sc[LSM_SLABS];
    bool el[LSM_SLABS];
    lsm_score_stage(a, g, cnt, su4, tile4, sid, sc, el);

    double x[LSM_SLABS], tau[LSM_SLABS];
    bool ms[LSM_SLABS];
    lsm_slots(a, g, sc, el, x, tau, ms);
    double mx = -INFINITY, mt = -INFINITY;
    bool anyel = false, anyms = false;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        mx = fmax(mx, x[s]);
        mt = fmax(mt, tau[s]);
        anyel = anyel || el[s];
        anyms = anyms || ms[s];
    }
    const int flags = (__syncthreads_or(anyel ? 1 : 0) ? 1 : 0) | (__syncthreads_or(anyms ? 1 : 0) ? 2 : 0);      // the barrier ORs truth values
    const double rx = lsm_ref(lsm_block_max(mx, red)), rt = lsm_ref(lsm_block_max(mt, red));
    double sx = 0.0, st = 0.0, cr = 0.0;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        if (el[s]) sx += exp(x[s] - rx);
        if (ms[s]) {
            const double w = exp(tau[s] - rt);
            st += w;
            cr += w * (tau[s] - x[s]);
        }
    }
    sx = lsm_block_sum(sx, red);
    st = lsm_block_sum(st, red);
    cr = lsm_block_sum(cr, red);
    if (tid == 0) {
        const double lse = (flags & 1) ? rx + log(sx) : (double)-INFINITY;
        a.lse[g] = (float)lse;
        a.valid[g] = flags == 3 ? 1 : 0;
        a.loss[g] = flags == 3 ? (float)((lse - (rt + log(st))) + cr / st) : 0.f;
    }
}

// The gather of a users kernel (lsm_users_kernel; digat_list_pairwise.inc's lpw_users_kernel): d_users[g, :] = sum_j scoef[j] rows[sid[j], :]
// over the slots below cnt whose sid is a row, wave w taking j = w, w + 4, .. in ascending order, lane l the channels l, l + 64, ..; the four
// waves' sums are added in wave order.  sid, scoef and part are the caller's LDS, written and behind a barrier; valid is workgroup-uniform.
__device__ __forceinline__ void lsm_gather_users(const LsmArgs& a, long g, int cnt, bool valid, const long long* sid, const float* scoef,
                                                 float (*part)[LSM_MAX_D]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float acc[LSM_DREGS];
#pragma unroll
    for (int i = 0; i < LSM_DREGS; ++i) acc[i] = 0.f;
    if (valid) {                                                  // workgroup-uniform
        for (int j0 = wave; j0 < cnt; j0 += 16) {
            const float* row[4];
            float cf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 4 * u;
                const long long id = j < cnt ? sid[j] : -1;
                row[u] = id >= 0 ? a.rows + id * a.d : nullptr;
                cf[u] = id >= 0 ? scoef[j] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < LSM_DREGS; ++i) {
                if (64 * i < a.d) {                               // workgroup-uniform
                    const int c = lane + 64 * i;
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = row[u] && c < a.d ? row[u][c] : 0.f;
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[i] = fmaf(cf[u], v[u], acc[i]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < LSM_DREGS; ++i) part[wave][lane + 64 * i] = acc[i];
    __syncthreads();
    for (int c = tid; c < a.d; c += 256) a.d_users[g * a.d + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

__global__ void __launch_bounds__(256) lsm_users_kernel(const LsmArgs a) {
    __shared__ long long sid[LSM_MAX_M];
    __shared__ float scoef[LSM_MAX_M];
    __shared__ float part[4][LSM_MAX_D];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int cnt = lsm_count(a, g);
    float sc[LSM_SLABS];
    bool el[LSM_SLABS];
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j = s * LSM_SLAB + tid;
        const long long id = j < a.M ? lsm_id(a, g, j, cnt) : -1;
        sid[j] = id;
        el[s] = id >= 0;
        sc[s] = el[s] ? a.scores[g * a.M + j] : 0.f;
    }
    double x[LSM_SLABS], tau[LSM_SLABS];
    bool ms[LSM_SLABS];
    lsm_slots(a, g, sc, el, x, tau, ms);
    double mt = -INFINITY;
    bool anyel = false, anyms = false;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        mt = fmax(mt, tau[s]);
        anyel = anyel || el[s];
        anyms = anyms || ms[s];
    }
    const bool some = __syncthreads_or(anyel ? 1 : 0) != 0, mass = __syncthreads_or(anyms ? 1 : 0) != 0;
    const bool valid = some && mass;
    const double rt = lsm_ref(lsm_block_max(mt, red));
    double st = 0.0;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s)
        if (ms[s]) st += exp(tau[s] - rt);
    st = lsm_block_sum(st, red);
    const double lse = (double)a.lse[g], gs = (double)a.grad_loss[g] * (double)a.scale;
#pragma unroll
    for (int s = 0; s < LSM_SLABS; ++s) {
        const int j = s * LSM_SLAB + tid;
        float cf = 0.f;
        if (valid && el[s]) cf = (float)(gs * (exp(x[s] - lse) - (ms[s] ? exp(tau[s] - rt) / st : 0.0)));
        scoef[j] = cf;
        if (j < a.M) a.coef[g * a.M + j] = cf;
    }
    __syncthreads();

    lsm_gather_users(a, g, cnt, valid, sid, scoef, part);
}

__global__ void __launch_bounds__(256) lsm_rows_kernel(const LsmArgs a) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P) return;                                         // wave-uniform; no barrier below
    const long long GM = (long long)a.G * a.M, k0 = (long long)p * GM, k1 = k0 + GM;
    long lo = 0, hi = a.E;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((long long)a.keys[mid] < k0) lo = mid + 1;
        else hi = mid;
    }
    float acc[LSM_DREGS];
#pragma unroll
    for (int i = 0; i < LSM_DREGS; ++i) acc[i] = 0.f;
    for (long e = lo; e < a.E; e += 4) {
        const float* row[4];
        float cf[4];
        bool more = true;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long key = e + u < a.E ? (long long)a.keys[e + u] : k1;
            more = more && key < k1;                              // the walk ends at the first key of a later row
            const bool ok = more && key >= k0;                    // a key below the row's range is no entry of a sorted array: never followed
            const long long flat = ok ? key - k0 : 0;
            row[u] = ok ? a.users + (flat / a.M) * a.d : nullptr;
            cf[u] = ok ? a.coef[flat] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < LSM_DREGS; ++i) {
            if (64 * i < a.d) {
                const int c = lane + 64 * i;
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = row[u] && c < a.d ? row[u][c] : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[i] = fmaf(cf[u], v[u], acc[i]);
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (int i = 0; i < LSM_DREGS; ++i) {
        const int c = lane + 64 * i;
        if (c < a.d) a.d_rows[p * a.d + c] = acc[i];
    }
}

static int lsm_check(const float* users, const float* rows, const int64_t* ids, const float* teacher, int64_t G, int64_t P, int M, int d,
                     float temperature) {
    if (!users || !rows || !ids || !teacher || G < 0 || P < 0 || !(temperature > 0.f) || temperature - temperature != 0.f)
        return DIGAT_ERR_ARG;
    if (M < 1 || M > LSM_MAX_M || d < 1 || d > LSM_MAX_D || G * (int64_t)M > 0x7fffffffL || P > 0x80000000L) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

extern "C" {

size_t digat_list_softmax_workspace_bytes(int64_t lists, int m) {
    if (lists < 0 || m < 1) return 0;
    return align_up((size_t)lists * (size_t)m * 4, 256);
}

int digat_list_softmax_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* teacher, int64_t G,
                           int64_t P, int M, int d, float scale, float temperature, float* out_loss, float* out_lse, int32_t* out_valid,
                           float* out_scores, void* stream) {
    if (!out_loss || !out_lse || !out_valid || !out_scores) return DIGAT_ERR_ARG;
    const int rc = lsm_check(users, rows, ids, teacher, G, P, M, d, temperature);
    if (rc != DIGAT_OK) return rc;
    if (G == 0) return DIGAT_OK;
    LsmArgs a{};
    a.users = users; a.rows = rows; a.ids = ids; a.count = count; a.teacher = teacher;
    a.G = (long)G; a.P = (long)P; a.M = M; a.d = d; a.scale = scale; a.temperature = temperature;
    a.loss = out_loss; a.lse = out_lse; a.valid = out_valid; a.scores = out_scores;
    hipLaunchKernelGGL(lsm_fwd_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_list_softmax_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* teacher, int64_t G,
                           int64_t P, int M, int d, float scale, float temperature, const float* lse, const float* scores,
                           const float* grad_loss, const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!lse || !scores || !grad_loss || !d_users) return DIGAT_ERR_ARG;
    const int rc = lsm_check(users, rows, ids, teacher, G, P, M, d, temperature);
    if (rc != DIGAT_OK) return rc;
    if (d_rows && (E < 0 || E > G * (int64_t)M || (E > 0 && !entry_keys))) return DIGAT_ERR_ARG;
    if (G > 0 && (!workspace || (((uintptr_t)workspace) & 3))) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_list_softmax_workspace_bytes(G, M)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LsmArgs a{};
    a.users = users; a.rows = rows; a.ids = ids; a.count = count; a.teacher = teacher;
    a.G = (long)G; a.P = (long)P; a.M = M; a.d = d; a.scale = scale; a.temperature = temperature;
    a.lse = const_cast<float*>(lse); a.scores = const_cast<float*>(scores); a.grad_loss = grad_loss;
    a.keys = entry_keys; a.E = G > 0 ? (long)E : 0;
    a.coef = (float*)workspace; a.d_users = d_users; a.d_rows = d_rows;
    if (G > 0) {
        hipLaunchKernelGGL(lsm_users_kernel, dim3((unsigned)G), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    if (d_rows && P > 0) {                                        // G == 0: no entry, every row zero
        hipLaunchKernelGGL(lsm_rows_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

}  // extern "C"
