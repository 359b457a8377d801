// digat_train.inc — backward / training kernels of the DIGAT hot path (included by digat_kernels.hip).
//
// The training step of the reference is plain autograd through graphEncoders.DIGAT.forward
// (trainer.py:98-102), which SAVES the [B,n,n,d] tensor of Eq. 8 (2.3 GB per layer at B=320).  Here
// every op on the path is a native forward/backward pair and Eq. 8's backward RECOMPUTES
// relu'(K3+K1+K2) from the saved projections, so nothing of size n*n*d is ever stored.
// Kernels are correctness-first (VALU, LDS-staged); the reductions are deterministic (no atomics).

// =================================================================================================
// T1. weight gradient: dW[o][i] = sum_m dY[m][o] X[m][i]   (a TN product with a very long K = M)
// =================================================================================================
// Output tile 80x80, M split over gridDim.y slices; each workgroup writes its partial tile to
// part[slice][o][i]; slice_reduce_kernel sums the slices in order.  MFMA 16x16x4 f32: both operands are
// read from the natural [m][.] LDS image (A[o][k=m] = dY[m][o], B[k=m][i] = X[m][i]), staged with float4
// loads.  The bias gradient db[o] = sum_m dY[m][o] rides along: the workgroups of input-column block 0 also sum
// their dY tile's columns (rows in ascending order) into part_db[slice][o].
struct TnArgs { const float* dY; long ldy; const float* X; long ldx; float* part; float* part_db; int M, No, Ni, slices, mper, vec; };

__device__ __forceinline__ void gemm_tn_tile(const TnArgs& g, const int tile, const int slice) {
    __shared__ float Ys[32][84];             // row stride 84 floats: 16-byte aligned rows, conflict-light column reads
    __shared__ float Xs[32][84];
    const int nti = (g.Ni + 79) / 80;
    const int to = tile / nti, ti = tile % nti;
    const int o0 = to * 80, i0 = ti * 80;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    v4f acc[7];                     // 5x5 tiles of 16x16 over 4 waves: tiles t = wave, wave+4, ... < 25
#pragma unroll
    for (int t = 0; t < 7; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    float dbsum = 0.f;              // thread c < 80 of a ti == 0 workgroup: column o0 + c of dY
    const int mbeg = slice * g.mper, mend = min(g.M, mbeg + g.mper);
    for (int m0 = mbeg; m0 < mend; m0 += 32) {
        if (g.vec) {                // 16-byte aligned rows, No / Ni multiples of 4: 32 rows x 20 float4 per operand
            for (int e = tid; e < 32 * 20; e += 256) {
                const int r = e / 20, c = (e - r * 20) * 4;
                const int m = m0 + r;
                float4 y = f4_zero(), x = f4_zero();
                if (m < mend) {
                    if (o0 + c < g.No) y = *reinterpret_cast<const float4*>(g.dY + (long)m * g.ldy + o0 + c);
                    if (i0 + c < g.Ni) x = *reinterpret_cast<const float4*>(g.X + (long)m * g.ldx + i0 + c);
                }
                *reinterpret_cast<float4*>(&Ys[r][c]) = y;
                *reinterpret_cast<float4*>(&Xs[r][c]) = x;
            }
        } else {
            for (int e = tid; e < 32 * 80; e += 256) {
                const int r = e / 80, c = e - r * 80;
                const int m = m0 + r;
                Ys[r][c] = (m < mend && o0 + c < g.No) ? g.dY[(long)m * g.ldy + o0 + c] : 0.f;
                Xs[r][c] = (m < mend && i0 + c < g.Ni) ? g.X[(long)m * g.ldx + i0 + c] : 0.f;
            }
        }
        __syncthreads();
        if (g.part_db && ti == 0 && tid < 80) {
#pragma unroll 8
            for (int r = 0; r < 32; ++r) dbsum += Ys[r][tid];
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int k = ks * 4 + lq;
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const int tile = wave + 4 * t;
                if (tile < 25) {
                    const int tr = tile / 5, tc = tile - tr * 5;
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ys[k][tr * 16 + lr], Xs[k][tc * 16 + lr], acc[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int tile = wave + 4 * t;
        if (tile >= 25) continue;
        const int tr = tile / 5, tc = tile - tr * 5;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + tr * 16 + lq * 4 + r, i = i0 + tc * 16 + lr;
            if (o < g.No && i < g.Ni) g.part[((long)slice * g.No + o) * g.Ni + i] = acc[t][r];
        }
    }
    if (g.part_db && ti == 0 && tid < 80 && o0 + tid < g.No) g.part_db[(long)slice * g.No + o0 + tid] = dbsum;
}
__global__ void __launch_bounds__(256) gemm_tn_kernel(const TnArgs g) { gemm_tn_tile(g, blockIdx.x, blockIdx.y); }

// Up to four SHORT products (M < 2048) in one launch and their slice sums in another (round 5): a context entry's backward has three
// or four weight gradients on 320 rows, each a 250-workgroup launch that leaves the chip a quarter full, plus its reduction — eight
// launches of 6-9 us become two.  blockIdx.z = product; the grid spans the largest tile / slice counts, the others' surplus
// workgroups leave at once.  Per product the tiles, slices and the order of every sum are those of the single launches: same bits.
constexpr int TN_GROUP_MAX = 4;
struct TnGroupArgs { TnArgs p[TN_GROUP_MAX]; int tiles[TN_GROUP_MAX]; };
__global__ void __launch_bounds__(256) gemm_tn_group_kernel(const TnGroupArgs a) {
    const int q = blockIdx.z;
    if ((int)blockIdx.x >= a.tiles[q] || (int)blockIdx.y >= a.p[q].slices) return;
    gemm_tn_tile(a.p[q], blockIdx.x, blockIdx.y);
}
struct ReduceGroupArgs { const float* part[TN_GROUP_MAX]; float* out[TN_GROUP_MAX]; long n[TN_GROUP_MAX]; const float* part_b[TN_GROUP_MAX];
                         float* out_b[TN_GROUP_MAX]; long nb[TN_GROUP_MAX]; int slices[TN_GROUP_MAX]; int accumulate[TN_GROUP_MAX]; };
__global__ void __launch_bounds__(256) slice_reduce_group_kernel(const ReduceGroupArgs a) {
    const int q = blockIdx.y;
    const long n = a.n[q], nb = a.nb[q];
    const int slices = a.slices[q], accumulate = a.accumulate[q];
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n + nb; e += (long)gridDim.x * 256) {       // slice_reduce2_kernel's loop
        const bool w = e < n;
        const float* src = w ? a.part[q] + e : a.part_b[q] + (e - n);
        float* dst = w ? a.out[q] + e : a.out_b[q] + (e - n);
        const long stride = w ? n : nb;
        float s = accumulate ? *dst : 0.f;
        for (int k = 0; k < slices; ++k) s += src[(long)k * stride];
        *dst = s;
    }
}

// The same product on the bf16 matrix cores (bf16x6: the exact 3-way operand split of digat_gemm.inc, six products, fp32
// accumulation — fp32-grade) for the long products (M >= 2048).  Output tile 160 x 160 per workgroup, four waves as 2 x 2 with
// 80 x 80 each (25 accumulator tiles); M split over gridDim.y slices as above.  Both operands are K-major in memory
// (dY[m][o], X[m][i]) while a lane's MFMA fragment is 8 consecutive k of ONE row, so the tile is transposed on its way into LDS:
// a thread loads 8 rows (k) x 5 columns, 32 apart (256 threads = 2 operands x 32 lanes x 4 k groups: one task each), splits every
// value into its three bf16 pieces and writes, per column and piece, the 8 k as one 16-byte fragment: LDS image
// [piece][k group][column].  Every value is split once per workgroup (two waves
// use it), ~0.4 vector cycles per MFMA cycle.  The next K tile's float4s are in flight in registers during the 150 MFMAs of a
// step (40 registers; 4-column float4 tasks would be 320: two per thread for a quarter of them, 64 registers and spills);
// two workgroups per CU (61 KB each) cover each other's split phase.  X is the MFMA's row operand, dY its column operand:
// a lane ends with four consecutive input columns of one output row (float4 stores).  db as in gemm_tn_kernel.
constexpr int TNB = 160;                  // tile edge
constexpr int TNB_PLANE = 4 * TNB;        // 16-byte slots of one piece image: 4 k groups x 160 columns
template <bool LITE>                      // LITE: one bf16 product (digat_set_train_precision(1))
__global__ void __launch_bounds__(256, 2) gemm_tn_bf16x6_kernel(const TnArgs g) {
    __shared__ uint4 Ys[3 * TNB_PLANE];
    __shared__ uint4 Xs[3 * TNB_PLANE];
    const int nti = (g.Ni + TNB - 1) / TNB;
    const int to = blockIdx.x / nti, ti = blockIdx.x % nti;
    const int slice = blockIdx.y;
    const int o0 = to * TNB, i0 = ti * TNB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kg = lane >> 4;
    const int wo = (wave >> 1) * 80, wi = (wave & 1) * 80;
    const int mbeg = slice * g.mper, mend = min(g.M, mbeg + g.mper);
    const bool want_db = g.part_db && ti == 0;
    // plain locals for the lambdas below (capturing the by-value argument struct sends it to scratch)
    const float* const pY = g.dY; const float* const pX = g.X;
    const long ldy = g.ldy, ldx = g.ldx;
    const int No = g.No, Ni = g.Ni;

    // staging tasks, one per thread: t < 128: dY, columns 5 (t % 32) .. + 4, k group t / 32; t >= 128: X likewise
    const bool isx = tid >= 128;
    const int tu = isx ? tid - 128 : tid;
    // the task's five columns are 32 apart (col + 32 e): the 32 lanes of a k group then read 128 contiguous bytes per load and
    // write 32 consecutive 16-byte LDS slots per store (five adjacent columns per lane made every load touch 10 cache lines)
    const int tk = tu >> 5, col = tu & 31;
    const int cbase = (isx ? i0 : o0) + col, climit = isx ? Ni : No;
    const float* const src = isx ? pX : pY;
    const long ld = isx ? ldx : ldy;
    int coff[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) coff[e] = min(cbase + 32 * e, climit - 1);     // clamped, straight-line loads; zeroed at the split
    float pre[8][5];
    auto request = [&](int m0) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = m0 + 8 * tk + r;
            const float* row = src + (long)(m < mend ? m : mend - 1) * ld;
#pragma unroll
            for (int e = 0; e < 5; ++e) pre[r][e] = row[coff[e]];
        }
    };
    float dbs[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // dY tasks of a ti == 0 workgroup: column sums of their 5 columns over their k
    auto split_store = [&](int m0) {
        uint4* img = (isx ? Xs : Ys) + tk * TNB + col;
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const bool cok = cbase + 32 * e < climit;
            Split3f sp[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float v = (cok && m0 + 8 * tk + r < mend) ? pre[r][e] : 0.f;
                if (want_db && !isx) dbs[e] += v;
                sp[r] = split3f(v);
            }
            img[32 * e] = make_uint4(pack_hi16(sp[0].a, sp[1].a), pack_hi16(sp[2].a, sp[3].a), pack_hi16(sp[4].a, sp[5].a), pack_hi16(sp[6].a, sp[7].a));
            if (!LITE) {
                img[TNB_PLANE + 32 * e] = make_uint4(pack_hi16(sp[0].b, sp[1].b), pack_hi16(sp[2].b, sp[3].b), pack_hi16(sp[4].b, sp[5].b), pack_hi16(sp[6].b, sp[7].b));
                img[2 * TNB_PLANE + 32 * e] = make_uint4(pack_hi16(sp[0].c, sp[1].c), pack_hi16(sp[2].c, sp[3].c), pack_hi16(sp[4].c, sp[5].c), pack_hi16(sp[6].c, sp[7].c));
            }
        }
    };

    v4f acc[5][5];                             // [o tile][i tile]
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = 0; b < 5; ++b) acc[a][b] = (v4f){0.f, 0.f, 0.f, 0.f};
    if (mbeg < mend) request(mbeg);
    for (int m0 = mbeg; m0 < mend; m0 += 32) {
        split_store(m0);
        __syncthreads();
        if (m0 + 32 < mend) request(m0 + 32);
        const int slot_o = kg * TNB + wo + lr, slot_i = kg * TNB + wi + lr;
#pragma unroll
        for (int grp = 0; grp < 3; ++grp) {                        // o tiles 0-1, 2-3, 4: 24 fragment registers instead of 60
            const int a0 = 2 * grp, an = grp == 2 ? 1 : 2;
            bf16x8 yf[2][3];
#pragma unroll
            for (int a = 0; a < 2; ++a)
                if (a < an)
#pragma unroll
                    for (int p = 0; p < (LITE ? 1 : 3); ++p) yf[a][p] = __builtin_bit_cast(bf16x8, Ys[p * TNB_PLANE + slot_o + 16 * (a0 + a)]);
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                bf16x8 xf[3];
#pragma unroll
                for (int p = 0; p < (LITE ? 1 : 3); ++p) xf[p] = __builtin_bit_cast(bf16x8, Xs[p * TNB_PLANE + slot_i + 16 * b]);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (a >= an) continue;
                    v4f c = acc[a0 + a][b];
                    if (!LITE) {
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[2], yf[a][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[1], yf[a][1], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[0], yf[a][2], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[1], yf[a][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[0], yf[a][1], c, 0, 0, 0);
                    }
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[0], yf[a][0], c, 0, 0, 0);
                    acc[a0 + a][b] = c;
                }
            }
        }
        __syncthreads();
    }
    // lane (lr, kg) of tile (a, b): output row o = .. + 16 a + lr, input columns i = .. + 16 b + 4 kg .. + 3
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const int o = o0 + wo + 16 * a + lr;
        if (o >= g.No) continue;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const int i = i0 + wi + 16 * b + 4 * kg;
            if (i < g.Ni) *reinterpret_cast<float4*>(g.part + ((long)slice * g.No + o) * g.Ni + i) =
                make_float4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
        }
    }
    if (want_db) {                             // the four k groups of a column block, in order
        float* red = reinterpret_cast<float*>(Ys);         // [4][160]
        if (!isx) {
#pragma unroll
            for (int e = 0; e < 5; ++e) red[tk * TNB + col + 32 * e] = dbs[e];
        }
        __syncthreads();
        if (tid < TNB && o0 + tid < g.No)
            g.part_db[(long)slice * g.No + o0 + tid] = ((red[tid] + red[TNB + tid]) + red[2 * TNB + tid]) + red[3 * TNB + tid];
    }
}

// out[e] (+)= sum_s part[s][e]   (slices in ascending order)
__global__ void __launch_bounds__(256) slice_reduce_kernel(const float* part, float* out, long n, int slices, int accumulate) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        float s = accumulate ? out[e] : 0.f;
        for (int k = 0; k < slices; ++k) s += part[(long)k * n + e];
        out[e] = s;
    }
}

// the weight and the bias gradient of one TN product in one launch: elements e < n of part -> out, the nb that follow of part_b -> out_b
// (stride_b >= nb: the partial bias rows may be wider than the nb leading columns wanted — dbW is the first d of [dh | dP' | dQ]'s 3 d sums)
__global__ void __launch_bounds__(256) slice_reduce2_kernel(const float* part, float* out, long n, const float* part_b, float* out_b, long nb,
                                                            long stride_b, int slices, int accumulate) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n + nb; e += (long)gridDim.x * 256) {
        const bool w = e < n;
        const float* src = w ? part + e : part_b + (e - n);
        float* dst = w ? out + e : out_b + (e - n);
        const long stride = w ? n : stride_b;
        float s = accumulate ? *dst : 0.f;
        for (int k = 0; k < slices; ++k) s += src[(long)k * stride];
        *dst = s;
    }
}

// column sums: out[c] (+)= sum_m x[m][c]; one workgroup per 64 columns, rows strided over 4 waves
// (flag != NULL: the launch runs only when (*flag != 0) == (want != 0) — the device chose between two producers of x)
__global__ void __launch_bounds__(256) colsum_kernel(const float* x, long ldx, float* out, int M, int N, int accumulate, const int* flag, int want) {
    __shared__ float red[4][64];
    if (flag && ((*flag != 0) != (want != 0))) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
    float s = 0.f;
    if (c < N) for (int m = w; m < M; m += 4) s += x[(long)m * ldx + c];
    red[w][threadIdx.x & 63] = s;
    __syncthreads();
    if (w == 0 && c < N) {
        const float t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        out[c] = accumulate ? out[c] + t : t;
    }
}

// the same for a few hundred rows in ONE launch: a workgroup per 16 columns, 16 row lanes of M / 16 consecutive rows each, the 16
// partial sums added in order (the two-stage form below costs two launches of ~5 us for the 320 x 400 partials of a training step)
__global__ void __launch_bounds__(256) colsum_small_kernel(const float* x, long ldx, float* out, int M, int N, int accumulate, const int* flag,
                                                           int want) {
    __shared__ float red[16][17];
    if (flag && ((*flag != 0) != (want != 0))) return;
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const int per = (M + 15) / 16, m0 = rl * per, m1 = min(M, m0 + per);
    float s = 0.f;
    if (c < N) for (int m = m0; m < m1; ++m) s += x[(long)m * ldx + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < N) {
        float t = red[0][cl];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += red[k][cl];
        out[c] = accumulate ? out[c] + t : t;
    }
}

// column sums of x [M, N] in two ordered stages: groups of `per` rows -> part [G, N]; colsum_kernel over the G partial rows
__global__ void __launch_bounds__(256) colsum_groups_kernel(const float* x, long ldx, float* part, int M, int N, int per, const int* flag, int want) {
    __shared__ float red[4][64];
    if (flag && ((*flag != 0) != (want != 0))) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
    const int m0 = blockIdx.y * per, m1 = min(M, m0 + per);
    float s = 0.f;
    if (c < N) for (int m = m0 + w; m < m1; m += 4) s += x[(long)m * ldx + c];
    red[w][threadIdx.x & 63] = s;
    __syncthreads();
    if (w == 0 && c < N) part[(long)blockIdx.y * N + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// out[c] = sum_m x[m][c] in two ordered stages (groups of 32 rows, then the groups): ~8x the workgroups of colsum_kernel alone,
// whose four waves per 64 columns walk all M rows (21 us at M = 320)
static size_t colsum2_scratch(int M, int N) { return (size_t)((M + 31) / 32) * N; }      // floats
// flag != NULL: run only when (*flag != 0) == (want != 0) (the device chose between two producers of the partial rows)
static int launch_colsum2_if(const float* x, long ldx, float* out, int M, int N, int accumulate, float* scratch, hipStream_t st,
                             const int* flag, int want) {
    const int per = 32, G = (M + per - 1) / per;
    if (G <= 1) {
        hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, st, x, ldx, out, M, N, accumulate, flag, want);
    } else if (M <= 512) {
        hipLaunchKernelGGL(colsum_small_kernel, dim3((N + 15) / 16), dim3(256), 0, st, x, ldx, out, M, N, accumulate, flag, want);
    } else {
        hipLaunchKernelGGL(colsum_groups_kernel, dim3((N + 63) / 64, G), dim3(256), 0, st, x, ldx, scratch, M, N, per, flag, want);
        hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, st, (const float*)scratch, (long)N, out, G, N, accumulate, flag, want);
    }
    return hipGetLastError() == hipSuccess ? DIGAT_OK : DIGAT_ERR_LAUNCH;
}
static int launch_colsum2(const float* x, long ldx, float* out, int M, int N, int accumulate, float* scratch, hipStream_t st) {
    return launch_colsum2_if(x, ldx, out, M, N, accumulate, scratch, st, nullptr, 0);
}

// =================================================================================================
// T2. elementwise pieces
// =================================================================================================
// y = x * keep / (1-p), keep from a counter-based hash of (seed, element index); mask byte saved
__global__ void __launch_bounds__(256) dropout_fwd_kernel(const float* x, float* y, uint8_t* mask, long n, float p,
                                                          unsigned seed) {
    const float scale = 1.f / (1.f - p);
    const unsigned thr = drop_threshold(p);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const uint8_t keep = drop_keep(seed, e, thr);
        mask[e] = keep;
        y[e] = keep ? x[e] * scale : 0.f;
    }
}
__global__ void __launch_bounds__(256) dropout_bwd_kernel(const float* dy, const uint8_t* mask, float* dx, long n, float p) {
    const float scale = 1.f / (1.f - p);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256)
        dx[e] = mask[e] ? dy[e] * scale : 0.f;
}
// gate mix (graphEncoders.py:112-113): out = s*l + (1-s)*g, s = sigmoid(zd), zd = dropout_p(z) applied HERE (round 6: the dropout
// launch before it and, in the backward, the one after it are gone).  zd (and the keep bytes, p > 0) are saved for the backward;
// l and g are rows of strides ldl / ldg (node 0 of X; the pooled half of the saved [l ; g] rows)
__global__ void __launch_bounds__(256) gate_fwd_kernel(const float* z, const float* l, long ldl, const float* gl, long ldg, float* out,
                                                       float* zd, uint8_t* zmask, float p, unsigned seed, int B, int d, const float* prev) {
    const long n = (long)B * d;
    const float scale = 1.f / (1.f - p);
    const unsigned thr = drop_threshold(p);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long b = e / d; const int c = (int)(e - b * d);
        float zv = z[e];
        if (zmask) {
            const uint8_t keep = drop_keep(seed, e, thr);
            zmask[e] = keep;
            zv = keep ? zv * scale : 0.f;
        }
        if (zd) zd[e] = zv;
        const float s = 1.f / (1.f + expf(-zv));
        const float v = s * l[b * ldl + c] + (1.f - s) * gl[b * ldg + c];
        out[e] = prev ? prev[e] + v : v;            // prev: the context accumulated so far (graphEncoders.py:185: c_n = c_n + ...)
    }
}
// dl, dg: rows of stride ldo (the two halves of one [B, 2 d] matrix in digat_news_ctx_bwd); dz through the dropout's keep bytes
__global__ void __launch_bounds__(256) gate_bwd_kernel(const float* dout, const float* z, const float* l, long ldl,
                                                       const float* gl, long ldg, const uint8_t* zmask, float scale, float* dz, float* dl,
                                                       float* dg, long ldo, int B, int d) {
    const long n = (long)B * d;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long b = e / d; const int c = (int)(e - b * d);
        const float s = 1.f / (1.f + expf(-z[e]));
        const float go = dout[e], lv = l[b * ldl + c], gv = gl[b * ldg + c];
        const float dzd = go * (lv - gv) * s * (1.f - s);
        dz[e] = zmask ? (zmask[e] ? dzd * scale : 0.f) : dzd;
        dl[b * ldo + c] = go * s;
        dg[b * ldo + c] = go * (1.f - s);
    }
}
// relu(y) + t  (graphEncoders.py:131) and its backward: dy = dout*[y>0], dt = dout
__global__ void __launch_bounds__(256) relu_res_fwd_kernel(const float* y, const float* t, float* out, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) out[e] = fmaxf(y[e], 0.f) + t[e];
}
__global__ void __launch_bounds__(256) relu_mask_kernel(const float* dout, const float* y, float* dy, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) dy[e] = y[e] > 0.f ? dout[e] : 0.f;
}
// the user context's (graphEncoders.py:131): out = dropout_p(relu(y) + t) in one pass, keep bytes saved; and its backward:
// g = dropout'(dout) (written: the residual path's gradient), dy = g [y > 0]
__global__ void __launch_bounds__(256) relu_res_drop_fwd_kernel(const float* y, const float* t, float* out, uint8_t* mask, long n, float p,
                                                                unsigned seed) {
    const float scale = 1.f / (1.f - p);
    const unsigned thr = drop_threshold(p);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float v = fmaxf(y[e], 0.f) + t[e];
        if (mask) {
            const uint8_t keep = drop_keep(seed, e, thr);
            mask[e] = keep;
            out[e] = keep ? v * scale : 0.f;
        } else {
            out[e] = v;
        }
    }
}
__global__ void __launch_bounds__(256) drop_relu_bwd_kernel(const float* dout, const uint8_t* mask, float scale, const float* y, float* dt,
                                                            float* dy, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const float g = mask ? (mask[e] ? dout[e] * scale : 0.f) : dout[e];
        dt[e] = g;
        dy[e] = y[e] > 0.f ? g : 0.f;
    }
}
// dZ = dOut * [out - Xres > 0]   (out = relu(Z) + Xres  =>  Z > 0  <=>  out - Xres > 0)
__global__ void __launch_bounds__(256) relu_res_mask_kernel(const float* dout, const float* out, const float* xres, float* dz, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256)
        dz[e] = (out[e] - xres[e]) > 0.f ? dout[e] : 0.f;
}
// dr[b][c] = sum_j dP[b][j][c]
__global__ void __launch_bounds__(256) sum_nodes_kernel(const float* dP, float* dr, int B, int n, int d, long ld) {
    const long total = (long)B * d;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long b = e / d; const int c = (int)(e - b * d);
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < n; ++j) s += dP[(b * n + j) * ld + c];     // (independent loads, one add chain in node order)
        dr[e] = s;
    }
}

// =================================================================================================
// T3. ScaledDotProductAttention pooling backward
// =================================================================================================
// forward: a_j = x_j.kq/sqrt(d) (mask -> -1e9), alpha = softmax(a), out = sum_j alpha_j x_j
// given dout [B,d] and the saved alpha [B,n]:
//   dalpha_j = dout.x_j ; da_j = alpha_j (dalpha_j - sum_k alpha_k dalpha_k)   (masked j: alpha = 0 -> 0;
//   an all-masked row is uniform and its da is the true softmax gradient, but a is constant there: da is dropped)
//   dx_j = alpha_j dout + da_j kq / sqrt(d)   (masked nodes: only the alpha term);  dkq = sum_j da_j x_j / sqrt(d)
struct PoolBwdArgs {
    const float* feat; long ld_b; const float* kq; const uint8_t* mask; const float* alpha; const float* dout;
    float* dfeat; long ldd_b; float* dkq; int B, n, d; float sqrt_d; int accumulate_dfeat;
    long ld_dout;       // row stride of dout (0: d)
};
__global__ void __launch_bounds__(256) attn_pool_bwd_kernel(const PoolBwdArgs g) {
    __shared__ float sd[DIGAT_MAX_NODES];
    __shared__ float sda[DIGAT_MAX_NODES];
    __shared__ float sal[DIGAT_MAX_NODES];      // alpha of the row: the last loop reads it between its stores (no reload from memory)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d4 = g.d >> 2, n = g.n;
    const float4* F4 = reinterpret_cast<const float4*>(g.feat + (long)b * g.ld_b);
    const float4* K4 = reinterpret_cast<const float4*>(g.kq + (long)b * g.d);
    const float4* D4 = reinterpret_cast<const float4*>(g.dout + (long)b * (g.ld_dout ? g.ld_dout : (long)g.d));
    float4* DF4 = reinterpret_cast<float4*>(g.dfeat + (long)b * g.ldd_b);
    const float* al = g.alpha + (long)b * n;
    for (int j = wave; j < n; j += 4) {
        float part = 0.f;
        for (int c4 = lane; c4 < d4; c4 += 64) {
            const float4 x = F4[(long)j * d4 + c4], q = D4[c4];
            part = fmaf(x.w, q.w, fmaf(x.z, q.z, fmaf(x.y, q.y, fmaf(x.x, q.x, part))));
        }
        part = wave_sum(part);
        // a weight of exactly zero (a masked node of a row that has live ones) takes no part: its row may never have been written
        // (dead nodes of a larger news graph) and 0 x NaN would poison dot, dkq and with them the whole row — the forward's rule.
        // Its dalpha is dropped here, so its da is 0 and dx_j = 0 x kq + 0 x dout = 0; below its x_j is zeroed before it meets dkq.
        if (lane == 0) sd[j] = al[j] != 0.f ? part : 0.f;
    }
    __syncthreads();
    if (tid < n) {
        float dot = 0.f;
        for (int k = 0; k < n; ++k) dot += al[k] * sd[k];
        const bool masked = g.mask[(long)b * n + tid] == 0;
        sda[tid] = masked ? 0.f : al[tid] * (sd[tid] - dot) / g.sqrt_d;
        sal[tid] = al[tid];
    }
    __syncthreads();
    for (int c4 = tid; c4 < d4; c4 += 256) {
        const float4 q = D4[c4], k = K4[c4];
        float4 dk = f4_zero();
        for (int j = 0; j < n; ++j) {
            const float a = sal[j], da = sda[j];
            const float4 xl = F4[(long)j * d4 + c4];
            const float4 x = a != 0.f ? xl : f4_zero();        // (a select after the load, not a branch: the loads stay in flight together)
            float4 dx = make_float4(fmaf(da, k.x, a * q.x), fmaf(da, k.y, a * q.y), fmaf(da, k.z, a * q.z), fmaf(da, k.w, a * q.w));
            if (g.accumulate_dfeat) dx = f4_add(DF4[(long)j * d4 + c4], dx);
            DF4[(long)j * d4 + c4] = dx;
            dk.x = fmaf(da, x.x, dk.x); dk.y = fmaf(da, x.y, dk.y); dk.z = fmaf(da, x.z, dk.z); dk.w = fmaf(da, x.w, dk.w);
        }
        reinterpret_cast<float4*>(g.dkq + (long)b * g.d)[c4] = dk;
    }
}

// =================================================================================================
// T4. topic pooling backward (scatter_softmax + scatter_sum)
// =================================================================================================
// forward: a_t = x_t.kq/sqrt(d); alpha = segment_softmax(a, idx); T_c = sum_{t in c} alpha_t x_t
// given dT [B,C1,d] and saved alpha [B,H]:
//   dalpha_t = dT_{idx_t}.x_t ; da_t = alpha_t (dalpha_t - sum_{u in seg} alpha_u dalpha_u)
//   dx_t = alpha_t dT_{idx_t} + da_t kq/sqrt(d) ; dkq = sum_t da_t x_t / sqrt(d)
struct TopicBwdArgs {
    const float* Xu; long ld_b; const float* kq; const int64_t* idx; const float* alpha; const float* dT;
    float* dXu; long ldd_b; float* dkq; int B, H, C1, d; float sqrt_d;
    int zero_to;        // > H: rows H .. zero_to - 1 of dXu (the topic nodes: no gradient from the pooling) are zero-filled here
};
__global__ void __launch_bounds__(256) topic_pool_bwd_kernel(const TopicBwdArgs g) {
    __shared__ float sd[TOPIC_MAX_H];
    __shared__ float sda[TOPIC_MAX_H];
    __shared__ int sidx[TOPIC_MAX_H];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d4 = g.d >> 2, H = g.H;
    const float4* F4 = reinterpret_cast<const float4*>(g.Xu + (long)b * g.ld_b);
    const float4* K4 = reinterpret_cast<const float4*>(g.kq + (long)b * g.d);
    const float4* T4 = reinterpret_cast<const float4*>(g.dT + (long)b * g.C1 * g.d);
    float4* DX4 = reinterpret_cast<float4*>(g.dXu + (long)b * g.ldd_b);
    const float* al = g.alpha + (long)b * H;
    for (int t = tid; t < H; t += 256) {
        const long v = g.idx[(long)b * H + t];
        sidx[t] = (v >= 0 && v < g.C1) ? (int)v : -1;
    }
    __syncthreads();
    // (round 6: this launch was a chain of dependent round trips — a history row at a time per wave here, a row at a time per channel
    // thread below with 100 of 256 threads busy at d = 400: 43 us per call.  Four rows per wave step now, and below five rows in
    // flight per thread with the two halves of the workgroup taking half of the history rows each.)
    for (int t0 = wave; t0 < H; t0 += 16) {
        float part[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = min(t0 + 4 * k, H - 1);
            const int c = max(sidx[t], 0);
            float p = 0.f;
            for (int c4 = lane; c4 < d4; c4 += 64) {
                const float4 x = F4[(long)t * d4 + c4], q = T4[(long)c * d4 + c4];
                p = fmaf(x.w, q.w, fmaf(x.z, q.z, fmaf(x.y, q.y, fmaf(x.x, q.x, p))));
            }
            part[k] = p;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + 4 * k;
            const float v = wave_sum(part[k]);
            if (lane == 0 && t < H) sd[t] = sidx[t] >= 0 ? v : 0.f;
        }
    }
    __syncthreads();
    for (int t = tid; t < H; t += 256) {
        const int c = sidx[t];
        float dot = 0.f;
        for (int u = 0; u < H; ++u) if (sidx[u] == c) dot += al[u] * sd[u];
        sda[t] = c >= 0 ? al[t] * (sd[t] - dot) / g.sqrt_d : 0.f;
    }
    __syncthreads();
    __shared__ float4 dk_half[128];
    const bool split = d4 <= 128;                              // the channels fit half a workgroup: the halves share the history rows
    const int half = split ? (tid >> 7) : 0, cstep = split ? 128 : 256;
    const int per = split ? (H + 1) / 2 : H;
    const int t_lo = half * per, t_hi = min(H, t_lo + per);
    const int z_lo = split ? (half == 0 ? H : H + (g.zero_to - H + 1) / 2) : H;
    const int z_hi = split ? (half == 0 ? min(g.zero_to, H + (g.zero_to - H + 1) / 2) : g.zero_to) : g.zero_to;
    for (int c4 = split ? (tid & 127) : tid; c4 < (split ? 128 : d4); c4 += cstep) {
        const bool live = c4 < d4;
        const int cc = live ? c4 : d4 - 1;
        const float4 k = K4[cc];
        float4 dk = f4_zero();
        for (int t0 = t_lo; t0 < t_hi; t0 += 5) {
            float4 x[5], q[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int t = min(t0 + u, t_hi - 1);
                x[u] = F4[(long)t * d4 + cc];
                q[u] = T4[(long)max(sidx[t], 0) * d4 + cc];
            }
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int t = t0 + u;
                if (t < t_hi) {
                    const float a = al[t], da = sda[t];
                    const float4 qv = sidx[t] >= 0 ? q[u] : f4_zero();
                    if (live) DX4[(long)t * d4 + c4] = make_float4(fmaf(da, k.x, a * qv.x), fmaf(da, k.y, a * qv.y), fmaf(da, k.z, a * qv.z),
                                                                   fmaf(da, k.w, a * qv.w));
                    dk.x = fmaf(da, x[u].x, dk.x); dk.y = fmaf(da, x[u].y, dk.y); dk.z = fmaf(da, x[u].z, dk.z); dk.w = fmaf(da, x[u].w, dk.w);
                }
            }
        }
        if (live) for (int t = z_lo; t < z_hi; ++t) DX4[(long)t * d4 + c4] = f4_zero();
        if (split) {                                           // dk = (rows of the first half, in order) + (rows of the second half, in order)
            if (half == 1) dk_half[c4] = dk;
            __syncthreads();
            if (half == 0 && live) reinterpret_cast<float4*>(g.dkq + (long)b * g.d)[c4] = f4_add(dk, dk_half[c4]);
        } else if (live) {
            reinterpret_cast<float4*>(g.dkq + (long)b * g.d)[c4] = dk;
        }
    }
}

// =================================================================================================
// T5. Eq. 8 backward
// =================================================================================================
// (a) dalpha'[i][j] = dZ_i . h_j, then through (dropout,) softmax, mask and leaky_relu to ds[i][j].
//     One workgroup per row b; dZ and h stream through LDS in channel chunks; thread per (i,j) tile 2x2.
struct DsArgs {
    const float* dZ; const float* Hh; const float* alpha; const float* s_pre; const uint8_t* A;
    const uint8_t* amask; float ascale;      // alpha dropout (mask [B,n,n] or NULL)
    float* ds; int B, n, d;
    // round 6: dZ = dOut [out - Xres > 0] is formed HERE, on the way in, and written to dZ_out for the launches that follow (dh, the
    // pairwise backward) — the element-wise launch that used to make it is gone (dOut != NULL; dZ is then ignored)
    const float* dOut; const float* out; const float* Xres; float* dZ_out;
    const int* skip_if;      // optional device int: the launch returns at once when *skip_if != 0 (the entry-wise kernels do this batch)
};
constexpr int DS_CH = 32;     // channels per LDS chunk
constexpr int DS_MAXT = 16;   // 16x16 tiles per wave: ceil(n/16)^2 <= 64 over four waves (n <= 128)
// dalpha' = dZ h^T on the fp32 matrix cores (v_mfma_f32_16x16x4_f32; the VALU version, a thread per 3x3 block of pairs, ran
// 127 us per user-graph launch at 320 rows for 0.6 GFLOP): four waves share the ceil(n/16)^2 output tiles, dZ and h pass through
// LDS in 32-channel chunks as [node][33] images (rows >= n zero).
__global__ void __launch_bounds__(256) xattn_ds_kernel(const DsArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (g.skip_if && *g.skip_if != 0) return;
    const int n = g.n, d = g.d, b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int nt = (n + 15) >> 4, n16 = nt * 16;
    float* Zs = reinterpret_cast<float*>(smem);               // [n16][DS_CH+1]
    float* Hs = Zs + n16 * (DS_CH + 1);                       // [n16][DS_CH+1]
    float* G = Hs + n16 * (DS_CH + 1);                        // [n][n] dalpha
    const float* Zb = g.dZ + (long)b * n * d;                  // (dOut's row when the launch forms dZ itself)
    const float* Hb = g.Hh + (long)b * n * d;
    v4f acc[DS_MAXT];
    int zoff[DS_MAXT], hoff[DS_MAXT];          // LDS offsets of this lane's operands per tile (-1: no such tile)
#pragma unroll
    for (int t = 0; t < DS_MAXT; ++t) {
        acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
        const int tile = wave + 4 * t;
        const int ti = tile / nt, tj = tile - ti * nt;
        zoff[t] = tile < nt * nt ? (16 * ti + lr) * (DS_CH + 1) + lq : -1;
        hoff[t] = (16 * tj + lr) * (DS_CH + 1) + lq;
    }
    // this thread's float4 slots of a chunk image (8 per node row): loads are clamped and straight-line, all in flight together
    constexpr int DS_SLOTS = (DIGAT_MAX_NODES * (DS_CH / 4) + 255) / 256;      // 4
    int srow[DS_SLOTS], sc4[DS_SLOTS];
#pragma unroll
    for (int u = 0; u < DS_SLOTS; ++u) {
        const int e = tid + 256 * u;
        srow[u] = e >> 3; sc4[u] = e & 7;
    }
    float4 zv[DS_SLOTS], hv[DS_SLOTS], ov[DS_SLOTS], xv[DS_SLOTS];
    const bool make_z = g.dOut != nullptr;                     // launch-uniform
    const float* Ob = make_z ? g.out + (long)b * n * d : Zb;
    const float* Xb = make_z ? g.Xres + (long)b * n * d : Zb;
    if (make_z) Zb = g.dOut + (long)b * n * d;
    auto request = [&](int c0) {                               // the next chunk is in flight during the MFMAs of this one
#pragma unroll
        for (int u = 0; u < DS_SLOTS; ++u) {
            const long off = (long)min(srow[u], n - 1) * d + min(c0 + 4 * sc4[u], d - 4);
            zv[u] = *reinterpret_cast<const float4*>(Zb + off);
            hv[u] = *reinterpret_cast<const float4*>(Hb + off);
            if (make_z) {
                ov[u] = *reinterpret_cast<const float4*>(Ob + off);
                xv[u] = *reinterpret_cast<const float4*>(Xb + off);
            }
        }
    };
    request(0);
    for (int c0 = 0; c0 < d; c0 += DS_CH) {
        if (make_z) {                                          // dZ = dOut [out - Xres > 0]: relu_res_mask_kernel's arithmetic
#pragma unroll
            for (int u = 0; u < DS_SLOTS; ++u) {
                zv[u] = make_float4((ov[u].x - xv[u].x) > 0.f ? zv[u].x : 0.f, (ov[u].y - xv[u].y) > 0.f ? zv[u].y : 0.f,
                                    (ov[u].z - xv[u].z) > 0.f ? zv[u].z : 0.f, (ov[u].w - xv[u].w) > 0.f ? zv[u].w : 0.f);
                if (srow[u] < n && c0 + 4 * sc4[u] < d)
                    *reinterpret_cast<float4*>(g.dZ_out + (long)b * n * d + (long)srow[u] * d + c0 + 4 * sc4[u]) = zv[u];
            }
        }
#pragma unroll
        for (int u = 0; u < DS_SLOTS; ++u) {
            if (srow[u] < n16) {
                const bool ok = srow[u] < n && c0 + 4 * sc4[u] < d;
                float* zp = Zs + srow[u] * (DS_CH + 1) + 4 * sc4[u];
                float* hp = Hs + srow[u] * (DS_CH + 1) + 4 * sc4[u];
                zp[0] = ok ? zv[u].x : 0.f; zp[1] = ok ? zv[u].y : 0.f; zp[2] = ok ? zv[u].z : 0.f; zp[3] = ok ? zv[u].w : 0.f;
                hp[0] = ok ? hv[u].x : 0.f; hp[1] = ok ? hv[u].y : 0.f; hp[2] = ok ? hv[u].z : 0.f; hp[3] = ok ? hv[u].w : 0.f;
            }
        }
        __syncthreads();
        if (c0 + DS_CH < d) request(c0 + DS_CH);
#pragma unroll
        for (int ks = 0; ks < DS_CH / 4; ++ks) {
#pragma unroll
            for (int t = 0; t < DS_MAXT; ++t)
                if (zoff[t] >= 0)                              // wave-uniform
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Zs[zoff[t] + 4 * ks], Hs[hoff[t] + 4 * ks], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < DS_MAXT; ++t) {
        const int tile = wave + 4 * t;
        if (tile >= nt * nt) continue;
        const int ti = tile / nt, tj = tile - ti * nt;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * ti + 4 * lq + r, j = 16 * tj + lr;
            if (i < n && j < n) {
                float v = acc[t][r];
                if (g.amask) v = g.amask[((long)b * n + i) * n + j] ? v * g.ascale : 0.f;
                G[i * n + j] = v;
            }
        }
    }
    __syncthreads();
    // softmax backward per centre i, then mask and leaky_relu'
    const float* al = g.alpha + (long)b * n * n;
    // row dots sum_k alpha_ik dalpha_ik once per centre (a wave per row, lanes over k in a fixed pattern), not once per pair
    float* dots = Zs;                                          // [n]: the chunk images are free now
    for (int i = wave; i < n; i += 4) {
        float part = 0.f;
        for (int k = lane; k < n; k += 64) part = fmaf(al[i * n + k], G[i * n + k], part);
        part = wave_sum(part);
        if (lane == 0) dots[i] = part;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += nth) {
        const int i = e / n;
        const float dot = dots[i];
        float de = al[e] * (G[e] - dot);
        if (g.A[(long)b * n * n + e] == 0) de = 0.f;                       // masked_fill: no gradient to the score
        const float sp = g.s_pre[(long)b * n * n + e];
        g.ds[(long)b * n * n + e] = de * (sp > 0.f ? 1.f : 0.2f);
    }
}
// every launch of it: the two [n16][33] chunk images and the row's n x n block in dynamic LDS, opted in above 64 KB
static int launch_ds(const DsArgs& t, hipStream_t st) {
    const int n16 = (t.n + 15) / 16 * 16;
    const size_t lds = ((size_t)2 * n16 * (DS_CH + 1) + (size_t)t.n * t.n) * 4;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)xattn_ds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(xattn_ds_kernel, dim3(t.B), dim3(256), lds, st, t);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// (b) pairwise backward: with x_ijc = P'_jc + Q_ic (recomputed), g_ijc = ds_ij a_c [x_ijc > 0]:
//     dQ_ic = sum_j g_ijc ; dP'_jc = sum_i g_ijc ; da_c += sum_ij ds_ij relu(x_ijc)
//     One workgroup per (row, 64-channel chunk); P' and Q pass through LDS; pass 1: thread (i, c) over j,
//     pass 2: thread (j, c) over i.  da partials [B][d] are reduced over b by colsum_kernel.
struct PairBwdArgs { const float* P; const float* Q; const float* a; const float* ds; float* dP; float* dQ; float* da_part; int B, n, d;
                     long ldo;         // row stride of dP / dQ (d, or 3 d when they are columns of one [dh | dP' | dQ] matrix)
                     float* dr;        // optional [B,d]: dr[b] = sum_j dP'[b,j] (K3's gradient: the sum_nodes launch of round 5)
                     const int* skip_if; };
template <int PB_CH>      // channels per workgroup: 64; 32 for graphs of more than 112 nodes (LDS: 6 n^2 + (12 PB_CH + 8) n bytes <= 160 KB)
__global__ void __launch_bounds__(1024) xattn_pair_bwd_kernel(const PairBwdArgs g) {
    constexpr int C4 = PB_CH / 4, C4S = PB_CH == 64 ? 4 : 3;       // float4 slots per node row, log2
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (g.skip_if && *g.skip_if != 0) return;
    const int n = g.n, d = g.d, b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    float* Ps = reinterpret_cast<float*>(smem);      // [n][PB_CH]
    float* Qs = Ps + n * PB_CH;                      // [n][PB_CH]
    float* Ds = Qs + n * PB_CH;                      // [n][n] ds
    float* Da = Ds + n * n;                          // [n][PB_CH] per-centre partial of da
    // ds is zero off the adjacency (a few entries per row on MIND graphs): compact lists of its non-zero columns per row and
    // rows per column, built once, so that the two passes walk ~9 pairs per node instead of n
    uint8_t* rowlist = reinterpret_cast<uint8_t*>(Da + n * PB_CH);    // [n][n]
    uint8_t* collist = rowlist + n * n;                               // [n][n]
    int* rowcnt = reinterpret_cast<int*>(collist + ((n * n + 3) & ~3));   // [n]
    int* colcnt = rowcnt + n;                                         // [n]
    const float* Pb = g.P + (long)b * n * d;
    const float* Qb = g.Q + (long)b * n * d;
    // every global read of the workgroup is requested before the first LDS store: ds (up to 16 per thread at n = 128) and this
    // chunk's P', Q rows as float4 (clamped, straight-line: a conditional per load makes the compiler wait after each one)
    const int c0 = blockIdx.y * PB_CH;
    float dsv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 1024 * u;
        dsv[u] = (u < 5 || e < n * n) ? g.ds[(long)b * n * n + min(e, n * n - 1)] : 0.f;     // u < 5 covers n <= 71 without a branch
    }
    float4 pv[2], qv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = tid + 1024 * u;                          // float4 slot: node e / C4, channels 4 (e % C4) ..
        const long off = (long)min(e >> C4S, n - 1) * d + min(c0 + 4 * (e & (C4 - 1)), d - 4);
        pv[u] = *reinterpret_cast<const float4*>(Pb + off);
        qv[u] = *reinterpret_cast<const float4*>(Qb + off);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + 1024 * u;
        if (e < n * n) Ds[e] = dsv[u];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = tid + 1024 * u;
        if ((e >> C4S) < n) {
            const bool ok = c0 + 4 * (e & (C4 - 1)) < d;
            *reinterpret_cast<float4*>(Ps + 4 * e) = ok ? pv[u] : f4_zero();
            *reinterpret_cast<float4*>(Qs + 4 * e) = ok ? qv[u] : f4_zero();
        }
    }
    __syncthreads();
    if (tid < n) {
        int c = 0;
        for (int j = 0; j < n; ++j) if (Ds[tid * n + j] != 0.f) rowlist[tid * n + c++] = (uint8_t)j;
        rowcnt[tid] = c;
    } else if (tid < 2 * n) {
        const int j = tid - n;
        int c = 0;
        for (int i = 0; i < n; ++i) if (Ds[i * n + j] != 0.f) collist[j * n + c++] = (uint8_t)i;
        colcnt[j] = c;
    }
    {   // one 64-channel chunk per workgroup (grid.y): seven times the workgroups of one-per-row, which left the chip a
        // quarter full on latency-bound passes (250 us per user-graph launch at 320 rows; the lists are rebuilt per chunk)
        __syncthreads();
        for (int e = tid; e < n * PB_CH; e += nth) {          // pass 1: centre i, channel c
            const int i = e / PB_CH, c = e - i * PB_CH;
            if (c0 + c >= d) { Da[e] = 0.f; continue; }
            const float q = Qs[e], ac = g.a[c0 + c];
            float dq = 0.f, da = 0.f;
            const int cnt = rowcnt[i];                     // pairs off the list have ds = 0: fma(0, ., acc) = acc, nothing is lost
            for (int k = 0; k < cnt; ++k) {
                const int j = rowlist[i * n + k];          // ascending j, as the full loop
                const float dsv = Ds[i * n + j];
                const float x = Ps[j * PB_CH + c] + q;
                if (x > 0.f) { dq = fmaf(dsv, ac, dq); da = fmaf(dsv, x, da); }
            }
            g.dQ[((long)b * n + i) * g.ldo + c0 + c] = dq;
            Da[e] = da;
        }
        // (walking the lists of a thread's nodes together, one step of each per iteration, to overlap their dependent LDS reads
        // costs more than it hides: every node then pays for the longest list — 135 -> 400 us per user-graph launch)
        if (g.dr) __syncthreads();                            // pass 2 overwrites P' with dP' (for the sum over the nodes): pass 1 must be done with it
        for (int e = tid; e < n * PB_CH; e += nth) {          // pass 2: neighbour j, channel c
            const int j = e / PB_CH, c = e - j * PB_CH;
            if (c0 + c >= d) continue;
            const float p = Ps[e], ac = g.a[c0 + c];
            float dp = 0.f;
            const int cnt = colcnt[j];
            for (int k = 0; k < cnt; ++k) {
                const int i = collist[j * n + k];          // ascending i
                const float x = p + Qs[i * PB_CH + c];
                if (x > 0.f) dp = fmaf(Ds[i * n + j], ac, dp);
            }
            g.dP[((long)b * n + j) * g.ldo + c0 + c] = dp;
            if (g.dr) Ps[e] = dp;
        }
        __syncthreads();
        for (int c = tid; c < PB_CH; c += nth) {              // da partial of this row, centres in order
            if (c0 + c >= d) continue;
            float s = 0.f;
            for (int i = 0; i < n; ++i) s += Da[i * PB_CH + c];
            g.da_part[(long)b * d + c0 + c] = s;
        }
        if (g.dr) {
            for (int c = tid - 64; c >= 0 && c < PB_CH; c += nth) {      // the second wave: dr of this row, nodes in order (sum_nodes_kernel's)
                if (c0 + c >= d) continue;
                float s = 0.f;
                for (int j = 0; j < n; ++j) s += Ps[j * PB_CH + c];
                g.dr[(long)b * d + c0 + c] = s;
            }
        }
    }
}

// (c) dh[j][c] = sum_i alpha'[i][j] dZ[i][c]: the aggregation kernel with alpha transposed and a plain epilogue
struct AggTArgs { const float* alpha; const uint8_t* amask; float ascale; const float* dZ; float* dh; int B, n, d; long ldh; const int* skip_if; };
__global__ void __launch_bounds__(256) xattn_aggT_kernel(const AggTArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (g.skip_if && *g.skip_if != 0) return;
    float* As = reinterpret_cast<float*>(smem);        // [n][n] alpha' (after dropout)
    const int n = g.n, d = g.d, b = blockIdx.x, tid = threadIdx.x;
    for (int e = tid; e < n * n; e += 256) {
        float v = g.alpha[(long)b * n * n + e];
        if (g.amask) v = g.amask[(long)b * n * n + e] ? v * g.ascale : 0.f;
        As[e] = v;
    }
    __syncthreads();
    // alpha' is zero off the adjacency: the rows i with alpha'[i][j] != 0, per column j, once (ascending i: the full loop's order)
    uint8_t* collist = reinterpret_cast<uint8_t*>(As + n * n);         // [n][n]
    int* colcnt = reinterpret_cast<int*>(collist + ((n * n + 3) & ~3)); // [n]
    if (tid < n) {
        int c = 0;
        for (int i = 0; i < n; ++i) if (As[i * n + tid] != 0.f) collist[tid * n + c++] = (uint8_t)i;
        colcnt[tid] = c;
    }
    __syncthreads();
    const float* Zb = g.dZ + (long)b * n * d;
    for (int e = tid; e < n * (d >> 2); e += 256) {
        const int j = e / (d >> 2), c4 = e - j * (d >> 2);
        float4 acc = f4_zero();
        const int cnt = colcnt[j];
        for (int k = 0; k < cnt; ++k) {
            const int i = collist[j * n + k];
            const float a = As[i * n + j];
            const float4 z = reinterpret_cast<const float4*>(Zb + (long)i * d)[c4];
            acc.x = fmaf(a, z.x, acc.x); acc.y = fmaf(a, z.y, acc.y); acc.z = fmaf(a, z.z, acc.z); acc.w = fmaf(a, z.w, acc.w);
        }
        reinterpret_cast<float4*>(g.dh + ((long)b * n + j) * g.ldh)[c4] = acc;
    }
}
// every launch of it: alpha' [n][n], the column lists [n][n] bytes and their counts [n] in dynamic LDS, opted in above 64 KB
static int launch_aggT(const AggTArgs& t, hipStream_t st) {
    const size_t lds = (size_t)t.n * t.n * 4 + (((size_t)t.n * t.n + 3) & ~(size_t)3) + (size_t)t.n * 4;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)xattn_aggT_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(xattn_aggT_kernel, dim3(t.B), dim3(256), lds, st, t);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// (d) the same backward OVER THE ADJACENCY'S ENTRIES (round 6): the three launches above visit all n^2 pairs of a row (dalpha' on the
//     matrix cores, lists rebuilt per 64-channel chunk); a MIND user graph holds ~9 entries per node.  Two launches, a wave per node:
//       centre kernel (node = centre i): dZ_i = dOut_i [out_i - X_i > 0] (stored), dalpha'_ij = dZ_i . h_j over i's entries, the
//         dropout / softmax / mask / leaky_relu chain to ds_ij (the row is stored: zero off the entries), then dQ_i = sum_j g_ij and
//         this row's share of da, with x_ij = P'_j + Q_i recomputed;
//       node kernel (node = neighbour j): over the centres i that hold j — column j of the adjacency, or every centre without any
//         entry (its attention is uniform over all nodes) — dh_j = sum_i alpha'_ij dZ_i and dP'_j = sum_i g_ij.
//     da is summed over the centre kernel's workgroups and sum_j dP'_j (K3's gradient) over the nodes by two small launches.
//     Every sum runs in ascending node order: bit-reproducible, no atomics.
struct SpBwdArgs {
    const float* dOut; const float* out; const float* X; const float* h; const float* P; const float* Q; const float* a;
    const uint8_t* A; const float* alpha; const float* s_pre; const uint8_t* amask; float ascale;
    float* dZ; float2* wds;                         // centre kernel -> node kernel: dZ rows, and per (centre, node) the pair
                                                    // (alpha'_ij = drop_p(alpha)_ij, ds_ij): all the node kernel needs of a pair
    float* dQ; float* dh; float* dP; long ldg;      // rows of stride ldg
    float* da_part;                                 // [ceil(B n / 4), d]: one row per workgroup of the centre kernel
    int B, n, d4;
    const int* run_if;                              // device int: run iff != 0
};
constexpr int SPB_NBR = 4;
template <int U>      // float4 pieces per lane: d <= 256 U
__global__ void __launch_bounds__(256) xattn_sparse_bwd_centre_kernel(const SpBwdArgs g) {
    if (g.run_if && *g.run_if == 0) return;
    __shared__ float4 red[4][64 * U];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = g.n, d4 = g.d4;
    const long node = (long)blockIdx.x * 4 + wave;                 // a wave per centre (a workgroup per row of sixteen waves walking ~4 nodes
    const bool valid = node < (long)g.B * n;                       // each ran 110 us: one workgroup per CU, two rounds for 320 rows)
    const int b = (int)((valid ? node : 0) / n);
    unsigned c4l[U];
    float4 av[U], da_acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        c4l[u] = (unsigned)min(lane + 64 * u, d4 - 1);
        const float4 aa = reinterpret_cast<const float4*>(g.a)[c4l[u]];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();               // a = 0 on the padding lanes: they add nothing
        da_acc[u] = f4_zero();
    }
    const float4* Pb = reinterpret_cast<const float4*>(g.P) + (long)b * n * d4;
    const float4* Hb = reinterpret_cast<const float4*>(g.h) + (long)b * n * d4;
    if (valid) {
        const long rho = node;
        // everything whose address is known: straight-line, clamped loads
        const uint8_t* Ar = g.A + rho * n;
        const int j0 = min(lane, n - 1), j1 = min(lane + 64, n - 1);
        const uint8_t ab0 = Ar[j0], ab1 = Ar[j1];
        const float al0 = g.alpha[rho * n + j0], al1 = g.alpha[rho * n + j1];
        const float sp0 = g.s_pre[rho * n + j0], sp1 = g.s_pre[rho * n + j1];
        const uint8_t k0 = g.amask ? g.amask[rho * n + j0] : (uint8_t)1, k1 = g.amask ? g.amask[rho * n + j1] : (uint8_t)1;
        float4 dz[U], q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 go = reinterpret_cast<const float4*>(g.dOut)[rho * d4 + c4l[u]];
            const float4 o = reinterpret_cast<const float4*>(g.out)[rho * d4 + c4l[u]];
            const float4 x = reinterpret_cast<const float4*>(g.X)[rho * d4 + c4l[u]];
            q[u] = reinterpret_cast<const float4*>(g.Q)[rho * d4 + c4l[u]];
            const bool ok = lane + 64 * u < d4;                    // padding lanes carry zeros: they add nothing to the dot products
            dz[u] = make_float4(ok && (o.x - x.x) > 0.f ? go.x : 0.f, ok && (o.y - x.y) > 0.f ? go.y : 0.f,
                                ok && (o.z - x.z) > 0.f ? go.z : 0.f, ok && (o.w - x.w) > 0.f ? go.w : 0.f);
            if (ok) reinterpret_cast<float4*>(g.dZ)[rho * d4 + lane + 64 * u] = dz[u];
        }
        const bool e0 = lane < n && ab0 != 0, e1 = lane + 64 < n && ab1 != 0;
        const unsigned long long m0 = __ballot(e0), m1 = __ballot(e1);
        const int deg = __popcll(m0) + __popcll(m1);
        float4 dq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dq[u] = f4_zero();
        float ds0 = 0.f, ds1 = 0.f;
        if (deg > 0) {                                             // (an edgeless centre: every score is masked, no gradient to them)
            // dalpha'_ij = dZ_i . h_j over the entries, four neighbour rows in flight
            float G0 = 0.f, G1 = 0.f;
            unsigned long long w0 = m0, w1 = m1;
            while (w0 | w1) {
                int j[SPB_NBR], cnt = 0;
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t) {
                    if (w0) { j[t] = __builtin_ctzll(w0); w0 &= w0 - 1ull; ++cnt; }
                    else if (w1) { j[t] = 64 + __builtin_ctzll(w1); w1 &= w1 - 1ull; ++cnt; }
                    else j[t] = j[0];
                }
                float4 hv[SPB_NBR][U];
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t)
#pragma unroll
                    for (int u = 0; u < U; ++u) hv[t][u] = (Hb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t) {
                    if (t < cnt) {                                 // wave-uniform
                        float part = 0.f;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            part = fmaf(dz[u].w, hv[t][u].w, fmaf(dz[u].z, hv[t][u].z, fmaf(dz[u].y, hv[t][u].y, fmaf(dz[u].x, hv[t][u].x, part))));
                        const float e = wave_sum(part);
                        if (lane == (j[t] & 63)) { if (j[t] < 64) G0 = e; else G1 = e; }
                    }
                }
            }
            if (g.amask) { G0 = k0 ? G0 * g.ascale : 0.f; G1 = k1 ? G1 * g.ascale : 0.f; }
            const float dot = wave_sum(fmaf(al1, G1, al0 * G0));
            ds0 = e0 ? al0 * (G0 - dot) * (sp0 > 0.f ? 1.f : 0.2f) : 0.f;       // masked_fill: no gradient off the entries
            ds1 = e1 ? al1 * (G1 - dot) * (sp1 > 0.f ? 1.f : 0.2f) : 0.f;
            // dQ_i and da over the same entries, x_ij = P'_j + Q_i recomputed
            w0 = m0; w1 = m1;
            while (w0 | w1) {
                int j[SPB_NBR], cnt = 0;
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t) {
                    if (w0) { j[t] = __builtin_ctzll(w0); w0 &= w0 - 1ull; ++cnt; }
                    else if (w1) { j[t] = 64 + __builtin_ctzll(w1); w1 &= w1 - 1ull; ++cnt; }
                    else j[t] = j[0];
                }
                float4 pv[SPB_NBR][U];
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t)
#pragma unroll
                    for (int u = 0; u < U; ++u) pv[t][u] = (Pb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
                for (int t = 0; t < SPB_NBR; ++t) {
                    if (t < cnt) {
                        const float w = j[t] < 64 ? lane_bcast(ds0, j[t]) : lane_bcast(ds1, j[t] - 64);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float4 x = f4_add(pv[t][u], q[u]);
                            if (x.x > 0.f) { dq[u].x = fmaf(w, av[u].x, dq[u].x); da_acc[u].x = fmaf(w, x.x, da_acc[u].x); }
                            if (x.y > 0.f) { dq[u].y = fmaf(w, av[u].y, dq[u].y); da_acc[u].y = fmaf(w, x.y, da_acc[u].y); }
                            if (x.z > 0.f) { dq[u].z = fmaf(w, av[u].z, dq[u].z); da_acc[u].z = fmaf(w, x.z, da_acc[u].z); }
                            if (x.w > 0.f) { dq[u].w = fmaf(w, av[u].w, dq[u].w); da_acc[u].w = fmaf(w, x.w, da_acc[u].w); }
                        }
                    }
                }
            }
        }
        // (alpha' is zero off the entries of a centre that has any, and uniform x keep / (1 - p) on an edgeless one)
        const float wa0 = g.amask ? (k0 ? al0 * g.ascale : 0.f) : al0, wa1 = g.amask ? (k1 ? al1 * g.ascale : 0.f) : al1;
        if (lane < n) g.wds[rho * n + lane] = make_float2(wa0, ds0);
        if (lane + 64 < n) g.wds[rho * n + 64 + lane] = make_float2(wa1, ds1);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (lane + 64 * u < d4) reinterpret_cast<float4*>(g.dQ + rho * g.ldg)[lane + 64 * u] = dq[u];
    }
    // the workgroup's share of da (four centres, in order): one row of da_part per workgroup, summed over the workgroups afterwards
#pragma unroll
    for (int u = 0; u < U; ++u) red[wave][lane + 64 * u] = da_acc[u];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 s = red[0][lane + 64 * u];
            for (int w = 1; w < 4; ++w) s = f4_add(s, red[w][lane + 64 * u]);
            if (lane + 64 * u < d4) reinterpret_cast<float4*>(g.da_part + (long)blockIdx.x * d4 * 4)[lane + 64 * u] = s;
        }
    }
}

template <int U>
__global__ void __launch_bounds__(256) xattn_sparse_bwd_node_kernel(const SpBwdArgs g) {
    if (g.run_if && *g.run_if == 0) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = g.n, d4 = g.d4;
    const long node = (long)blockIdx.x * 4 + wave;                 // a wave per node
    if (node >= (long)g.B * n) return;
    const int b = (int)(node / n);
    unsigned c4l[U];
    float4 av[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        c4l[u] = (unsigned)min(lane + 64 * u, d4 - 1);
        const float4 aa = reinterpret_cast<const float4*>(g.a)[c4l[u]];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();
    }
    const float4* Zb = reinterpret_cast<const float4*>(g.dZ) + (long)b * n * d4;
    const float4* Qb = reinterpret_cast<const float4*>(g.Q) + (long)b * n * d4;
    const int i0 = min(lane, n - 1), i1 = min(lane + 64, n - 1);
    {
        const long rho = node;
        const int j = (int)(node - (long)b * n);
        // lane i (and 64 + i): centre i's pair for this node — one 8-byte load each (the column of a [B,n,n] array: strided)
        const float2 c0 = g.wds[((long)b * n + i0) * n + j], c1 = g.wds[((long)b * n + i1) * n + j];
        float4 pj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) pj[u] = reinterpret_cast<const float4*>(g.P)[rho * d4 + c4l[u]];
        const float w0 = lane < n ? c0.x : 0.f, w1 = lane + 64 < n ? c1.x : 0.f;              // alpha' = drop_p(alpha)
        const float t0 = lane < n ? c0.y : 0.f, t1 = lane + 64 < n ? c1.y : 0.f;              // ds (zero off the entries)
        // the centres that give this node anything: a weight (an entry that kept its alpha, or an edgeless centre) or a score gradient
        unsigned long long m0 = __ballot(w0 != 0.f || t0 != 0.f), m1 = __ballot(w1 != 0.f || t1 != 0.f);
        float4 dh[U], dp[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { dh[u] = f4_zero(); dp[u] = f4_zero(); }
        while (m0 | m1) {
            int i[SPB_NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < SPB_NBR; ++t) {
                if (m0) { i[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { i[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else i[t] = i[0];
            }
            float4 zv[SPB_NBR][U], qv[SPB_NBR][U];
#pragma unroll
            for (int t = 0; t < SPB_NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) { zv[t][u] = (Zb + (long)i[t] * d4)[c4l[u]]; qv[t][u] = (Qb + (long)i[t] * d4)[c4l[u]]; }
#pragma unroll
            for (int t = 0; t < SPB_NBR; ++t) {
                if (t < cnt) {                                     // wave-uniform
                    const float w = i[t] < 64 ? lane_bcast(w0, i[t]) : lane_bcast(w1, i[t] - 64);
                    const float sg = i[t] < 64 ? lane_bcast(t0, i[t]) : lane_bcast(t1, i[t] - 64);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        dh[u].x = fmaf(w, zv[t][u].x, dh[u].x); dh[u].y = fmaf(w, zv[t][u].y, dh[u].y);
                        dh[u].z = fmaf(w, zv[t][u].z, dh[u].z); dh[u].w = fmaf(w, zv[t][u].w, dh[u].w);
                        const float4 x = f4_add(pj[u], qv[t][u]);
                        if (x.x > 0.f) dp[u].x = fmaf(sg, av[u].x, dp[u].x);
                        if (x.y > 0.f) dp[u].y = fmaf(sg, av[u].y, dp[u].y);
                        if (x.z > 0.f) dp[u].z = fmaf(sg, av[u].z, dp[u].z);
                        if (x.w > 0.f) dp[u].w = fmaf(sg, av[u].w, dp[u].w);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (lane + 64 * u < d4) {
                reinterpret_cast<float4*>(g.dh + rho * g.ldg)[lane + 64 * u] = dh[u];
                reinterpret_cast<float4*>(g.dP + rho * g.ldg)[lane + 64 * u] = dp[u];
            }
        }
    }
}

// forward helper for training: scores before the mask (needed for leaky_relu') are recomputed by a tiny kernel
// from alpha? No: alpha loses the sign of masked-out scores but those get zero gradient anyway, and for
// unmasked entries sign(s) = sign(e) where e = log(alpha) + const is not recoverable -> the training forward
// saves s explicitly (xattn_score_kernel writes it when ScoreArgs.s_out is set).

// ---- the step's head and tail around the encoder (model.py:75-77, trainer.py:100) as two launches each way -------------------------
// logits_b = news_ctx_b . user_ctx_b is digat_row_logits; its backward: dnews = dlogit user, duser = dlogit news
__global__ void __launch_bounds__(256) row_logits_bwd_kernel(const float* dl, const float* nc, const float* uc, float* dn, float* du, long B, int d) {
    const long total = B * d;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const float gl = dl[e / d];
        dn[e] = gl * uc[e];
        du[e] = gl * nc[e];
    }
}
// loss = mean_b(-log_softmax(logits[b, :])[0]) (the clicked candidate is column 0) and d loss / d logits, one workgroup: a thread per
// impression, the mean as an ordered tree
__global__ void __launch_bounds__(256) click_loss_kernel(const float* logits, int B, int K, float* loss, float* dlogits) {
    __shared__ float red[256];
    float mine = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* row = logits + (long)b * K;
        float m = row[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, row[k]);
        float z = 0.f;
        for (int k = 0; k < K; ++k) z += expf(row[k] - m);
        // log_softmax as (x - m) - log z: m + log z would round at the size of the largest logit (half an ulp of 100 is 4e-6, of a
        // loss of about 1), the differences from the maximum do not
        const float lz = logf(z);
        mine += lz - (row[0] - m);
        for (int k = 0; k < K; ++k) dlogits[(long)b * K + k] = (expf((row[k] - m) - lz) - (k == 0 ? 1.f : 0.f)) / (float)B;
    }
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0] / (float)B;
}

// ---- the optimiser's step (trainer.py:30, :103-105): gradient clipping by the global norm + Adam as three launches ------------------
// torch's pair — clip_grad_norm_ (two multi-tensor norm launches, eight small ones, two multi-tensor multiplies) and the fused Adam
// (three launches, two of them for the ~70 small tensors) — is 15 launches and ~340 us of a 5 ms step that is one pass over the
// gradients and one over (p, g, m, v).  Here: chunk c = OPT_CHUNK consecutive elements of tensor chunk_tensor[c] from chunk_off[c]:
//   grad_sq_chunks_kernel   partial[c] = sum of g^2 over the chunk (a workgroup per chunk, ordered tree)
//   grad_sq_total_kernel    total = sum_c partial[c] in chunk order (one workgroup)
//   clip_adam_kernel        coef = min(1, max_norm / (sqrt(total) + 1e-6)) (max_norm <= 0: 1); g' = coef g (+ wd p: coupled L2, as
//                           torch.optim.Adam); m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2;
//                           p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)     — torch's fused kernel's arithmetic
// The gradients are not rewritten (clip_grad_norm_ scales them in place: an observable difference for a caller that reads .grad after
// the step).  Fixed summation order: the step is bit-reproducible.
constexpr int OPT_CHUNK = 16384;
struct OptTensor { float* p; const float* g; float* m; float* v; long n; float wd; int pad; };
__global__ void __launch_bounds__(256) grad_sq_chunks_kernel(const OptTensor* tensors, const int* chunk_tensor, const long* chunk_off, float* partial) {
    __shared__ float red[256];
    const OptTensor t = tensors[chunk_tensor[blockIdx.x]];
    const long o = chunk_off[blockIdx.x];
    const long end = min(t.n, o + OPT_CHUNK);
    float s = 0.f;
    if (((uintptr_t)(t.g + o) & 15) == 0) {
        const long n4 = (end - o) >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(t.g + o);
        for (long i = threadIdx.x; i < n4; i += 256) { const float4 v = g4[i]; s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s); }
        for (long i = o + 4 * n4 + threadIdx.x; i < end; i += 256) s = fmaf(t.g[i], t.g[i], s);
    } else {
        for (long i = o + threadIdx.x; i < end; i += 256) s = fmaf(t.g[i], t.g[i], s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(1024) grad_sq_total_kernel(const float* partial, int n, float* total) {
    __shared__ double red[1024];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += (double)partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = (float)red[0];
}
struct AdamArgs { const OptTensor* tensors; const int* chunk_tensor; const long* chunk_off; const float* total_sq; float max_norm;
                  float step_size, bc2_sqrt, beta1, beta2, eps; };
__global__ void __launch_bounds__(256) clip_adam_kernel(const AdamArgs a) {
    const OptTensor t = a.tensors[a.chunk_tensor[blockIdx.x]];
    const long o = a.chunk_off[blockIdx.x];
    const long end = min(t.n, o + OPT_CHUNK);
    float coef = 1.f;
    if (a.max_norm > 0.f) coef = fminf(a.max_norm / (sqrtf(*a.total_sq) + 1e-6f), 1.f);
    const float b1 = a.beta1, b2 = a.beta2, c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
    auto one = [&](float p, float g, float& m, float& v) -> float {
        g *= coef;
        if (t.wd != 0.f) g = fmaf(t.wd, p, g);
        m = fmaf(b1, m, c1 * g);
        v = fmaf(b2, v, c2 * g * g);
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        return p - a.step_size * (m / denom);
    };
    const bool vec = (((uintptr_t)(t.p + o) | (uintptr_t)(t.g + o) | (uintptr_t)(t.m + o) | (uintptr_t)(t.v + o)) & 15) == 0;
    long i0 = o;
    if (vec) {
        const long n4 = (end - o) >> 2;
        float4* p4 = reinterpret_cast<float4*>(t.p + o); const float4* g4 = reinterpret_cast<const float4*>(t.g + o);
        float4* m4 = reinterpret_cast<float4*>(t.m + o); float4* v4 = reinterpret_cast<float4*>(t.v + o);
        for (long i = threadIdx.x; i < n4; i += 256) {
            float4 p = p4[i], m = m4[i], v = v4[i];
            const float4 g = g4[i];
            p.x = one(p.x, g.x, m.x, v.x); p.y = one(p.y, g.y, m.y, v.y); p.z = one(p.z, g.z, m.z, v.z); p.w = one(p.w, g.w, m.w, v.w);
            p4[i] = p; m4[i] = m; v4[i] = v;
        }
        i0 = o + 4 * n4;
    }
    for (long i = i0 + threadIdx.x; i < end; i += 256) {
        float m = t.m[i], v = t.v[i];
        t.p[i] = one(t.p[i], t.g[i], m, v);
        t.m[i] = m; t.v[i] = v;
    }
}

static int grid_for(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

extern "C" {

int digat_row_logits_bwd(const float* dlogits, const float* news_ctx, const float* user_ctx, float* dnews, float* duser, int B, int d,
                         void* stream) {
    if (!dlogits || !news_ctx || !user_ctx || !dnews || !duser || B < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    hipLaunchKernelGGL(row_logits_bwd_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, (hipStream_t)stream, dlogits, news_ctx, user_ctx, dnews,
                       duser, (long)B, d);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_click_loss(const float* logits, int B, int K, float* loss, float* dlogits, void* stream) {
    if (!logits || !loss || !dlogits || B <= 0 || K <= 0) return DIGAT_ERR_ARG;
    hipLaunchKernelGGL(click_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, B, K, loss, dlogits);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// tensors [ntensors] (digat_opt_tensor, DEVICE memory), chunk_tensor [nchunks] int32 and chunk_off [nchunks] int64 (device): chunk c =
// the DIGAT_OPT_CHUNK elements of tensor chunk_tensor[c] from element chunk_off[c] on; scratch [nchunks + 1] floats (device)
int digat_clip_adam_step(const void* tensors, const int32_t* chunk_tensor, const int64_t* chunk_off, int nchunks, float* scratch, float max_norm,
                         float lr, float beta1, float beta2, float eps, int step, void* stream) {
    if (!tensors || !chunk_tensor || !chunk_off || !scratch || nchunks < 0 || step < 1 || beta1 < 0.f || beta1 >= 1.f || beta2 < 0.f || beta2 >= 1.f)
        return DIGAT_ERR_ARG;
    if (nchunks == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    float* total = scratch + nchunks;
    if (max_norm > 0.f) {
        hipLaunchKernelGGL(grad_sq_chunks_kernel, dim3(nchunks), dim3(256), 0, st, (const OptTensor*)tensors, (const int*)chunk_tensor,
                           (const long*)chunk_off, scratch);
        hipLaunchKernelGGL(grad_sq_total_kernel, dim3(1), dim3(1024), 0, st, (const float*)scratch, nchunks, total);
        DIGAT_CHECK_LAUNCH();
    }
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    AdamArgs a{(const OptTensor*)tensors, (const int*)chunk_tensor, (const long*)chunk_off, total, max_norm, (float)((double)lr / bc1),
               (float)sqrt(bc2), beta1, beta2, eps};
    hipLaunchKernelGGL(clip_adam_kernel, dim3(nchunks), dim3(256), 0, st, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_opt_chunk(void) { return OPT_CHUNK; }

// ---- generic primitives -----------------------------------------------------------------------------
// dx = dy @ W   (W [N,K] as in nn.Linear);  accumulate != 0: dx += ...
int digat_linear_bwd_input(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx,
                           int M, int N, int K, int accumulate, void* stream) {
    if (!dy || !w || !dx || M < 0 || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    if (N % 4 || lddy % 4) return DIGAT_ERR_SHAPE;
    // y[M,K] = dy[M,N] @ W[N,K]: the NT kernel with its weight operand read as [K_red = N, N_out = K]
    GemmArgs g = gemm_plain(dy, lddy, w, nullptr, dx, lddx, M, K, N, 1);
    if (accumulate) { g.epi = EPI_ACCUM; }
    return launch_gemm(g, (hipStream_t)stream);
}

// M is cut into slices (multiples of 32 rows, at most 64 of them): 256-row slices for the long products, but at least
// ~512 workgroups when M allows — the [B,d] linears' weight gradients (M = 320 rows: 47 of a step's 56 TN launches) ran as 50
// workgroups of five dependent 32-row steps each, 44 us apiece; as 10 slices x 25 tiles they are one step deep
static bool tn_bf16x6_ok(int M, int vec) {
    return vec && M >= 2048;
}
static int tn_slices(int M, int No, int Ni) {
    if (M >= 2048 && tn_bf16x6_ok(M, 1)) {           // 160 x 160 tiles: about two rounds of 512 workgroup slots, K tiles of 32 rows
        const int tiles = ((No + TNB - 1) / TNB) * ((Ni + TNB - 1) / TNB);
        int slices = (1024 + tiles - 1) / tiles;
        const int most = (M + 255) / 256;
        if (slices > most) slices = most;
        if (slices > 64) slices = 64;
        if (slices < 1) slices = 1;
        return slices;
    }
    const int tiles = ((No + 79) / 80) * ((Ni + 79) / 80);
    int slices = (M + 255) / 256;
    const int want = (512 + tiles - 1) / tiles, most = (M + 31) / 32;
    if (slices < want) slices = want;
    if (slices > most) slices = most;
    if (slices < 1) slices = 1;
    if (slices > 64) slices = 64;
    return slices;
}
// The same on the bf16 matrix cores (bf16x6, fp32-grade): W^T is split into `wsplit` (digat_split_weights_bytes(K, N)
// bytes, rewritten by every call: the weights change every optimiser step).  M >= 2048, K % 80 == 0, N % 8 == 0, N >= 32.
int digat_linear_bwd_input_x3(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx,
                              int M, int N, int K, int accumulate, void* wsplit, void* stream) {
    if (!dy || !w || !dx || !wsplit || M < 0 || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    if (M < 2048 || K % 80 || N % 8 || N < 32 || lddy % 4 || lddx % 4) return DIGAT_ERR_SHAPE;
    int rc = launch_split(w, w, w, K, 1, N, wsplit, (hipStream_t)stream, 1);
    if (rc) return rc;
    GemmArgs g = gemm_plain(dy, lddy, w, nullptr, dx, lddx, M, K, N, 0);
    g.wsplit = (const unsigned short*)wsplit;
    if (g_train_bf16) g.x1_segs = 7;           // digat_set_train_precision(1): one bf16 product
    if (accumulate) g.epi = EPI_ACCUM;
    return launch_gemm(g, (hipStream_t)stream);
}

// dx = addend + dy @ W (addend [M, K] with dx's row stride): the residual path's gradient joins in the epilogue
// w1 / w2 != NULL: W is the stack [w; w1; w2] of three [N / 3, K] matrices given separately (no concatenated copy is made)
// dmask != NULL: dx = (addend + dy @ W) through a dropout's keep bytes [M, K] (x dscale where kept, 0 elsewhere)
static int linear_bwd_input_x3_add(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx, const float* addend,
                                   int M, int N, int K, void* wsplit, void* stream, const float* w1 = nullptr, const float* w2 = nullptr,
                                   const uint8_t* dmask = nullptr, float dscale = 1.f) {
    if (!dy || !w || !dx || !wsplit || !addend || M < 0 || N <= 0 || K <= 0) return DIGAT_ERR_ARG;
    if (M < 2048 || K % 80 || N % 8 || N < 32 || lddy % 4 || lddx % 4 || ((w1 || w2) && (!w1 || !w2 || N % 3))) return DIGAT_ERR_SHAPE;
    int rc = w1 ? launch_split(w, w1, w2, K, 1, N, wsplit, (hipStream_t)stream, 2) : launch_split(w, w, w, K, 1, N, wsplit, (hipStream_t)stream, 1);
    if (rc) return rc;
    GemmArgs g = gemm_plain(dy, lddy, w, nullptr, dx, lddx, M, K, N, 0);
    g.wsplit = (const unsigned short*)wsplit;
    if (g_train_bf16) g.x1_segs = 7;
    g.epi = EPI_ADD_E0; g.e0 = addend; g.lde0 = lddx;
    g.dmask = dmask; g.lddm = K; g.dscale = dscale;
    return launch_gemm(g, (hipStream_t)stream);
}

size_t digat_linear_bwd_weight_workspace(int M, int No, int Ni) {
    return (size_t)tn_slices(M, No, Ni) * ((size_t)No * Ni + No) * 4;
}
// the product's launch arguments over `workspace`: M in tn_slices slices of whole 32-row steps, the slices' partial dW [slices][No, Ni]
// and, when the column sums are wanted, their partial db [slices][No] behind them; 16-byte loads where strides and addresses allow
static TnArgs tn_args(const float* dy, int64_t lddy, const float* x, int64_t ldx, bool want_db, int M, int No, int Ni, void* workspace) {
    const int slices = tn_slices(M, No, Ni);
    const int mper = ((M + slices - 1) / slices + 31) / 32 * 32;
    float* part = (float*)workspace;
    float* part_db = want_db ? part + (size_t)slices * No * Ni : nullptr;
    const int vec = (lddy % 4 == 0 && ldx % 4 == 0 && No % 4 == 0 && Ni % 4 == 0 &&
                     ((uintptr_t)dy & 15) == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    return TnArgs{dy, lddy, x, ldx, part, part_db, M, No, Ni, slices, mper > 0 ? mper : 32, vec};
}
// dW[No,Ni] (+)= dy[M,No]^T @ x[M,Ni] ;  db (+)= the leading db_cols <= No column sums of dy (db [db_cols], may be NULL)
static int linear_bwd_weight_dbn(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dW, float* db, int db_cols,
                                 int M, int No, int Ni, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dy || !x || !dW || !workspace || M < 0 || No <= 0 || Ni <= 0 || db_cols < 0 || db_cols > No) return DIGAT_ERR_ARG;
    if (workspace_bytes < digat_linear_bwd_weight_workspace(M, No, Ni)) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const TnArgs t = tn_args(dy, lddy, x, ldx, db != nullptr, M, No, Ni, workspace);
    // the weight-gradient product as an MFMA launch of the step (bench.py's train-step roofline): 2 M No Ni flops, both operands in, dW out
    ProfScope prof(DIGAT_KERNEL_LINEAR, 2.0 * M * (double)No * Ni, st, 4.0 * ((double)M * (No + Ni) + (double)No * Ni));
    if (tn_bf16x6_ok(M, t.vec)) {
        const int tiles = ((No + TNB - 1) / TNB) * ((Ni + TNB - 1) / TNB);
        if (g_train_bf16) hipLaunchKernelGGL(gemm_tn_bf16x6_kernel<true>, dim3(tiles, t.slices), dim3(256), 0, st, t);
        else hipLaunchKernelGGL(gemm_tn_bf16x6_kernel<false>, dim3(tiles, t.slices), dim3(256), 0, st, t);
    } else {
        const int tiles = ((No + 79) / 80) * ((Ni + 79) / 80);
        hipLaunchKernelGGL(gemm_tn_kernel, dim3(tiles, t.slices), dim3(256), 0, st, t);
    }
    DIGAT_CHECK_LAUNCH();
    const long nel = (long)No * Ni;
    if (db) hipLaunchKernelGGL(slice_reduce2_kernel, dim3(grid_for(nel + db_cols)), dim3(256), 0, st, (const float*)t.part, dW, nel,
                               (const float*)t.part_db, db, (long)db_cols, (long)No, t.slices, accumulate);
    else hipLaunchKernelGGL(slice_reduce_kernel, dim3(grid_for(nel)), dim3(256), 0, st, (const float*)t.part, dW, nel, t.slices, accumulate);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_linear_bwd_weight(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dW, float* db,
                            int M, int No, int Ni, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return linear_bwd_weight_dbn(dy, lddy, x, ldx, dW, db, No, M, No, Ni, accumulate, workspace, workspace_bytes, stream);
}

// collects the short products of one backward entry; flush() issues them as one product launch + one reduction launch.  A product
// that is not short (the bf16x6 path) is issued at once, as before.  `ws` must hold the sum of the collected products' workspaces.
struct TnGroup {
    TnGroupArgs a; ReduceGroupArgs r; int n; char* ws; size_t left; hipStream_t st; double flops, bytes;
    TnGroup(void* workspace, size_t bytes_, hipStream_t stream) : n(0), ws((char*)workspace), left(bytes_), st(stream), flops(0), bytes(0) {
        memset(&a, 0, sizeof(a)); memset(&r, 0, sizeof(r));
    }
    int add(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dW, float* db, int M, int No, int Ni, int accumulate) {
        if (!dy || !x || !dW || M < 0 || No <= 0 || Ni <= 0) return DIGAT_ERR_ARG;
        const size_t need = align_up(digat_linear_bwd_weight_workspace(M, No, Ni), 256);
        if (need > left) return DIGAT_ERR_WORKSPACE;
        const TnArgs t = tn_args(dy, lddy, x, ldx, db != nullptr, M, No, Ni, ws);
        if (tn_bf16x6_ok(M, t.vec)) return digat_linear_bwd_weight(dy, lddy, x, ldx, dW, db, M, No, Ni, accumulate, ws, left, st);
        if (n == TN_GROUP_MAX) { const int rc = flush(); if (rc) return rc; }
        ws += need; left -= need;
        a.p[n] = t;
        a.tiles[n] = ((No + 79) / 80) * ((Ni + 79) / 80);
        r.part[n] = t.part; r.out[n] = dW; r.n[n] = (long)No * Ni; r.part_b[n] = t.part_db; r.out_b[n] = db; r.nb[n] = db ? No : 0;
        r.slices[n] = t.slices; r.accumulate[n] = accumulate;
        flops += 2.0 * M * (double)No * Ni; bytes += 4.0 * ((double)M * (No + Ni) + (double)No * Ni);
        ++n;
        return DIGAT_OK;
    }
    int flush() {
        if (n == 0) return DIGAT_OK;
        int tiles = 0, slices = 0;
        long most = 0;
        for (int q = 0; q < n; ++q) {
            if (a.tiles[q] > tiles) tiles = a.tiles[q];
            if (a.p[q].slices > slices) slices = a.p[q].slices;
            if (r.n[q] + r.nb[q] > most) most = r.n[q] + r.nb[q];
        }
        {
            ProfScope prof(DIGAT_KERNEL_LINEAR, flops, st, bytes);
            hipLaunchKernelGGL(gemm_tn_group_kernel, dim3(tiles, slices, n), dim3(256), 0, st, a);
        }
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(slice_reduce_group_kernel, dim3(grid_for(most), n), dim3(256), 0, st, r);
        DIGAT_CHECK_LAUNCH();
        n = 0; flops = bytes = 0;
        return DIGAT_OK;
    }
};

int digat_colsum(const float* x, int64_t ldx, float* out, int M, int N, int accumulate, void* stream) {
    if (!x || !out || M < 0 || N <= 0) return DIGAT_ERR_ARG;
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, out, M, N, accumulate, (const int*)nullptr, 0);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint32_t seed, void* stream) {
    if (!x || !y || !mask || n < 0 || p < 0.f || p >= 1.f) return DIGAT_ERR_ARG;
    if (n == 0) return DIGAT_OK;
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, y, mask, (long)n, p, seed);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream) {
    if (!dy || !mask || !dx || n < 0) return DIGAT_ERR_ARG;
    if (n == 0) return DIGAT_OK;
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dy, mask, dx, (long)n, p);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_gate_fwd(const float* z, const float* l, int64_t ldl, const float* gl, float* out, int B, int d, void* stream) {
    if (!z || !l || !gl || !out) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, (hipStream_t)stream, z, l, (long)ldl, gl, (long)d, out,
                       (float*)nullptr, (uint8_t*)nullptr, 0.f, 0u, B, d, (const float*)nullptr);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_gate_bwd(const float* dout, const float* z, const float* l, int64_t ldl, const float* gl, float* dz, float* dl,
                   float* dg, int B, int d, void* stream) {
    if (!dout || !z || !l || !gl || !dz || !dl || !dg) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, (hipStream_t)stream, dout, z, l, (long)ldl, gl, (long)d,
                       (const uint8_t*)nullptr, 1.f, dz, dl, dg, (long)d, B, d);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_relu_res_fwd(const float* y, const float* t, float* out, int64_t n, void* stream) {
    if (!y || !t || !out) return DIGAT_ERR_ARG;
    if (n == 0) return DIGAT_OK;
    hipLaunchKernelGGL(relu_res_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, y, t, out, (long)n);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_relu_mask(const float* dout, const float* y, float* dy, int64_t n, void* stream) {
    if (!dout || !y || !dy) return DIGAT_ERR_ARG;
    if (n == 0) return DIGAT_OK;
    hipLaunchKernelGGL(relu_mask_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dout, y, dy, (long)n);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// ---- pooling ------------------------------------------------------------------------------------------
// forward that also returns the attention weights (needed by the backward)
// out rows of stride ld_out (0: d); node0 != NULL: node 0 of every row is copied there too (rows of stride ld_node0) — the news
// context's [l ; g] rows are written by the pooling launch itself
static int attn_pool_fwd_ld(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, float* out, long ld_out, float* node0,
                            long ld_node0, float* alpha_out, int B, int n, int d, void* stream, const float* addend = nullptr) {
    if (!feat || !kq || !mask || !out) return DIGAT_ERR_ARG;
    if (n > DIGAT_MAX_NODES || d % 4 || ld_out % 4 || ld_node0 % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    PoolArgs g{feat, (long)ld_b, kq, mask, addend, out, B, n, d, sqrtf((float)d), alpha_out, ld_out, node0, ld_node0};
    hipLaunchKernelGGL(attn_pool_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_attn_pool_fwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, float* out, float* alpha_out,
                        int B, int n, int d, void* stream) {
    return attn_pool_fwd_ld(feat, ld_b, kq, mask, out, 0, nullptr, 0, alpha_out, B, n, d, stream);
}
static int attn_pool_bwd_ld(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, const float* alpha,
                            const float* dout, long ld_dout, float* dfeat, int64_t ldd_b, float* dkq, int B, int n, int d,
                            int accumulate_dfeat, void* stream) {
    if (!feat || !kq || !mask || !alpha || !dout || !dfeat || !dkq) return DIGAT_ERR_ARG;
    if (n > DIGAT_MAX_NODES || d % 4 || ld_dout % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    PoolBwdArgs g{feat, (long)ld_b, kq, mask, alpha, dout, dfeat, (long)ldd_b, dkq, B, n, d, sqrtf((float)d), accumulate_dfeat, ld_dout};
    hipLaunchKernelGGL(attn_pool_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_attn_pool_bwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, const float* alpha,
                        const float* dout, float* dfeat, int64_t ldd_b, float* dkq, int B, int n, int d,
                        int accumulate_dfeat, void* stream) {
    return attn_pool_bwd_ld(feat, ld_b, kq, mask, alpha, dout, 0, dfeat, ldd_b, dkq, B, n, d, accumulate_dfeat, stream);
}
int digat_topic_pool_fwd_train(const float* Xu, const float* kq, const int64_t* cat_idx, float* out, float* alpha_out,
                               int B, int U, int H, int C1, int d, void* stream) {
    if (!Xu || !kq || !cat_idx || !out || !alpha_out) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    TopicArgs g{Xu, (long)U * d, kq, cat_idx, out, B, H, C1, d, sqrtf((float)d), alpha_out};
    return launch_topic_args(g, (hipStream_t)stream);
}
// the same launch, also zero-filling the topic rows of dXu (digat_user_ctx_bwd: one 34 MB memset launch per call less)
static int topic_pool_bwd_zero(const float* Xu, const float* kq, const int64_t* cat_idx, const float* alpha, const float* dT,
                               float* dXu, float* dkq, int B, int U, int H, int C1, int d, hipStream_t st) {
    if (H > TOPIC_MAX_H || d % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    TopicBwdArgs g{Xu, (long)U * d, kq, cat_idx, alpha, dT, dXu, (long)U * d, dkq, B, H, C1, d, sqrtf((float)d), U};
    hipLaunchKernelGGL(topic_pool_bwd_kernel, dim3(B), dim3(256), 0, st, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
int digat_topic_pool_bwd(const float* Xu, const float* kq, const int64_t* cat_idx, const float* alpha, const float* dT,
                         float* dXu, float* dkq, int B, int U, int H, int C1, int d, void* stream) {
    if (!Xu || !kq || !cat_idx || !alpha || !dT || !dXu || !dkq) return DIGAT_ERR_ARG;
    if (H > TOPIC_MAX_H || d % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    // dXu is [B,U,d]: history rows get the gradient, topic rows are untouched here (caller zero-fills)
    TopicBwdArgs g{Xu, (long)U * d, kq, cat_idx, alpha, dT, dXu, (long)U * d, dkq, B, H, C1, d, sqrtf((float)d), 0};
    hipLaunchKernelGGL(topic_pool_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, g);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// ---- Eq. 8 --------------------------------------------------------------------------------------------
// training forward of the pairwise part: like digat_xattn_pairwise_fwd but keeps what the backward needs:
// alpha [B,n,n] (before dropout), s_pre [B,n,n] (scores before leaky_relu/mask), and applies the attention
// dropout (amask [B,n,n] written; p = 0 -> no dropout, amask may be NULL).
// Which kernels run is eq8_train_fwd_route's decision (digat_xattn_plan.h), from the sizes and the caller's TrainEq8Opts; the choice
// is one of speed only: both sides compute the same function.
struct TrainEq8Opts {
    int* sparse_flag = nullptr;             // a device int of the caller's scratch.  Forward: with mode AUTO, graphs of more than 16 nodes take the
                                            // wave-per-centre kernel when a sample of the batch's adjacency is sparse (decided on the device: the
                                            // dense pair then returns at once, and vice versa).  Backward: the forward's choice, read there.
    int mode = DIGAT_TRAIN_XATTN_AUTO;      // _AUTO = that device-side choice; _SPARSE = the entry-wise kernels, _DENSE = the all-pairs kernels,
                                            // unguarded — a caller that knows its corpus (digat_amd: the encoder's corpus hint) saves the decision
                                            // launch and the launches that return at once.  A hint: see eq8_train_bwd_route
    float* dr = nullptr;                    // backward only: [B,d], the gradient of K3 (the node sums of dP')
};
static int xattn_pairwise_fwd_train_flag(const float* Pr, const float* Q, const float* h, const float* X, const float* a,
                                        const uint8_t* A, float* out, float* alpha, float* s_pre, float* alpha_drop,
                                        uint8_t* amask, float p, uint32_t seed, int B, int n, int d, void* stream,
                                        const TrainEq8Opts& o = TrainEq8Opts()) {
    if (!Pr || !Q || !h || !X || !a || !A || !out || !alpha || !s_pre) return DIGAT_ERR_ARG;
    if (p > 0.f && (!alpha_drop || !amask)) return DIGAT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    Eq8TrainIn in = {};
    in.B = B; in.n = n; in.d = d; in.mode = o.mode; in.flag = o.sparse_flag != nullptr;
    const Eq8TrainFwdRoute r = eq8_train_fwd_route(in);
    if (r.status || r.path == EQ8_TRAIN_NOTHING) return r.status;
    const bool small = r.path == EQ8_TRAIN_SMALL, guarded = r.path == EQ8_TRAIN_GUARDED;
    if (guarded) {
        hipLaunchKernelGGL(train_sparse_decide_kernel, dim3(1), dim3(1024), 0, st, A, B, n, SPARSE_PER_NODE, o.sparse_flag);
        DIGAT_CHECK_LAUNCH();
    }
    if (r.sparse.kernel != EQ8_NONE) {
        // round 6: the user graph's forward on the sparse kernel (a wave per centre walks its ~9 adjacency entries: score, softmax,
        // dropout and aggregation from registers; the tile kernel + aggregation pair visits all n^2 pairs)
        SparseArgs g = sparse_args(Pr, Q, h, X, a, A, out, B, n, d / 4);
        if (guarded) g.run_if = o.sparse_flag;
        g.xcd_group = r.sparse.xcd_group;
        g.t_alpha = alpha; g.t_spre = s_pre; g.t_amask = p > 0.f ? amask : nullptr; g.t_p = p; g.t_seed = seed;
        launch_sparse_kernel(r.sparse, g, st);
        DIGAT_CHECK_LAUNCH();
        if (!guarded) return DIGAT_OK;      // the caller knows the corpus is sparse: the entry-wise kernel alone
    }
    ScoreArgs g = score_args(r.tile);
    g.P = Pr; g.Q = Q; g.a = a; g.A = A; g.alpha = alpha; g.s_out = s_pre;
    // the attention dropout happens where alpha is produced (round 6: one dropout launch per layer and graph less); graphs of at
    // most 16 nodes (the news graph) are also aggregated there, from registers (no aggregation launch, no dropped copy of alpha)
    if (p > 0.f) { g.amask = amask; g.adrop = small ? nullptr : alpha_drop; g.drop_p = p; g.drop_seed = seed; }
    if (small) { g.agg_h = h; g.agg_x = X; g.agg_out = out; }
    if (guarded) g.skip_if = o.sparse_flag;
    const int rc = launch_score(r.score, g, st);
    if (rc || small) return rc;
    AggArgs ag = agg_args(p > 0.f ? alpha_drop : alpha, h, X, out, B, n, d);
    if (guarded) ag.skip_if = o.sparse_flag;
    return launch_agg(ag, r.agg, st);
}
int digat_xattn_pairwise_fwd_train(const float* Pr, const float* Q, const float* h, const float* X, const float* a,
                                   const uint8_t* A, float* out, float* alpha, float* s_pre, float* alpha_drop,
                                   uint8_t* amask, float p, uint32_t seed, int B, int n, int d, void* stream) {
    return xattn_pairwise_fwd_train_flag(Pr, Q, h, X, a, A, out, alpha, s_pre, alpha_drop, amask, p, seed, B, n, d, stream);
}

// the pairwise backward's scratch.  All-pairs launches: dZ [B,n,d], ds [B,n,n], the rows' da partials [B,d] and their group sums;
// entry-wise kernels: the (alpha', ds) pairs [B,n,n], a row of da per workgroup and the group sums of those rows
static long spb_blocks(int B, int n) { return ((long)B * n + 3) / 4; }
struct PairBwdWs { float *dZ, *ds, *dap, *dag; float2* wds; float *dap2, *dag2; };
static PairBwdWs pair_bwd_carve(Arena& w, int B, int n, int d) {
    const size_t nn = (size_t)B * n * n;
    const long nblk = spb_blocks(B, n);
    PairBwdWs o;
    o.dZ = w.take<float>((size_t)B * n * d); o.ds = w.take<float>(nn);
    o.dap = w.take<float>((size_t)B * d); o.dag = w.take<float>(colsum2_scratch(B, d));
    o.wds = w.take<float2>(nn);
    o.dap2 = w.take<float>((size_t)nblk * d); o.dag2 = w.take<float>(colsum2_scratch((int)nblk, d));
    return o;
}
size_t digat_xattn_pairwise_bwd_workspace(int B, int n, int d) { Arena a; pair_bwd_carve(a, B, n, d); return a.used; }
// given dOut [B,n,d]: dPr, dQ, dh [B,n,d], da [d] (accumulated if accumulate_da), dXres [B,n,d] = dOut (caller adds)
// ldg: row stride of the three gradient outputs (d, or 3 d when they are the column blocks of one [dh | dP' | dQ] matrix)
static int xattn_pairwise_bwd_ld(const float* dOut, const float* out, const float* Xres, const float* Pr, const float* Q,
                                 const float* h, const float* a, const uint8_t* A, const float* alpha, const float* s_pre,
                                 const uint8_t* amask, float p, float* dPr, float* dQ, float* dh, long ldg, float* da, int accumulate_da,
                                 int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream,
                                 const TrainEq8Opts& opts = TrainEq8Opts()) {
    if (!dOut || !out || !Xres || !Pr || !Q || !h || !a || !A || !alpha || !s_pre || !dPr || !dQ || !dh || !da || !workspace)
        return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    Arena w(workspace, workspace_bytes);
    const PairBwdWs o = pair_bwd_carve(w, B, n, d);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const float ascale = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const uint8_t* am = p > 0.f ? amask : nullptr;
    // the forward's choice (a device int in its save buffer): the entry-wise pair below when the batch's adjacency is sparse, the three
    // all-pairs launches otherwise — the launches of the other side return at once (eq8_train_bwd_route: which sides are launched)
    float* const dr = opts.dr;
    Eq8TrainIn in = {};
    in.B = B; in.n = n; in.d = d; in.mode = opts.mode; in.flag = opts.sparse_flag != nullptr; in.dr = dr != nullptr;
    const Eq8TrainBwdRoute r = eq8_train_bwd_route(in);
    const bool only_sparse = r.only_sparse;
    const int* guard = r.guard ? opts.sparse_flag : nullptr;
    const int nblk = (int)spb_blocks(B, n);
    if (r.sparse.kernel != EQ8_NONE) {
        SpBwdArgs t{dOut, out, Xres, h, Pr, Q, a, A, alpha, s_pre, am, ascale, o.dZ, o.wds, dQ, dh, dPr, ldg, o.dap2, B, n, d / 4, guard};
        eq8_by_width<2>(r.sparse.U, [&](auto u) {
            constexpr int U = decltype(u)::value;
            hipLaunchKernelGGL(xattn_sparse_bwd_centre_kernel<U>, dim3(r.sparse.grid), dim3(r.sparse.block), 0, st, t);
            hipLaunchKernelGGL(xattn_sparse_bwd_node_kernel<U>, dim3(r.sparse.grid), dim3(r.sparse.block), 0, st, t);
        });
        DIGAT_CHECK_LAUNCH();
    }
    if (only_sparse) {
        hipLaunchKernelGGL(sum_nodes_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, st, (const float*)dPr, dr, B, n, d, ldg);
        DIGAT_CHECK_LAUNCH();
        return launch_colsum2(o.dap2, d, da, nblk, d, accumulate_da, o.dag2, st);
    }
    // ds — and dZ = dOut [out - Xres > 0] on its way in (written for the two launches below)
    int rc = launch_ds(DsArgs{o.dZ, h, alpha, s_pre, A, am, ascale, o.ds, B, n, d, dOut, out, Xres, o.dZ, guard}, st);
    if (rc) return rc;
    rc = launch_aggT(AggTArgs{alpha, am, ascale, o.dZ, dh, B, n, d, ldg, guard}, st);                // dh = alpha'^T dZ
    if (rc) return rc;
    {   // dP', dQ, da partials
        PairBwdArgs t{Pr, Q, a, o.ds, dPr, dQ, o.dap, B, n, d, ldg, dr, guard};
        const Eq8Launch& l = r.pair;
        auto kern = l.ch == 64 ? xattn_pair_bwd_kernel<64> : xattn_pair_bwd_kernel<32>;
        if (l.raise_lds && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, dim3(l.grid, l.grid_y), dim3(l.block), l.lds, st, t);
        DIGAT_CHECK_LAUNCH();
    }
    if (guard) {
        // entry-wise side: da over the centre kernel's workgroup rows (guarded: nothing when the all-pairs side ran), K3's gradient
        // over the nodes of dP' (valid on both sides; the all-pairs kernel wrote the same sums already)
        hipLaunchKernelGGL(sum_nodes_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, st, (const float*)dPr, dr, B, n, d, ldg);
        DIGAT_CHECK_LAUNCH();
        rc = launch_colsum2_if(o.dap2, d, da, nblk, d, accumulate_da, o.dag2, st, guard, 1);
        if (rc) return rc;
        return launch_colsum2_if(o.dap, d, da, B, d, accumulate_da, o.dag, st, guard, 0);
    }
    return launch_colsum2(o.dap, d, da, B, d, accumulate_da, o.dag, st);
}
int digat_xattn_pairwise_bwd(const float* dOut, const float* out, const float* Xres, const float* Pr, const float* Q,
                             const float* h, const float* a, const uint8_t* A, const float* alpha, const float* s_pre,
                             const uint8_t* amask, float p, float* dPr, float* dQ, float* dh, float* da, int accumulate_da,
                             int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream) {
    return xattn_pairwise_bwd_ld(dOut, out, Xres, Pr, Q, h, a, A, alpha, s_pre, amask, p, dPr, dQ, dh, (long)d, da, accumulate_da, B, n, d,
                                 workspace, workspace_bytes, stream);
}

int digat_sum_nodes(const float* dP, float* dr, int B, int n, int d, void* stream) {
    if (!dP || !dr) return DIGAT_ERR_ARG;
    if (B == 0) return DIGAT_OK;
    hipLaunchKernelGGL(sum_nodes_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, (hipStream_t)stream, dP, dr, B, n, d, (long)d);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// the fused Eq. 8 projection for training: [h | P' | Q] = X [W | F1 | F2]^T (+bW on h, +r on P'), fp32 MFMA
int digat_xattn_project(const float* X, const float* r, const float* W, const float* bW, const float* F1, const float* F2,
                        float* h, float* Pr, float* Q, int B, int n, int d, void* stream) {
    if (!X || !r || !W || !F1 || !F2 || !h || !Pr || !Q) return DIGAT_ERR_ARG;
    if (d % 4) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    GemmArgs g = proj3_args(X, B * n, d, W, bW, F1, F2, h, Pr, Q, nullptr, 0, 0, nullptr);
    g.radd = r; g.radd_seg = 1; g.rows_per_b = n;
    return launch_gemm(g, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}
// the same with the bf16x6 kernel: [W|F1|F2] is split into `wsplit` (digat_split_weights_bytes(3 d, d) bytes) first
int digat_xattn_project_x3(const float* X, const float* r, const float* W, const float* bW, const float* F1, const float* F2,
                           float* h, float* Pr, float* Q, int B, int n, int d, void* wsplit, void* stream) {
    if (!X || !r || !W || !F1 || !F2 || !h || !Pr || !Q || !wsplit) return DIGAT_ERR_ARG;
    if (d % 80 || (long)B * n < 2048) return DIGAT_ERR_SHAPE;
    int rc = launch_split(W, F1, F2, d, 3, d, wsplit, (hipStream_t)stream, 0, 0);
    if (rc) return rc;
    GemmArgs g = proj3_args(X, B * n, d, W, bW, F1, F2, h, Pr, Q, wsplit, 0, DIGAT_GEMM_BF16X6, nullptr);
    if (g_train_bf16) g.x1_segs = 7;           // digat_set_train_precision(1): one bf16 product
    g.radd = r; g.radd_seg = 1; g.rows_per_b = n;
    return launch_gemm(g, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}

}  // extern "C"
