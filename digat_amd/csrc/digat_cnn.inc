// digat_cnn.inc — CNN news encoder, inference and training (reference: newsEncoders.py:29-54, layers.py:7-47 Conv1D,
// layers.py:91-115 Attention).  Three stages, the last one owned by the MSA encoder's files and called from here:
//   A. x = dropout_1(embedding[tokens])                                           [T, Lw, dm]     (never stored)
//   B. h = dropout_2(relu(conv1d(x) + b)), zero padding of p = (taps-1)/2 positions at both ends OF EACH TITLE    [T, Lw, Kc]
//   C. additive attention pooling: news_pool_fwd (digat_news.inc) / news_pool_bwd (digat_news_train.inc).
// The convolution is a GEMM with M = T Lw rows, N = Kc columns and K = taps x dm whose A operand is never materialised: row (t, j),
// tap s is x[t, j+s-p] inside the title and zero outside.  cnn_conv_tiled_kernel stages, per 32-deep slice of dm, the rows of a
// tile's titles ONCE in LDS with p zero halo rows around each title, already split into the three bf16 pieces of the bf16x6 format
// (digat_gemm.inc §1b), and the taps read that image at row offsets 0..taps-1 against taps sub-tiles of the split weight image: the
// gather and the operand split are paid once per slice, not once per tap.  The same kernel takes a DIRECT source (rows t Lw + j of an
// [M, ld] array): the input gradient is the same convolution of dz with the weights flipped in s and transposed in (c, i).
// `group3` (windows 1, 3, 5 on a third of the kernels each) is the 5-tap convolution whose weights are zero where a branch has no tap.
// Included by digat_kernels.hip after digat_news_train.inc.

struct CnnConvArgs {
    const float* src; long lds;            // tokens != NULL: the table [V, lds] (rows gathered);  NULL: rows t Lw + j of [M, lds]
    const int* tokens;
    const unsigned short* wimg;            // tiled kernel: the split weight image (cnn_split_kernel)
    const float* w; long sn, sk; int flip; // plain kernel: W(n, k, s) = w[n sn + k sk + (flip ? taps-1-s : s)]
    const float* bias; float* out; long ldo;
    int T, Lw, K, N, taps, relu;
    unsigned in_thr, in_seed; float in_scale;       // dropout on the source elements (flat index over [M, K]); thr = 0: none
    unsigned out_thr, out_seed; float out_scale;    // dropout in the epilogue (flat index over [M, N])
};

// ---- any shape: one thread per output element, fp32 fma chain -------------------------------------------------------------------
__global__ void __launch_bounds__(256) cnn_conv_plain_kernel(const CnnConvArgs g) {
    const long total = (long)g.T * g.Lw * g.N;
    const int p = (g.taps - 1) / 2;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / g.N;
        const int n = (int)(e - row * g.N), j = (int)(row % g.Lw);
        float acc = g.bias ? g.bias[n] : 0.f;
        for (int s = 0; s < g.taps; ++s) {
            const int jj = j + s - p;
            if (jj < 0 || jj >= g.Lw) continue;                       // the title's zero padding
            const long r2 = row + (s - p);
            const float* x = g.src + (g.tokens ? (long)g.tokens[r2] : r2) * g.lds;
            const float* w = g.w + (long)n * g.sn + (g.flip ? g.taps - 1 - s : s);
            for (int k = 0; k < g.K; ++k) {
                float v = x[k];
                if (g.in_thr) v = drop_keep(g.in_seed, r2 * g.K + k, g.in_thr) ? v * g.in_scale : 0.f;
                acc = fmaf(v, w[(long)k * g.sk], acc);
            }
        }
        if (g.relu) acc = fmaxf(acc, 0.f);
        if (g.out_thr) acc = drop_keep(g.out_seed, e, g.out_thr) ? acc * g.out_scale : 0.f;
        g.out[row * g.ldo + n] = acc;
    }
}

// ---- the matrix-core kernel ---------------------------------------------------------------------------------------------------
// Tile: CNN_BM rows (a whole number of titles: tpt = CNN_BM / Lw of them, tpt Lw rows used) x CNN_BN columns, four waves as 2 x 2,
// wave tile 64 x 64 = 4 x 4 blocks of v_mfma_f32_16x16x32_bf16 with the weights as the row operand (a lane ends with four consecutive
// output columns of one row: float4 epilogue).  A step is one (32-deep slice kc of K, tap s): 96 MFMAs per wave (16 blocks x six
// products).  The weight image holds one ready-made [piece][128 columns][32 k] block per (column tile, step), zero where n >= N or
// k >= K (K is padded to the slice in the image: no tail path), so a step's block is one contiguous 24 KB copy.  Both operands
// of the next step travel global -> registers under the current step's MFMAs and registers -> LDS between two barriers.
// LDS rows are 80 bytes apart (64 of data): the 16-byte fragment reads of eight consecutive rows start at banks 0, 20, 40, 60, 16, 36,
// 56, 12 and do not collide (a 64-byte stride would put every other row on the same banks).  Bank conflicts were not measured.
constexpr int CNN_BM = 128, CNN_BN = 128, CNN_BK = 32, CNN_ROWB = 80;
constexpr int CNN_MAX_AROWS = CNN_BM + 6 * (CNN_BM / 16);             // Lw >= 16, p <= 3: at most 8 titles x 6 halo rows
constexpr int CNN_BPIECE = CNN_BN * CNN_ROWB;                         // bytes of one piece of the weight block in LDS
constexpr int CNN_BLOCK_U4 = 3 * CNN_BN * CNN_BK * 2 / 16;            // 16-byte words of one weight block (1536)
constexpr int CNN_AU = (CNN_MAX_AROWS * (CNN_BK / 4) + 255) / 256;    // float4 of the A slice per thread

static bool cnn_tiled_ok(long M, int Lw, int K, int N, int taps) {
    return M >= 2048 && Lw >= 16 && Lw <= 64 && K % 4 == 0 && K >= 32 && N % 4 == 0 && taps >= 1 && taps <= 7 && (taps & 1);
}
static int cnn_arows(int Lw, int taps) { return (CNN_BM / Lw) * (Lw + taps - 1); }
static size_t cnn_tiled_lds(int Lw, int taps) {
    return (size_t)3 * cnn_arows(Lw, taps) * CNN_ROWB + 3 * CNN_BPIECE + (size_t)2 * cnn_arows(Lw, taps) * 4;
}
static size_t cnn_image_bytes(int K, int N, int taps) {
    return (size_t)((N + CNN_BN - 1) / CNN_BN) * ((K + CNN_BK - 1) / CNN_BK) * taps * CNN_BLOCK_U4 * 16;
}

struct CnnSplitArgs { const float* w; long sn, sk; int flip, N, K, taps; unsigned short* img; };
__global__ void __launch_bounds__(256) cnn_split_kernel(const CnnSplitArgs g) {
    const int nch = (g.K + CNN_BK - 1) / CNN_BK, ntn = (g.N + CNN_BN - 1) / CNN_BN;
    const long total = (long)ntn * nch * g.taps * CNN_BN * CNN_BK;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int k = (int)(e & (CNN_BK - 1)), n = (int)((e >> 5) & (CNN_BN - 1));
        const long blk = e >> 12;
        const int step = (int)(blk % ((long)nch * g.taps)), nt = (int)(blk / ((long)nch * g.taps));
        const int kc = step / g.taps, s = step - kc * g.taps;
        const int ng = nt * CNN_BN + n, kg = kc * CNN_BK + k;
        const float v = (ng < g.N && kg < g.K) ? g.w[(long)ng * g.sn + (long)kg * g.sk + (g.flip ? g.taps - 1 - s : s)] : 0.f;
        const Split3 sp = split3(v);
        unsigned short* o = g.img + blk * (3 * CNN_BN * CNN_BK) + n * CNN_BK + k;
        o[0] = sp.a; o[CNN_BN * CNN_BK] = sp.b; o[2 * CNN_BN * CNN_BK] = sp.c;
    }
}

__global__ void __launch_bounds__(256, 2) cnn_conv_tiled_kernel(const CnnConvArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lq = lane >> 4;
    const int Lw = g.Lw, taps = g.taps, p = (taps - 1) >> 1, Lp = Lw + 2 * p;
    const int tpt = CNN_BM / Lw, tile_rows = tpt * Lw, arows = tpt * Lp;
    const int ntn = (g.N + CNN_BN - 1) / CNN_BN;
    const int nt = blockIdx.x % ntn;
    const long mt = blockIdx.x / ntn;
    const long M = (long)g.T * Lw;
    const int nch = (g.K + CNN_BK - 1) / CNN_BK, nsteps = nch * taps;
    const int apiece = arows * CNN_ROWB;
    unsigned char* As = smem;
    unsigned char* Bs = smem + 3 * apiece;
    int* srcrow = reinterpret_cast<int*>(Bs + 3 * CNN_BPIECE);         // per image row: the source row (token / global row), -1 = zeros
    int* growrow = srcrow + arows;                                     // ... and its global row t Lw + j (the dropout's element index)

    for (int ar = tid; ar < arows; ar += 256) {
        const int kt = ar / Lp, j = ar - kt * Lp - p;
        const long t = mt * tpt + kt;
        const bool ok = j >= 0 && j < Lw && t < g.T;
        const long grow = ok ? t * Lw + j : 0;
        srcrow[ar] = ok ? (g.tokens ? g.tokens[grow] : (int)grow) : -1;
        growrow[ar] = (int)grow;
    }
    __syncthreads();

    // the next step's operands wait in NAMED registers (indexed arrays of them stayed in scratch memory)
    typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
    static_assert(CNN_BLOCK_U4 == 6 * 256, "CNN_A_EACH lists the B prefetch registers too");
    static_assert(CNN_AU == 6, "CNN_A_EACH lists the A prefetch registers");
#define CNN_A_EACH(F) F(0) F(1) F(2) F(3) F(4) F(5)
#define CNN_A_DECL(u) v4f areg##u; v4u_ breg##u;
    CNN_A_EACH(CNN_A_DECL)
    auto load_a1 = [&](int kc, int u) __attribute__((always_inline)) -> v4f {
        const int idx = tid + 256 * u, row = idx >> 3, col = kc * CNN_BK + (idx & 7) * 4;
        float4 v = f4_zero();
        if (row < arows) {
            const int sr = srcrow[row];
            if (sr >= 0 && col < g.K) {
                v = *reinterpret_cast<const float4*>(g.src + (long)sr * g.lds + col);
                if (g.in_thr) {
                    const long e = (long)growrow[row] * g.K + col;
                    v.x = drop_keep(g.in_seed, e, g.in_thr) ? v.x * g.in_scale : 0.f;
                    v.y = drop_keep(g.in_seed, e + 1, g.in_thr) ? v.y * g.in_scale : 0.f;
                    v.z = drop_keep(g.in_seed, e + 2, g.in_thr) ? v.z * g.in_scale : 0.f;
                    v.w = drop_keep(g.in_seed, e + 3, g.in_thr) ? v.w * g.in_scale : 0.f;
                }
            }
        }
        return (v4f){v.x, v.y, v.z, v.w};
    };
    auto store_a1 = [&](int u, const v4f r) __attribute__((always_inline)) {
        const int idx = tid + 256 * u, row = idx >> 3;
        if (row < arows) {
            const Split3f a = split3f(r[0]), b = split3f(r[1]), c = split3f(r[2]), d = split3f(r[3]);
            unsigned char* o = As + row * CNN_ROWB + (idx & 7) * 8;
            *reinterpret_cast<uint2*>(o) = make_uint2(pack_hi16(a.a, b.a), pack_hi16(c.a, d.a));
            *reinterpret_cast<uint2*>(o + apiece) = make_uint2(pack_hi16(a.b, b.b), pack_hi16(c.b, d.b));
            *reinterpret_cast<uint2*>(o + 2 * apiece) = make_uint2(pack_hi16(a.c, b.c), pack_hi16(c.c, d.c));
        }
    };
#define CNN_A_LOAD(u) areg##u = load_a1(kc_next, u);
#define CNN_A_STORE(u) store_a1(u, areg##u);
    const uint4* img = reinterpret_cast<const uint4*>(g.wimg) + (long)nt * nsteps * CNN_BLOCK_U4;
    auto store_b1 = [&](int u, const v4u_ r) __attribute__((always_inline)) {
        const int i = tid + 256 * u, pc = i >> 9, n = (i & 511) >> 2, kq = i & 3;
        *reinterpret_cast<v4u_*>(Bs + pc * CNN_BPIECE + n * CNN_ROWB + kq * 16) = r;
    };
#define CNN_B_LOAD(u) breg##u = reinterpret_cast<const v4u_*>(img)[(long)step_next * CNN_BLOCK_U4 + tid + 256 * u];
#define CNN_B_STORE(u) store_b1(u, breg##u);

    typedef int v4i_ __attribute__((ext_vector_type(4)));
    v4i_ arow;                                    // image row of this lane's output row in each 16-row block, tap 0
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int r = wm * 64 + mb * 16 + lr;
        arow[mb] = r < tile_rows ? r + 2 * p * (r / Lw) : 0;
    }
    v4f acc[4][4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = (v4f){0.f, 0.f, 0.f, 0.f};

    { const int kc_next = 0; CNN_A_EACH(CNN_A_LOAD) }
    { const int step_next = 0; CNN_A_EACH(CNN_B_LOAD) }
    int kc = 0, s = 0;
    for (int step = 0; step < nsteps; ++step) {
        __syncthreads();                          // every wave has finished the previous step's reads
        if (s == 0) { CNN_A_EACH(CNN_A_STORE) }
        CNN_A_EACH(CNN_B_STORE)
        __syncthreads();
        if (s == 0 && kc + 1 < nch) { const int kc_next = kc + 1; CNN_A_EACH(CNN_A_LOAD) }
        if (step + 1 < nsteps) { const int step_next = step + 1; CNN_A_EACH(CNN_B_LOAD) }
        bf16x8 wf[3][4];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
                wf[pc][nb] = *reinterpret_cast<const bf16x8*>(Bs + pc * CNN_BPIECE + (wn * 64 + nb * 16 + lr) * CNN_ROWB + lq * 16);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const unsigned char* ab = As + (arow[mb] + s) * CNN_ROWB + lq * 16;
            const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(ab), x2 = *reinterpret_cast<const bf16x8*>(ab + apiece),
                         x3 = *reinterpret_cast<const bf16x8*>(ab + 2 * apiece);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                v4f c = acc[mb][nb];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[2][nb], x1, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][nb], x2, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][nb], x3, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][nb], x1, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][nb], x2, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][nb], x1, c, 0, 0, 0);
                acc[mb][nb] = c;
            }
        }
        if (++s == taps) { s = 0; ++kc; }
    }

#undef CNN_A_EACH
#undef CNN_A_DECL
#undef CNN_A_LOAD
#undef CNN_A_STORE
#undef CNN_B_LOAD
#undef CNN_B_STORE
    // epilogue: lane (lr, lq) of block (mb, nb) holds out[row 16 mb + lr][columns 16 nb + 4 lq .. + 3]
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int r = wm * 64 + mb * 16 + lr;
        const long grow = mt * tile_rows + r;
        if (r >= tile_rows || grow >= M) continue;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int n0 = nt * CNN_BN + wn * 64 + nb * 16 + 4 * lq;
            if (n0 >= g.N) continue;                                   // N % 4 == 0: all four columns or none
            v4f v = acc[mb][nb];
            if (g.bias) {
                const float4 b = *reinterpret_cast<const float4*>(g.bias + n0);
                v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (g.relu) v[q] = fmaxf(v[q], 0.f);
                if (g.out_thr) v[q] = drop_keep(g.out_seed, grow * g.N + n0 + q, g.out_thr) ? v[q] * g.out_scale : 0.f;
            }
            *reinterpret_cast<float4*>(g.out + grow * g.ldo + n0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
static int cnn_launch_split(const float* w, long sn, long sk, int flip, int N, int K, int taps, void* img, hipStream_t st) {
    CnnSplitArgs a{w, sn, sk, flip, N, K, taps, (unsigned short*)img};
    const long total = (long)(cnn_image_bytes(K, N, taps) / 6);
    hipLaunchKernelGGL(cnn_split_kernel, dim3(grid_for(total)), dim3(256), 0, st, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
// a.wimg != NULL and the shape on the tile rules: the matrix-core kernel; otherwise the plain one (a.w must be set)
static int cnn_launch_conv(const CnnConvArgs& a, hipStream_t st) {
    const long M = (long)a.T * a.Lw;
    if (M == 0) return DIGAT_OK;
    ProfScope prof(DIGAT_KERNEL_LINEAR, 2.0 * M * (double)a.N * a.K * a.taps, st, 4.0 * ((double)M * (a.K + a.N) + (double)a.N * a.K * a.taps));
    if (a.wimg && cnn_tiled_ok(M, a.Lw, a.K, a.N, a.taps) && a.lds % 4 == 0 && a.ldo % 4 == 0) {
        const size_t lds = cnn_tiled_lds(a.Lw, a.taps);
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)cnn_conv_tiled_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess) return DIGAT_ERR_LAUNCH;
        const int tpt = CNN_BM / a.Lw;
        const long tiles = ((long)a.T + tpt - 1) / tpt * ((a.N + CNN_BN - 1) / CNN_BN);
        if (tiles > 0x7fffffffL) return DIGAT_ERR_SHAPE;
        hipLaunchKernelGGL(cnn_conv_tiled_kernel, dim3((unsigned)tiles), dim3(256), lds, st, a);
    } else {
        if (!a.w) return DIGAT_ERR_ARG;
        hipLaunchKernelGGL(cnn_conv_plain_kernel, dim3(grid_for(M * a.N)), dim3(256), 0, st, a);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// ---- training helpers --------------------------------------------------------------------------------------------------------
// dz = dh . [h > 0] / (1 - p_2) (h is stored AFTER the second dropout: h > 0 exactly where the unit was kept and its ReLU open), in
// place, and its copy with p zero halo rows around each title ([T, Lw + 2p, Kc]); x = dropout_1(embedding[tokens]) with the same halo
// ([T, Lw + 2p, dm]), its keep bits REGENERATED from the counter hash.  With the halos a flat row shift of s - p is exact: the weight
// gradient of tap s is one TN product of the two padded arrays.
struct CnnPadArgs { const float* h; float* dh; float* dzpad; const float* table; const int* tokens; float* xpad;
                    int T, Lw, p, Kc, dm; float scale2; unsigned thr1, seed1; float scale1; };
__global__ void __launch_bounds__(256) cnn_pad_kernel(const CnnPadArgs g) {
    const int Lp = g.Lw + 2 * g.p, k4 = g.Kc >> 2, d4 = g.dm >> 2, per = k4 + d4;
    const long total = (long)g.T * Lp * per;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long prow = e / per;
        const int c = (int)(e - prow * per);
        const long t = prow / Lp;
        const int j = (int)(prow - t * Lp) - g.p;
        const bool in = j >= 0 && j < g.Lw;
        const long row = t * g.Lw + j;
        float4 v = f4_zero();
        if (c < k4) {
            if (in) {
                const float4 hv = reinterpret_cast<const float4*>(g.h + row * g.Kc)[c];
                float4* dp = reinterpret_cast<float4*>(g.dh + row * g.Kc) + c;
                const float4 d = *dp;
                v = make_float4(hv.x > 0.f ? d.x * g.scale2 : 0.f, hv.y > 0.f ? d.y * g.scale2 : 0.f, hv.z > 0.f ? d.z * g.scale2 : 0.f,
                                hv.w > 0.f ? d.w * g.scale2 : 0.f);
                *dp = v;
            }
            reinterpret_cast<float4*>(g.dzpad + prow * g.Kc)[c] = v;
        } else {
            const int q = c - k4;
            if (in) {
                v = reinterpret_cast<const float4*>(g.table + (long)g.tokens[row] * g.dm)[q];
                if (g.thr1) {
                    const long el = row * g.dm + 4 * q;
                    v.x = drop_keep(g.seed1, el, g.thr1) ? v.x * g.scale1 : 0.f;
                    v.y = drop_keep(g.seed1, el + 1, g.thr1) ? v.y * g.scale1 : 0.f;
                    v.z = drop_keep(g.seed1, el + 2, g.thr1) ? v.z * g.scale1 : 0.f;
                    v.w = drop_keep(g.seed1, el + 3, g.thr1) ? v.w * g.scale1 : 0.f;
                }
            }
            reinterpret_cast<float4*>(g.xpad + prow * g.dm)[q] = v;
        }
    }
}
// [taps][Kc][dm] (one TN product per tap) -> torch's Conv1d layout [Kc][dm][taps]
__global__ void __launch_bounds__(256) cnn_taps_last_kernel(const float* in, float* out, long per, int taps) {
    const long total = per * taps;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long ci = e / taps;
        out[e] = in[(e - ci * taps) * per + ci];
    }
}
// the zero-filled 5-tap form of group3 (layers.py:16-19): kernels [0, K3) window 1 (tap 2), [K3, 2 K3) window 3 (taps 1..3), the rest window 5
struct CnnMergeArgs { const float *W1, *W2, *W3, *b1, *b2, *b3; float* W; float* b; int K3, dm; };
__global__ void __launch_bounds__(256) cnn_merge_group3_kernel(const CnnMergeArgs g) {
    const long nw = (long)3 * g.K3 * g.dm * 5, total = nw + 3 * g.K3;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e >= nw) {
            const int c = (int)(e - nw), br = c / g.K3;
            g.b[c] = (br == 0 ? g.b1 : br == 1 ? g.b2 : g.b3)[c - br * g.K3];
            continue;
        }
        const int s = (int)(e % 5);
        const long ci = e / 5;
        const int i = (int)(ci % g.dm), c = (int)(ci / g.dm), br = c / g.K3, cl = c - br * g.K3;
        const int win = 2 * br + 1, off = 2 - br;
        const float* w = br == 0 ? g.W1 : br == 1 ? g.W2 : g.W3;
        g.W[e] = (s >= off && s < off + win) ? w[((long)cl * g.dm + i) * win + (s - off)] : 0.f;
    }
}

extern "C" {

size_t digat_cnn_split_bytes(int word_embedding_dim, int kernel_num, int taps) {
    if (word_embedding_dim <= 0 || kernel_num <= 0 || taps <= 0) return 0;
    return cnn_image_bytes(word_embedding_dim, kernel_num, taps);
}
// W [Kc][dm][taps] (torch's Conv1d layout; group3: the output of digat_cnn_merge_group3) -> the forward kernel's weight image
int digat_split_cnn_weights(const float* W, int word_embedding_dim, int kernel_num, int taps, void* w_split, void* stream) {
    if (!W || !w_split || word_embedding_dim <= 0 || kernel_num <= 0) return DIGAT_ERR_ARG;
    if (taps < 1 || taps > 7 || !(taps & 1)) return DIGAT_ERR_SHAPE;
    return cnn_launch_split(W, (long)word_embedding_dim * taps, taps, 0, kernel_num, word_embedding_dim, taps, w_split, (hipStream_t)stream);
}
int digat_cnn_merge_group3(const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                           int word_embedding_dim, int kernel_num, float* W, float* b, void* stream) {
    if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !W || !b || word_embedding_dim <= 0 || kernel_num <= 0) return DIGAT_ERR_ARG;
    if (kernel_num % 3) return DIGAT_ERR_SHAPE;
    CnnMergeArgs a{W1, W2, W3, b1, b2, b3, W, b, kernel_num / 3, word_embedding_dim};
    hipLaunchKernelGGL(cnn_merge_group3_kernel, dim3(grid_for((long)kernel_num * word_embedding_dim * 5 + kernel_num)), dim3(256), 0,
                       (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

static int cnn_shape_ok(const digat_cnn_params* p, int Lw, int max_Lw) {
    const int dm = p->word_embedding_dim, Kc = p->kernel_num, taps = p->taps, att = p->attention_dim;
    return dm > 0 && dm % 4 == 0 && Kc > 0 && Kc % 4 == 0 && taps >= 1 && taps <= 7 && (taps & 1) && att > 0 && Lw <= max_Lw;
}
static bool cnn_params_set(const digat_cnn_params* p) { return p->word_embedding && p->W && p->b && p->A1 && p->b1 && p->a2; }

struct CnnFwdWs { float *h, *pre; };
static size_t cnn_fwd_carve(Arena& w, int T, int Lw, int Kc, int att, CnnFwdWs* o) {
    const size_t M = (size_t)T * Lw;
    o->h = w.take<float>(M * Kc); o->pre = w.take<float>(M * msa_attp(att));
    return w.used;
}
size_t digat_cnn_workspace_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim) {
    (void)word_embedding_dim; (void)taps;
    if (T <= 0 || Lw <= 0 || kernel_num <= 0 || attention_dim <= 0) return 0;
    Arena measure;
    CnnFwdWs o;
    return cnn_fwd_carve(measure, T, Lw, kernel_num, attention_dim, &o);
}

int digat_cnn_fwd(const digat_cnn_params* p, const int32_t* title_text, const uint8_t* title_mask, float* out, int T, int Lw,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !title_text || !title_mask || !out || !workspace || T < 0 || Lw <= 0) return DIGAT_ERR_ARG;
    if (!cnn_params_set(p)) return DIGAT_ERR_ARG;
    if (!cnn_shape_ok(p, Lw, 64)) return DIGAT_ERR_SHAPE;
    const int dm = p->word_embedding_dim, Kc = p->kernel_num, taps = p->taps, att = p->attention_dim;
    Arena w(workspace, workspace_bytes);
    CnnFwdWs o;
    cnn_fwd_carve(w, T, Lw, Kc, att, &o);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    if (T == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    CnnConvArgs c{};
    c.src = p->word_embedding; c.lds = dm; c.tokens = title_text; c.wimg = (const unsigned short*)p->w_split;
    c.w = p->W; c.sn = (long)dm * taps; c.sk = taps; c.flip = 0; c.bias = p->b; c.out = o.h; c.ldo = Kc;
    c.T = T; c.Lw = Lw; c.K = dm; c.N = Kc; c.taps = taps; c.relu = 1;
    T_TRY(cnn_launch_conv(c, st));
    return news_pool_fwd(o.h, Kc, p->A1, p->a1_wsplit, p->b1, p->a2, o.pre, title_mask, out, nullptr, T, Lw, att, false, st);
}

// ---- the training pair ------------------------------------------------------------------------------------------------------
struct CnnSave { float *h, *pre, *alpha; };
static size_t cnn_save_carve(Arena& a, int T, int Lw, int Kc, int att, CnnSave* s) {
    const size_t M = (size_t)T * Lw;
    s->h = a.take<float>(M * Kc); s->pre = a.take<float>(M * msa_attp(att)); s->alpha = a.take<float>(M);
    return a.used;
}
size_t digat_cnn_train_save_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim) {
    (void)word_embedding_dim; (void)taps;
    if (T <= 0 || Lw <= 0 || kernel_num <= 0 || attention_dim <= 0) return 0;
    Arena measure;
    CnnSave s;
    return cnn_save_carve(measure, T, Lw, kernel_num, attention_dim, &s);
}
struct CnnTrainWs { void *w_img, *a1_img, *wt_img; PoolBwdWs pool; float *dzpad, *xpad, *dwt; void* wg; size_t wgb; };
static size_t cnn_train_carve(Arena& w, int T, int Lw, int dm, int Kc, int taps, int att, CnnTrainWs* o) {
    const size_t M = (size_t)T * Lw, Mp = (size_t)T * (Lw + taps - 1), attp = msa_attp(att);
    o->w_img = w.take<char>(cnn_image_bytes(dm, Kc, taps));
    o->a1_img = w.take<char>(digat_split_weights_bytes(att, Kc));
    o->pool.a1t_img = w.take<char>(digat_split_weights_bytes(Kc, att));
    o->wt_img = w.take<char>(cnn_image_bytes(Kc, dm, taps));
    o->pool.dh = w.take<float>(M * Kc);
    o->pool.dpre = w.take<float>(M * attp);
    o->pool.da2p = w.take<float>((size_t)T * att);
    o->pool.da2g = w.take<float>((size_t)((T + 63) / 64) * att);
    o->dzpad = w.take<float>(Mp * Kc);
    o->xpad = w.take<float>(Mp * dm);
    o->dwt = w.take<float>((size_t)taps * Kc * dm);
    o->wgb = 0;
    for (int d = 0; d <= (taps - 1) / 2; ++d) {                         // a tap shifted by d rows runs over Mp - d of them
        const size_t b = digat_linear_bwd_weight_workspace((int)Mp - d, Kc, dm);
        if (b > o->wgb) o->wgb = b;
    }
    const size_t wgb2 = digat_linear_bwd_weight_workspace((int)M, att, Kc);
    if (wgb2 > o->wgb) o->wgb = wgb2;
    o->wg = w.take<char>(o->wgb);
    return w.used;
}
size_t digat_cnn_train_workspace_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim) {
    if (T <= 0 || Lw <= 0 || word_embedding_dim <= 0 || kernel_num <= 0 || taps <= 0 || attention_dim <= 0) return 0;
    Arena measure;
    CnnTrainWs o;
    return cnn_train_carve(measure, T, Lw, word_embedding_dim, kernel_num, taps, attention_dim, &o);
}

// out [T, Kc].  p_drop: both dropouts of newsEncoders.py:46-48 — site 1 on the embedded tokens (keep bits: the counter hash of `seed`
// over the [T Lw, dm] elements), site 2 on relu(conv) (`seed + 1` over the [T Lw, Kc] elements).  `save` carries h (after the second
// dropout), the affine1 product and the pooling weights; the backward regenerates site 1's bits and reads site 2's off h.  params'
// *_split fields are not used (the weights change every optimiser step: they are split here, into the workspace).
int digat_cnn_fwd_train(const digat_cnn_params* p, const int32_t* title_text, const uint8_t* title_mask, float* out, float p_drop,
                        uint32_t seed, int T, int Lw, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !title_text || !title_mask || !out || !save || !workspace || T < 0 || Lw <= 0 || p_drop < 0.f || p_drop >= 1.f)
        return DIGAT_ERR_ARG;
    if (!cnn_params_set(p)) return DIGAT_ERR_ARG;
    if (!cnn_shape_ok(p, Lw, 32) || p->attention_dim % 4) return DIGAT_ERR_SHAPE;
    const int dm = p->word_embedding_dim, Kc = p->kernel_num, taps = p->taps, att = p->attention_dim;
    if (T == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    CnnSave s;
    CnnTrainWs o;
    cnn_save_carve(sa, T, Lw, Kc, att, &s);
    cnn_train_carve(w, T, Lw, dm, Kc, taps, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)T * Lw;
    CnnConvArgs c{};
    c.src = p->word_embedding; c.lds = dm; c.tokens = title_text;
    c.w = p->W; c.sn = (long)dm * taps; c.sk = taps; c.flip = 0; c.bias = p->b; c.out = s.h; c.ldo = Kc;
    c.T = T; c.Lw = Lw; c.K = dm; c.N = Kc; c.taps = taps; c.relu = 1;
    if (p_drop > 0.f) {
        c.in_thr = c.out_thr = drop_threshold(p_drop); c.in_seed = seed; c.out_seed = seed + 1u;
        c.in_scale = c.out_scale = 1.f / (1.f - p_drop);
    }
    if (cnn_tiled_ok(M, Lw, dm, Kc, taps)) {
        T_TRY(cnn_launch_split(p->W, (long)dm * taps, taps, 0, Kc, dm, taps, o.w_img, st));
        c.wimg = (const unsigned short*)o.w_img;
    }
    T_TRY(cnn_launch_conv(c, st));
    const void* a1_img = nullptr;
    if (M >= 2048 && Kc >= 32) {
        T_TRY(launch_split(p->A1, p->A1, p->A1, att, 1, Kc, o.a1_img, st));
        a1_img = o.a1_img;
    }
    // bf16_ok = false: affine1 stays fp32-grade under digat_set_train_precision(1) (digat_msa_fwd_train's follows it)
    return news_pool_fwd(s.h, Kc, p->A1, a1_img, p->b1, p->a2, s.pre, title_mask, out, s.alpha, T, Lw, att, false, st);
}

// dout [T, Kc].  Written (not accumulated): row_grad [T*Lw, dm], rows ld_row_grad >= dm floats apart (a multiple of 4) — the gradient
// at the embedded tokens after site 1's backward: feed it to digat_embedding_bwd; dW [Kc][dm][taps], db [Kc], dA1 [att, Kc], db1 da2 [att].
// p_drop and seed are the forward's.
int digat_cnn_bwd(const digat_cnn_params* p, const int32_t* title_text, const uint8_t* title_mask, const float* dout, float p_drop,
                  uint32_t seed, const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW, float* db, float* dA1,
                  float* db1, float* da2, int T, int Lw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !title_text || !title_mask || !dout || !save || !row_grad || !dW || !db || !dA1 || !db1 || !da2 || !workspace || T < 0 ||
        Lw <= 0 || p_drop < 0.f || p_drop >= 1.f) return DIGAT_ERR_ARG;
    if (!cnn_params_set(p)) return DIGAT_ERR_ARG;
    if (!cnn_shape_ok(p, Lw, 32) || p->attention_dim % 4) return DIGAT_ERR_SHAPE;
    const int dm = p->word_embedding_dim, Kc = p->kernel_num, taps = p->taps, att = p->attention_dim;
    const int pad = (taps - 1) / 2;
    if (ld_row_grad < dm || ld_row_grad % 4) return DIGAT_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t kn = Kc, an = att;
    if (T == 0) return zero_floats(st, {{dW, kn * dm * taps}, {db, kn}, {dA1, an * kn}, {db1, an}, {da2, an}});
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    CnnSave s;
    CnnTrainWs o;
    cnn_save_carve(sa, T, Lw, Kc, att, &s);
    cnn_train_carve(w, T, Lw, dm, Kc, taps, att, &o);
    if (!sa.ok || !w.ok) return DIGAT_ERR_WORKSPACE;
    const long M = (long)T * Lw, Mp = (long)T * (Lw + 2 * pad);
    T_TRY(news_pool_bwd(dout, s.h, Kc, s.pre, s.alpha, title_mask, p->A1, p->b1, p->a2, o.pool, o.wg, o.wgb, dA1, db1, da2, T, Lw, att, st));
    float* const dh = o.pool.dh;
    // second dropout + ReLU (dh becomes dz), and the halo-padded copies for the weight gradient
    {
        const float sc = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
        CnnPadArgs a{s.h, dh, o.dzpad, p->word_embedding, title_text, o.xpad, T, Lw, pad, Kc, dm, sc,
                     p_drop > 0.f ? drop_threshold(p_drop) : 0u, seed, sc};
        hipLaunchKernelGGL(cnn_pad_kernel, dim3(grid_for(Mp * ((Kc + dm) / 4))), dim3(256), 0, st, a);
        DIGAT_CHECK_LAUNCH();
    }
    // input gradient: the same convolution of dz with W flipped in s and transposed in (c, i); site 1's backward in its epilogue
    {
        CnnConvArgs c{};
        c.src = dh; c.lds = Kc; c.tokens = nullptr;
        c.w = p->W; c.sn = taps; c.sk = (long)dm * taps; c.flip = 1; c.bias = nullptr; c.out = row_grad; c.ldo = ld_row_grad;
        c.T = T; c.Lw = Lw; c.K = Kc; c.N = dm; c.taps = taps; c.relu = 0;
        if (p_drop > 0.f) { c.out_thr = drop_threshold(p_drop); c.out_seed = seed; c.out_scale = 1.f / (1.f - p_drop); }
        if (cnn_tiled_ok(M, Lw, Kc, dm, taps)) {
            T_TRY(cnn_launch_split(p->W, taps, (long)dm * taps, 1, dm, Kc, taps, o.wt_img, st));
            c.wimg = (const unsigned short*)o.wt_img;
        }
        T_TRY(cnn_launch_conv(c, st));
    }
    // weight gradient: tap s is dzpad^T xpad with xpad shifted by s - p rows (halo rows of dz are zero: no term crosses a title)
    for (int sI = 0; sI < taps; ++sI) {
        const int d = sI - pad;
        const float* dy = o.dzpad + (d < 0 ? (size_t)(-d) * Kc : 0);
        const float* x = o.xpad + (d > 0 ? (size_t)d * dm : 0);
        T_TRY(digat_linear_bwd_weight(dy, Kc, x, dm, o.dwt + (size_t)sI * Kc * dm, d == 0 ? db : nullptr, (int)(Mp - (d < 0 ? -d : d)), Kc, dm, 0,
                                      o.wg, o.wgb, st));
    }
    hipLaunchKernelGGL(cnn_taps_last_kernel, dim3(grid_for((long)Kc * dm * taps)), dim3(256), 0, st, (const float*)o.dwt, dW, (long)Kc * dm, taps);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
