// digat_qdot.inc — the quantised first stage: digat_dot_scores', digat_dot_topk's and digat_dot_shortlist's contracts on int8 codes with
// one fp32 scale per row, the product on v_mfma_i32_16x16x64_i8 (nrms.build_index, nrms.recommend(index=)).  Included at the end of
// digat_kernels.hip: the chunk walk and the selection (dot_chunk_walk with dot_append / dot_cut, dot_topk_user_kernel, topk_finish) are
// digat_dot_topk.inc's, the slab driver and the long selection (short_dot_slabs, shortlist_chunk_kernel, shortlist_segment_kernel) are
// digat_shortlist.inc's.  This file adds the quantiser and the 64 x 64 product tile, and no selection of its own.
//
// Codes.  digat_quantize_rows_i8, one wave per row of x [R, d]: amax = max |x|, scale = amax / 127.0f (an fp32 division, correctly
//   rounded), q[c] = clamp(rint(x[c] / scale), -127, 127) (fp32 division, round to nearest even), q[d .. dq) = 0 with dq = d rounded up
//   to 16: every row of codes is a whole number of 16-byte pieces.  scale == 0 (a zero row, or an amax that underflows) gives codes 0; a
//   row with a NaN or an infinity gives codes 0 and scale NaN: its scores are NaN and order last.  numpy float32 reproduces every step
//   (evaluate.quantize_rows_host).
// Scores.  score(g, p) = ((float)acc * su[g]) * sn[id], acc = the int32 sum over c of qu[g][c] * qn[id][c], id = pool[p] or p; an id
//   outside [0, N) is no element and its score is stored as +0.0.  d <= DIGAT_QDOT_MAX_D = 1024 keeps |acc| <= 127^2 * 1024 < 2^24: the
//   conversion is exact, and an integer sum has no order, so the bits are a function of the two code rows and the two scales alone —
//   whichever entry, tile, chunk or pool order computed them.  Two fp32 multiplications, left to right; there is nothing to contract.
// The tile, qdot_tile: dot_tile's wave layout (wave w owns users 32 (w / 2) .. + 32 and positions 32 (w % 2) .. + 32 as 2 x 2 MFMA tiles,
//   news = A, users = B, C/D row = position, column = user), K blocks of QDOT_KB = 128 codes staged in the bytes of DotShared's two fp32
//   operand tiles (64 rows of 128 + 16 bytes are exactly their 9 216 bytes), two k-steps of 64 per block, the next block's global loads
//   in flight under the MFMAs.  The lane map of the i8 operands inside a k-step is not relied on: lane (lr, lq) hands BOTH operands the
//   16 bytes at qdot_piece(ks, lq) of its row, so whatever k the hardware assigns to (lane group, byte), A and B agree on it, and the sum
//   over k is order-free.  Pieces at or beyond dq are zeros in both operands; k-steps wholly beyond dq are not issued.
//
// The error of a quantised score against the real product (evaluate.qdot_bound).  Write a row as x = s q + e.  rint puts |e_c| <= s / 2
//   (the clamp never bites beyond that: |x_c / s| <= 127 up to the rounding of the two divisions, which moves e_c by at most
//   127 * 2^-23 s — the factor (1 + 2^-15) below).  With u^ = su qu and v^ = sn qn, per channel
//       u v - u^ v^ = u (v - v^) + (u - u^) v^,   |v^| <= |v| + sn / 2,
//   so |<u, v> - su sn acc| <= sn/2 |u|_1 + su/2 |v|_1 + d su sn / 4.  The two fp32 multiplications add at most 2^-23 |su sn acc|
//   <= 2^-23 (|u|_2 |v|_2 + that bound).  Nothing else rounds.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup; the fused kernel adds
// dot_chunk_kernel<true>'s 512 (k + 64) bytes of dynamic LDS:
//   quantize_rows_kernel            VGPRs 17    SGPRs 26    LDS 0 B              scratch 0   occupancy 8 waves / SIMD
//   qdot_chunk_kernel<true>         VGPRs 126   SGPRs 106   LDS 43008 B static   scratch 0   occupancy 3 waves / SIMD (by static LDS)
//   qdot_chunk_kernel<false>        VGPRs 92    SGPRs 80    LDS 43008 B static   scratch 0   occupancy 3 waves / SIMD (by static LDS)
//   qdot_chunk_kernel<false, 256>   the lines of <false>: the slab's score launch of digat_qdot_shortlist
// dot_chunk_kernel<true>, <false>, <false, 256> and dot_topk_user_kernel keep the lines of their files from the same build.

#define QDOT_MAX_D DIGAT_QDOT_MAX_D
#define QDOT_KB 128                      // codes per staged K block: two k-steps of the 16x16x64 MFMA
#define QDOT_LD (QDOT_KB + 16)           // bytes per row of an operand tile: rows stay 16-byte aligned, 36 dwords apart as dot_tile's

typedef int qdot_v4i __attribute__((ext_vector_type(4)));
typedef qdot_v4i qdot_piece_t __attribute__((may_alias, aligned(16)));      // 16 codes, read and written in the bytes of fp32 tiles

static_assert(sizeof(((DotShared*)0)->Us) == DOT_USERS * QDOT_LD && sizeof(((DotShared*)0)->Ns) == DOT_SUB * QDOT_LD,
              "qdot_tile stages its code tiles in the bytes of DotShared's operand tiles");
static_assert(QDOT_MAX_D % QDOT_KB == 0 && 127 * 127 * QDOT_MAX_D < (1 << 24), "the int32 sum converts to fp32 exactly");

struct QdotArgs {
    DotArgs a;                   // users / news unused; the pool, the sizes, the skip rows, the workspace and the outputs
    const int8_t* qu;            // [G, dq]
    const int8_t* qn;            // [N, dq]
    const float* su;             // [G]
    const float* sn;             // [N]
    int dq;
};

__device__ __forceinline__ qdot_v4i qdot_load16(const int8_t* row, int k0, int dq) {
    // dq is a multiple of 16: a piece lies wholly inside the row or wholly beyond it
    return row && k0 < dq ? *(const qdot_piece_t*)(row + k0) : (qdot_v4i){0, 0, 0, 0};
}

// The one address function of both operands: the 16 bytes lane group lq contributes to k-step ks of a staged block.
__device__ __forceinline__ int qdot_piece(int ks, int lq) { return ks * 64 + lq * 16; }

// Ss[u][j] = score(u0 + u, position j of the sub-tile) for the 64 x 64 sub-tile (positions with id -1: +0.0; rows beyond G are never
// read back).  Called by the whole workgroup; ends behind a barrier.
__device__ __forceinline__ void qdot_tile(const QdotArgs& q, DotShared& s, long u0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int c16 = (tid & 7) * 16, r0 = tid >> 3;               // this thread stages rows r0 and r0 + 32, codes c16 .. c16 + 15
    char* Uq = (char*)s.Us;
    char* Nq = (char*)s.Ns;
    const int8_t* urow[2];
    const int8_t* nrow[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long g = u0 + r0 + 32 * h;
        const long long id = s.id[r0 + 32 * h];
        urow[h] = g < q.a.G ? q.qu + g * q.dq : nullptr;
        nrow[h] = id >= 0 ? q.qn + id * q.dq : nullptr;
    }
    const int ur = (wave >> 1) * 32, nc = (wave & 1) * 32;
    // the scales of this lane's outputs, asked for before the K loop: D[row = position nc + 16 tn + 4 lq + r][col = user ur + 16 tu + lr]
    float su[2], sn[2][4];
    bool elem[2][4];
#pragma unroll
    for (int tu = 0; tu < 2; ++tu) {
        const long g = u0 + ur + 16 * tu + lr;
        su[tu] = g < q.a.G ? q.su[g] : 0.f;
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long id = s.id[nc + 16 * tn + 4 * lq + r];
            elem[tn][r] = id >= 0;
            sn[tn][r] = id >= 0 ? q.sn[id] : 0.f;
        }
    qdot_v4i acc[2][2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tu = 0; tu < 2; ++tu) acc[tn][tu] = (qdot_v4i){0, 0, 0, 0};
    qdot_v4i ru[2], rn[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) { ru[h] = qdot_load16(urow[h], c16, q.dq); rn[h] = qdot_load16(nrow[h], c16, q.dq); }
    for (int kb = 0; kb < q.dq; kb += QDOT_KB) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(qdot_piece_t*)(Uq + (r0 + 32 * h) * QDOT_LD + c16) = ru[h];
            *(qdot_piece_t*)(Nq + (r0 + 32 * h) * QDOT_LD + c16) = rn[h];
        }
        __syncthreads();
        if (kb + QDOT_KB < q.dq) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ru[h] = qdot_load16(urow[h], kb + QDOT_KB + c16, q.dq);
                rn[h] = qdot_load16(nrow[h], kb + QDOT_KB + c16, q.dq);
            }
        }
#pragma unroll
        for (int ks = 0; ks < QDOT_KB / 64; ++ks) {
            if (kb + ks * 64 < q.dq) {                            // workgroup-uniform: no k-step wholly beyond dq
                const int k = qdot_piece(ks, lq);
                const qdot_v4i n0 = *(const qdot_piece_t*)(Nq + (nc + lr) * QDOT_LD + k);
                const qdot_v4i n1 = *(const qdot_piece_t*)(Nq + (nc + 16 + lr) * QDOT_LD + k);
                const qdot_v4i x0 = *(const qdot_piece_t*)(Uq + (ur + lr) * QDOT_LD + k);
                const qdot_v4i x1 = *(const qdot_piece_t*)(Uq + (ur + 16 + lr) * QDOT_LD + k);
                acc[0][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(n0, x0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(n0, x1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(n1, x0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(n1, x1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tu = 0; tu < 2; ++tu) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = elem[tn][r] ? ((float)acc[tn][tu][r] * su[tu]) * sn[tn][r] : 0.f;
            *(float4*)&s.Ss[ur + 16 * tu + lr][nc + 16 * tn + 4 * lq] = make_float4(v[0], v[1], v[2], v[3]);
        }
    __syncthreads();
}

template <bool FUSED, int CHUNK = DIGAT_DOT_TOPK_CHUNK>
__global__ void __launch_bounds__(256) qdot_chunk_kernel(const QdotArgs q) {
    __shared__ DotShared s;
    extern __shared__ uint2 dot_lists[];            // [DOT_USERS][k + DOT_SUB]
    dot_chunk_walk<FUSED, CHUNK>(q.a, s, dot_lists, [&](long u0) { qdot_tile(q, s, u0); });
}

// One wave per row, four rows per workgroup.
__global__ void __launch_bounds__(256) quantize_rows_kernel(const float* x, long R, int d, int dq, int8_t* q, float* scale) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;                           // a whole wave: the shuffles below stay among lanes of one row
    const float* xr = x + row * d;
    float amax = 0.f;
    bool bad = false;
    for (int c = lane; c < d; c += 64) {
        const float v = fabsf(xr[c]);
        bad = bad || !(v < INFINITY);               // a NaN or an infinity
        amax = fmaxf(amax, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    bad = __ballot(bad) != 0ull;
    const float sc = bad ? __uint_as_float(0x7fc00000u) : amax / 127.0f;
    const bool live = !bad && sc > 0.f;
    int8_t* qr = q + row * dq;
    for (int c = lane; c < dq; c += 64) {
        float r = 0.f;
        if (live && c < d) r = fminf(fmaxf(rintf(xr[c] / sc), -127.f), 127.f);
        qr[c] = (int8_t)(int)r;
    }
    if (lane == 0) scale[row] = sc;
}

static int qdot_check(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N, int64_t P,
                      int d, int dq) {
    if (!qu || !su || !qn || !sn || G < 0 || N < 0 || P < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (!pool && P != N) return DIGAT_ERR_ARG;
    if (d > QDOT_MAX_D) return DIGAT_ERR_SHAPE;
    if (dq != (d + 15) / 16 * 16 || ((((uintptr_t)qu) | ((uintptr_t)qn)) & 15)) return DIGAT_ERR_ARG;
    if ((double)dot_tiles((long)G) * (double)dot_chunks((long)P) > 2147483647.0) return DIGAT_ERR_SHAPE;
    return DIGAT_OK;
}

extern "C" {

int digat_quantize_rows_i8(const float* x, int64_t R, int d, int dq, int8_t* q, float* scale, void* stream) {
    if (!x || !q || !scale || R < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d > QDOT_MAX_D) return DIGAT_ERR_SHAPE;
    if (dq != (d + 15) / 16 * 16) return DIGAT_ERR_ARG;
    if ((R + 3) / 4 > 2147483647L) return DIGAT_ERR_SHAPE;
    if (R == 0) return DIGAT_OK;
    hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long)R, d, dq, q, scale);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

int digat_qdot_scores(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N, int64_t P,
                      int d, int dq, float* out, void* stream) {
    if (!out) return DIGAT_ERR_ARG;
    const int rc = qdot_check(qu, su, qn, sn, pool, G, N, P, d, dq);
    if (rc != DIGAT_OK) return rc;
    if (G == 0 || P == 0) return DIGAT_OK;
    const QdotArgs q{DotArgs{nullptr, nullptr, pool, (long)G, (long)N, (long)P, d, nullptr, 0, 0, dot_tiles((long)G), dot_chunks((long)P), out,
                             nullptr, nullptr, nullptr, nullptr},
                     qu, qn, su, sn, dq};
    hipLaunchKernelGGL(qdot_chunk_kernel<false>, dim3((unsigned)(q.a.tiles * q.a.chunks)), dim3(256), 0, (hipStream_t)stream, q);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

size_t digat_qdot_topk_workspace_bytes(int64_t users, int64_t pool, int k) { return digat_dot_topk_workspace_bytes(users, pool, k); }

int digat_qdot_topk(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N, int64_t P,
                    int d, int dq, const int64_t* skip, int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!out_scores || !out_ids || !out_count) return DIGAT_ERR_ARG;
    const size_t need = digat_qdot_topk_workspace_bytes(G, P, k);
    const int rc = topk_check_args(k, skip, skip_len, qdot_check(qu, su, qn, sn, pool, G, N, P, d, dq), need > 0, workspace);
    if (rc != DIGAT_OK) return rc;
    if (workspace_bytes < need) return DIGAT_ERR_WORKSPACE;
    if (G == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const QdotArgs q{DotArgs{nullptr, nullptr, pool, (long)G, (long)N, (long)P, d, skip, skip_len, k, dot_tiles((long)G), dot_chunks((long)P),
                             nullptr, (uint2*)workspace, out_scores, out_ids, out_count},
                     qu, qn, su, sn, dq};
    if (P > 0) {
        const size_t lds = (size_t)DOT_USERS * (size_t)(k + DOT_SUB) * sizeof(uint2);
        if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)qdot_chunk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess) return DIGAT_ERR_LAUNCH;
        hipLaunchKernelGGL(qdot_chunk_kernel<true>, dim3((unsigned)(q.a.tiles * q.a.chunks)), dim3(256), lds, st, q);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dot_topk_user_kernel, dim3((unsigned)G), dim3(256), 0, st, q.a);    // P == 0: no slot, every count 0
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

size_t digat_qdot_shortlist_workspace_bytes(int64_t G, int64_t P, int m, int64_t slab_users) {
    return digat_dot_shortlist_workspace_bytes(G, P, m, slab_users);
}

int digat_qdot_shortlist(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N,
                         int64_t P, int d, int dq, const int64_t* skip, int skip_len, int m, int64_t slab_users, float* out_scores,
                         int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
    return short_dot_slabs(
        pool, G, N, P, skip, skip_len, m, slab_users, out_scores, out_ids, out_count, workspace, workspace_bytes, (hipStream_t)stream,
        [&](long slab) { return qdot_check(qu, su, qn, sn, pool, G < 0 ? G : slab, N, P, d, dq); },
        [&](long g0, long gs, float* slab_scores, hipStream_t st) {
            const QdotArgs q{DotArgs{nullptr, nullptr, pool, gs, (long)N, (long)P, d, nullptr, 0, 0, dot_tiles(gs), short_dot_chunks((long)P),
                                     slab_scores, nullptr, nullptr, nullptr, nullptr},
                             qu + g0 * dq, qn, su + g0, sn, dq};
            hipLaunchKernelGGL((qdot_chunk_kernel<false, SHORT_DOT_CHUNK>), dim3((unsigned)(q.a.tiles * q.a.chunks)), dim3(256), 0, st, q);
        });
}

}  // extern "C"
