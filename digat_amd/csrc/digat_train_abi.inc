// digat_train_abi.inc — the three functions of the path as ONE training-forward and ONE backward C-ABI call each
// (SURVEY section 8b: digat_xattn_fwd/bwd, digat_news_ctx_fwd/bwd, digat_user_ctx_fwd/bwd).
// Included by digat_kernels.hip after digat_train.inc (one translation unit: hipcc --offload-arch=gfx950).
//
// Each pair composes the primitives of digat_train.inc on the C++ side — what digat_amd/training.py used to compose from
// ~15 autograd Functions per layer is now 3 Functions with one library call per direction: the host enqueues a training
// step's ~500 launches from ~45 library calls instead of ~500 (the step was bound by the host, DESIGN.md section 4).  What a
// backward needs from its forward travels in a caller-owned `save` buffer (sizes from the *_save_bytes functions; the
// layout is private to this file); scratch comes from `workspace`.  Dropout uses the library's counter-hash generator
// (digat_dropout_fwd) with the caller's seeds; p = 0 disables it.  All reductions are ordered: gradients are bit-reproducible.

static bool x3_ok(long M, int n_out, int k_in) { return M >= 2048 && n_out % 80 == 0 && k_in % 8 == 0 && k_in >= 32; }
static size_t wsplit_scratch(int d) { return digat_split_weights_bytes(3 * d, 2 * d); }     // covers every split made here

// y[M,N] = x[M,K] W[N,K]^T (+ b): bf16x6 on >= 2048 rows, fp32 MFMA below (training.py's _linear_fwd)
static int t_linear_fwd(const float* x, long ldx, const float* W, const float* b, float* y, int M, int N, int K, void* wsplit,
                        hipStream_t st) {
    if (x3_ok(M, N, K) && ldx % 4 == 0) return digat_linear_f32x3(x, ldx, W, b, y, N, M, N, K, wsplit, DIGAT_GEMM_BF16X6, st);
    return digat_linear_f32(x, ldx, W, b, y, N, M, N, K, st);
}
// dx[M,K] (+)= dy[M,N] W[N,K]
static int t_linear_bwd_input(const float* dy, const float* W, float* dx, int M, int N, int K, int accumulate, void* wsplit,
                              hipStream_t st) {
    if (x3_ok(M, K, N)) return digat_linear_bwd_input_x3(dy, N, W, dx, K, M, N, K, accumulate, wsplit, st);
    return digat_linear_bwd_input(dy, N, W, dx, K, M, N, K, accumulate, st);
}
// dW[No,Ni] = dy[M,No]^T x[M,Ni]; db = colsum(dy) (db may be NULL)
static int t_linear_bwd_weight(const float* dy, const float* x, long ldx, float* dW, float* db, int M, int No, int Ni, void* ws,
                               size_t ws_bytes, hipStream_t st) {
    return digat_linear_bwd_weight(dy, No, x, ldx, dW, db, M, No, Ni, 0, ws, ws_bytes, st);
}
#define T_TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)

extern "C" {

// ============================================================================================================
// a1 / a2: Eq. 8 layer, training (graphEncoders.py:143-154 / :163-174)
//   X: the layer's input AFTER its input dropout (the caller applies drop_{p/2}; the residual uses the dropped input, :145,153)
//   out = relu(drop_p(alpha) h) + X, alpha from the masked softmax of leaky_relu(a . relu(K3 + K1 + K2))
// ============================================================================================================
// save: h, P', Q, r, alpha, s_pre, the attention dropout's keep bytes; the dropped input and the input dropout's keep bytes (p_in > 0)
struct XattnSave { float *h, *Pr, *Q, *r, *alpha, *s_pre; uint8_t* amask; float* Xd; uint8_t* xmask; int* sflag; };
static XattnSave xattn_save_carve(Arena& a, int B, int n, int d) {
    const size_t nd = (size_t)B * n * d, nn = (size_t)B * n * n;
    XattnSave s;
    s.h = a.take<float>(nd); s.Pr = a.take<float>(nd); s.Q = a.take<float>(nd); s.r = a.take<float>((size_t)B * d);
    s.alpha = a.take<float>(nn); s.s_pre = a.take<float>(nn); s.amask = a.take<uint8_t>(nn);
    s.Xd = a.take<float>(nd); s.xmask = a.take<uint8_t>(nd);
    s.sflag = a.take<int>(1);                      // sparse or dense Eq. 8 for this batch: decided on the device by the forward, read by the backward
    return s;
}
// forward workspace: alpha after dropout + split scratch
struct XattnFwdWs { float* adrop; void* wsplit; };
static XattnFwdWs xattn_fwd_carve(Arena& w, int B, int n, int d) {
    return XattnFwdWs{w.take<float>((size_t)B * n * n), w.take<char>(wsplit_scratch(d))};      // braces: taken left to right
}
// backward workspace: G = [dh | dP' | dQ] ([B n, 3 d]), dr, the pairwise backward's own scratch, dW scratch, split scratch, the
// stacked [dW; dF1; dF2] for callers whose three buffers are not one, the image of the stacked weights' transpose
struct XattnBwdWs { float *G, *dr; void* pws; size_t pb; void* wws; size_t wb; void* wsplit; float* wg3; void* wcat_split; };
static XattnBwdWs xattn_bwd_carve(Arena& w, int B, int n, int d) {
    XattnBwdWs o;
    o.G = w.take<float>(3 * (size_t)B * n * d);
    o.dr = w.take<float>((size_t)B * d);
    o.pb = digat_xattn_pairwise_bwd_workspace(B, n, d);
    o.wb = digat_linear_bwd_weight_workspace(B * n, 3 * d, d);
    o.pws = w.take<char>(o.pb); o.wws = w.take<char>(o.wb); o.wsplit = w.take<char>(wsplit_scratch(d));
    o.wg3 = w.take<float>(3 * (size_t)d * d);
    o.wcat_split = w.take<char>(digat_split_weights_bytes(d, 3 * d));
    return o;
}
size_t digat_xattn_train_save_bytes(int B, int n, int d) { Arena a; xattn_save_carve(a, B, n, d); return a.used; }
size_t digat_xattn_train_workspace_bytes(int B, int n, int d) {        // one buffer serves both directions
    Arena fwd, bwd;
    xattn_fwd_carve(fwd, B, n, d); xattn_bwd_carve(bwd, B, n, d);
    return larger(fwd, bwd);
}

int digat_xattn_fwd_train(const float* X, const uint8_t* A, const float* ctx, const float* W, const float* bW, const float* F1,
                          const float* F2, const float* F3, const float* b3, const float* a, float* out, float p_alpha,
                          uint32_t seed, float p_in, uint32_t seed_in, int B, int n, int d, void* save, size_t save_bytes, void* workspace,
                          size_t workspace_bytes, const void* proj_image, int xattn_mode, void* stream) {
    if (!X || !A || !ctx || !W || !bW || !F1 || !F2 || !F3 || !b3 || !a || !out || !save || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0 || p_alpha < 0.f || p_alpha >= 1.f || p_in < 0.f || p_in >= 1.f || xattn_mode < 0 || xattn_mode > 2) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    const XattnSave s = xattn_save_carve(sa, B, n, d);
    if (!sa.ok || workspace_bytes < digat_xattn_train_workspace_bytes(B, n, d)) return DIGAT_ERR_WORKSPACE;
    const XattnFwdWs o = xattn_fwd_carve(w, B, n, d);
    void* wsplit = o.wsplit;
    hipStream_t st = (hipStream_t)stream;
    if (p_in > 0.f) {        // the layer's input dropout (:145 / :165), kept with its keep bytes: the projections, the residual and the backward read Xd
        T_TRY(digat_dropout_fwd(X, s.Xd, s.xmask, (int64_t)B * n * d, p_in, seed_in, st));
        X = s.Xd;
    }
    T_TRY(digat_linear_f32(ctx, d, F3, b3, s.r, d, B, d, d, st));                                   // K3
    // proj_image: [W | F1 | F2] already split by the caller (digat_split_jobs, layout 0): no split launch here
    const PremadeImage premade(proj_image);
    if (proj_image) wsplit = const_cast<void*>(proj_image);
    if (x3_ok((long)B * n, d, d)) T_TRY(digat_xattn_project_x3(X, s.r, W, bW, F1, F2, s.h, s.Pr, s.Q, B, n, d, wsplit, st));
    else T_TRY(digat_xattn_project(X, s.r, W, bW, F1, F2, s.h, s.Pr, s.Q, B, n, d, st));
    // (s_pre is written on the adjacency's entries only and read, by xattn_ds_kernel, behind the adjacency test only: de = 0 off the
    // entries whatever the slot holds — 0 x (sp > 0 ? 1 : 0.2) — so the rest of the buffer needs no zero-fill: six memsets per step less)
    TrainEq8Opts eo;
    eo.sparse_flag = s.sflag; eo.mode = xattn_mode;
    return xattn_pairwise_fwd_train_flag(s.Pr, s.Q, s.h, X, a, A, out, s.alpha, s.s_pre, p_alpha > 0.f ? o.adrop : nullptr,
                                         p_alpha > 0.f ? s.amask : nullptr, p_alpha, seed, B, n, d, st, eo);
}

// dX [B,n,d], dctx [B,d], dW dF1 dF2 dF3 [d,d], dbW db3 [d], da [d]: all written (not accumulated)
int digat_xattn_bwd(const float* dOut, const float* out, const float* X, const uint8_t* A, const float* ctx, const float* W,
                    const float* F1, const float* F2, const float* F3, const float* a, float p_alpha, float p_in, const void* save,
                    size_t save_bytes, float* dX, float* dctx, float* dW, float* dbW, float* dF1, float* dF2, float* dF3,
                    float* db3, float* da, int B, int n, int d, void* workspace, size_t workspace_bytes, const void* bwd_image,
                    int xattn_mode, void* stream) {
    if (!dOut || !out || !X || !A || !ctx || !W || !F1 || !F2 || !F3 || !a || !save || !dX || !dctx || !dW || !dbW || !dF1 || !dF2 ||
        !dF3 || !db3 || !da || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0 || xattn_mode < 0 || xattn_mode > 2) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const size_t dd = (size_t)d * d;
    if (B == 0) return zero_floats(st, {{dW, dd}, {dF1, dd}, {dF2, dd}, {dF3, dd}, {dbW, (size_t)d}, {db3, (size_t)d}, {da, (size_t)d}});
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    const XattnSave s = xattn_save_carve(sa, B, n, d);
    if (!sa.ok || workspace_bytes < digat_xattn_train_workspace_bytes(B, n, d)) return DIGAT_ERR_WORKSPACE;
    const XattnBwdWs o = xattn_bwd_carve(w, B, n, d);
    const size_t nd = (size_t)B * n * d;
    // the three gradients are the column blocks of ONE matrix G = [dh | dP' | dQ] ([B n, 3 d]): their input-gradient products are
    // then a single product with the stacked weights [W; F1; F2] (one pass over dX instead of three read-modify-writes)
    float* G = o.G;
    const long ldg = 3L * d;
    float* dh = G; float* dPr = G + d; float* dQ = G + 2 * d;
    void* wcat_split = o.wcat_split;
    const int M = B * n;
    const uint8_t* xmask = nullptr;
    const float xscale = p_in > 0.f ? 1.f / (1.f - p_in) : 1.f;
    if (p_in > 0.f) { X = s.Xd; xmask = s.xmask; }     // the forward dropped its input itself: the layer saw Xd; dX goes back through the keep bytes
    // bwd_image: the stack [W; F1; F2] already split for the input-gradient product (digat_split_jobs, layout 1, three matrices)
    const PremadeImage premade(bwd_image);
    if (bwd_image) wcat_split = const_cast<void*>(bwd_image);
    // (dr[b] = sum_j dP'[b,j] — K3 = ctx F3^T + b3 was added to every neighbour-side row — leaves the pairwise backward's launch)
    TrainEq8Opts eo;
    eo.sparse_flag = s.sflag; eo.mode = xattn_mode; eo.dr = o.dr;
    T_TRY(xattn_pairwise_bwd_ld(dOut, out, X, s.Pr, s.Q, s.h, a, A, s.alpha, s.s_pre, p_alpha > 0.f ? s.amask : nullptr, p_alpha,
                                dPr, dQ, dh, ldg, da, 0, B, n, d, o.pws, o.pb, st, eo));
    // projections: dX = dOut (residual) + dh W + dP' F1 + dQ F2 = dOut + G [W; F1; F2]
    if (x3_ok(M, d, 3 * d)) {
        // the stacked weights [W; F1; F2] are split from their three homes
        T_TRY(linear_bwd_input_x3_add(G, ldg, W, dX, d, dOut, M, 3 * d, d, wcat_split, st, F1, F2, xmask, xscale));   // dOut joins in the epilogue, and the input dropout's backward
    } else {
        if (hipMemcpyAsync(dX, dOut, nd * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
        T_TRY(digat_linear_bwd_input(dh, ldg, W, dX, d, M, d, d, 1, st));
        T_TRY(digat_linear_bwd_input(dPr, ldg, F1, dX, d, M, d, d, 1, st));
        T_TRY(digat_linear_bwd_input(dQ, ldg, F2, dX, d, M, d, d, 1, st));
        if (xmask) T_TRY(digat_dropout_bwd(dX, xmask, dX, (int64_t)nd, p_in, st));
    }
    // ... and the three weight gradients one product G^T X ([3 d, d]; the column sums of G's first block are dbW)
    // a caller that hands over dW, dF1, dF2 as the three blocks of ONE [3 d, d] buffer (training.XattnFused does) gets the product
    // written in place: no copies; separate buffers get theirs from o.wg3 by three device copies
    const bool stacked = dF1 == dW + dd && dF2 == dW + 2 * dd;
    // (the reduction writes the d leading column sums — dbW — where they belong)
    T_TRY(linear_bwd_weight_dbn(G, ldg, X, d, stacked ? dW : o.wg3, dbW, d, M, 3 * d, d, 0, o.wws, o.wb, st));
    if (!stacked && (hipMemcpyAsync(dW, o.wg3, dd * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                     hipMemcpyAsync(dF1, o.wg3 + dd, dd * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                     hipMemcpyAsync(dF2, o.wg3 + 2 * dd, dd * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)) return DIGAT_ERR_LAUNCH;
    T_TRY(t_linear_bwd_input(o.dr, F3, dctx, B, d, d, 0, o.wsplit, st));
    return t_linear_bwd_weight(o.dr, ctx, d, dF3, db3, B, d, d, o.wws, o.wb, st);
}

// ============================================================================================================
// a3: news-graph context, training (graphEncoders.py:109-114):  l = X[:,0]; g = SDPA(X, l, mask);
//     out = gate(drop_{p/2}(W_g [l;g] + b_g), l, g)
// ============================================================================================================
struct NewsCtxSave { float *qv, *kq, *zd, *alpha, *cat; uint8_t* zmask; };
static NewsCtxSave news_save_carve(Arena& a, int B, int N, int d) {
    NewsCtxSave s;
    s.qv = a.take<float>((size_t)B * d); s.kq = a.take<float>((size_t)B * d); s.zd = a.take<float>((size_t)B * d);
    s.alpha = a.take<float>((size_t)B * N); s.cat = a.take<float>((size_t)B * 2 * d); s.zmask = a.take<uint8_t>((size_t)B * d);
    return s;
}
// forward workspace: the gate's pre-activation z [B,d]
static float* news_fwd_carve(Arena& w, int B, int d) { return w.take<float>((size_t)B * d); }
// backward workspace: dz, dkq, dqv [B,d]; [dl | dg] [B,2d]; the scratch of the three weight-gradient products (collected and issued
// together: each has its own slices)
struct NewsCtxBwdWs { float *dz, *dkq, *dqv, *dlg; void* wws; size_t wb; };
static NewsCtxBwdWs news_bwd_carve(Arena& w, int B, int d) {
    const size_t bd = (size_t)B * d;
    NewsCtxBwdWs o;
    o.dz = w.take<float>(bd); o.dkq = w.take<float>(bd); o.dqv = w.take<float>(bd); o.dlg = w.take<float>(2 * bd);
    o.wb = align_up(digat_linear_bwd_weight_workspace(B, d, 2 * d), 256) + 2 * align_up(digat_linear_bwd_weight_workspace(B, d, d), 256);
    o.wws = w.take<char>(o.wb);
    return o;
}
size_t digat_news_ctx_train_save_bytes(int B, int N, int d) { Arena a; news_save_carve(a, B, N, d); return a.used; }
size_t digat_news_ctx_train_workspace_bytes(int B, int N, int d) {
    (void)N;
    Arena fwd, bwd;
    news_fwd_carve(fwd, B, d); news_bwd_carve(bwd, B, d);
    return larger(fwd, bwd);
}
// dX[b,0,:] += dl[b] (the local context is node 0 of every row)
__global__ void __launch_bounds__(256) add_node0_kernel(float4* dX, long ldx4, const float4* dl, long ldl4, long B, int d4) {
    const long total = B * d4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / d4;
        const int c = (int)(i - b * d4);
        dX[b * ldx4 + c] = f4_add(dX[b * ldx4 + c], dl[b * ldl4 + c]);
    }
}
int digat_news_ctx_fwd_train(const float* X, const uint8_t* mask, const float* Kc, const float* Qc, const float* bQc,
                             const float* Wg, const float* bg, float* out, float p_gate, uint32_t seed, int B, int N, int d,
                             void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, const float* prev, void* stream) {
    if (!X || !mask || !Kc || !Qc || !bQc || !Wg || !bg || !out || !save || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || N <= 0 || d <= 0 || p_gate < 0.f || p_gate >= 1.f) return DIGAT_ERR_ARG;
    if (d % 4 || N > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    const NewsCtxSave s = news_save_carve(sa, B, N, d);
    if (!sa.ok || workspace_bytes < digat_news_ctx_train_workspace_bytes(B, N, d)) return DIGAT_ERR_WORKSPACE;
    float* z = news_fwd_carve(w, B, d);
    hipStream_t st = (hipStream_t)stream;
    const long ldx = (long)N * d;
    T_TRY(digat_linear_f32(X, ldx, Qc, bQc, s.qv, d, B, d, d, st));                                 // Q l + b
    T_TRY(digat_linear_bwd_input(s.qv, d, Kc, s.kq, d, B, d, d, 0, st));                            // K^T (Q l + b)
    // the pooling launch writes the saved [l ; g] rows itself: g into the second half, node 0 (= l) into the first (round 6: the
    // concatenation launch is gone); the gate applies its own dropout (one launch instead of dropout + gate)
    T_TRY(attn_pool_fwd_ld(X, ldx, s.kq, mask, s.cat + d, 2L * d, s.cat, 2L * d, s.alpha, B, N, d, st));
    T_TRY(digat_linear_f32(s.cat, 2 * d, Wg, bg, z, d, B, d, 2 * d, st));
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(grid_for((long)B * d)), dim3(256), 0, st, (const float*)z, X, ldx, (const float*)(s.cat + d), 2L * d,
                       out, s.zd, p_gate > 0.f ? s.zmask : (uint8_t*)nullptr, p_gate, seed, B, d, prev);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// dX [B,N,d] is WRITTEN (every node: pooled values + node 0's extra paths); dKc dQc [d,d], dbQc [d], dWg [d,2d], dbg [d]
int digat_news_ctx_bwd(const float* dout, const float* X, const uint8_t* mask, const float* Kc, const float* Qc, const float* Wg,
                       float p_gate, const void* save, size_t save_bytes, float* dX, float* dKc, float* dQc, float* dbQc,
                       float* dWg, float* dbg, int B, int N, int d, int accumulate_params, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!dout || !X || !mask || !Kc || !Qc || !Wg || !save || !dX || !dKc || !dQc || !dbQc || !dWg || !dbg || !workspace)
        return DIGAT_ERR_ARG;
    if (B <= 0 || N <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || N > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    const NewsCtxSave s = news_save_carve(sa, B, N, d);
    if (!sa.ok || workspace_bytes < digat_news_ctx_train_workspace_bytes(B, N, d)) return DIGAT_ERR_WORKSPACE;
    const NewsCtxBwdWs o = news_bwd_carve(w, B, d);
    float *dz = o.dz, *dkq = o.dkq, *dqv = o.dqv, *dlg = o.dlg;
    const size_t bd = (size_t)B * d;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate_params ? 1 : 0;
    TnGroup dws(o.wws, o.wb, st);                      // the entry's three weight gradients: one product launch + one reduction at the end
    const long ldx = (long)N * d;
    // gate: out = sig(zd) l + (1 - sig(zd)) g, zd = dropout(z).  Round 6: one launch gives dz (through the dropout's keep bytes) and
    // the gate's dl, dg as the two halves of ONE [B, 2 d] matrix [dl | dg] — the matrix z's other path adds to: [dl | dg] += dz Wg —
    // where round 5 ran a copy of g, the gate, the dropout, the product into a scratch matrix and two column-block adds
    float* dl = dlg; float* dg = dlg + d;
    const long ld2 = 2L * d;
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(grid_for((long)bd)), dim3(256), 0, st, dout, (const float*)s.zd, X, ldx, (const float*)(s.cat + d), ld2,
                       p_gate > 0.f ? (const uint8_t*)s.zmask : (const uint8_t*)nullptr, p_gate > 0.f ? 1.f / (1.f - p_gate) : 1.f, dz, dl, dg,
                       ld2, B, d);
    DIGAT_CHECK_LAUNCH();
    // z = [l ; g] Wg^T + bg
    T_TRY(dws.add(dz, d, s.cat, 2 * d, dWg, dbg, B, d, 2 * d, acc));
    T_TRY(digat_linear_bwd_input(dz, d, Wg, dlg, 2 * d, B, d, 2 * d, 1, st));                       // [dl | dg] += dz Wg
    // g = SDPA pooling of X with the folded query kq
    T_TRY(attn_pool_bwd_ld(X, ldx, s.kq, mask, s.alpha, dg, ld2, dX, ldx, dkq, B, N, d, 0, st));
    // kq = qv @ Kc: dqv = dkq Kc^T, dKc[n][k] = sum_m qv[m][n] dkq[m][k]
    T_TRY(digat_linear_f32(dkq, d, Kc, nullptr, dqv, d, B, d, d, st));
    T_TRY(dws.add(s.qv, d, dkq, d, dKc, nullptr, B, d, d, acc));
    // qv = l Qc^T + bQc
    T_TRY(dws.add(dqv, d, X, ldx, dQc, dbQc, B, d, d, acc));
    T_TRY(digat_linear_bwd_input(dqv, d, Qc, dl, ld2, B, d, d, 1, st));                             // dl += dqv Qc
    hipLaunchKernelGGL(add_node0_kernel, dim3(grid_for((long)bd / 4)), dim3(256), 0, st, (float4*)dX, ldx / 4, (const float4*)dl, ld2 / 4, (long)B, d / 4);
    DIGAT_CHECK_LAUNCH();
    return dws.flush();                            // (their operands dz, s.cat, s.qv, dkq, dqv, X are not written after their producers)
}

// ============================================================================================================
// a4 (+a6, a7): user-graph context, training (graphEncoders.py:123-134)
// ============================================================================================================
struct UserCtxSave { float *qv, *kq, *qv2, *kq2, *alpha_t, *T, *y, *T2d, *alpha_u; uint8_t* tmask; };
static UserCtxSave user_save_carve(Arena& a, int B, int H, int C1, int d) {
    const size_t bd = (size_t)B * d, t = (size_t)B * C1 * d;
    UserCtxSave s;
    s.qv = a.take<float>(bd); s.kq = a.take<float>(bd); s.qv2 = a.take<float>(bd); s.kq2 = a.take<float>(bd);
    s.alpha_t = a.take<float>((size_t)B * H);
    s.T = a.take<float>(t); s.y = a.take<float>(t); s.T2d = a.take<float>(t);
    s.tmask = a.take<uint8_t>(t); s.alpha_u = a.take<float>((size_t)B * C1);
    return s;
}
// forward workspace: split scratch
static void* user_fwd_carve(Arena& w, int d) { return w.take<char>(wsplit_scratch(d)); }
// backward workspace: dT2d, dT2, dy [B,C1,d]; dkq2, dqv2, dkq, dqv [B,d]; the scratch of dFa's product and of the four short ones of
// the query chains (collected and issued together); split scratch
struct UserCtxBwdWs { float *dT2d, *dT2, *dy, *dkq2, *dqv2, *dkq, *dqv; void* wws; size_t wb; void* wsplit; };
static UserCtxBwdWs user_bwd_carve(Arena& w, int B, int C1, int d) {
    const size_t bd = (size_t)B * d, t = (size_t)B * C1 * d;
    UserCtxBwdWs o;
    o.dT2d = w.take<float>(t); o.dT2 = w.take<float>(t); o.dy = w.take<float>(t);
    o.dkq2 = w.take<float>(bd); o.dqv2 = w.take<float>(bd); o.dkq = w.take<float>(bd); o.dqv = w.take<float>(bd);
    o.wb = align_up(digat_linear_bwd_weight_workspace(B * C1, d, d), 256) + 4 * align_up(digat_linear_bwd_weight_workspace(B, d, d), 256);
    o.wws = w.take<char>(o.wb); o.wsplit = w.take<char>(wsplit_scratch(d));
    return o;
}
size_t digat_user_ctx_train_save_bytes(int B, int U, int H, int C1, int d) { (void)U; Arena a; user_save_carve(a, B, H, C1, d); return a.used; }
size_t digat_user_ctx_train_workspace_bytes(int B, int U, int H, int C1, int d) {
    (void)U; (void)H;
    Arena fwd, bwd;
    user_fwd_carve(fwd, d); user_bwd_carve(bwd, B, C1, d);
    return larger(fwd, bwd);
}

int digat_user_ctx_fwd_train(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n, const float* Ku,
                             const float* Qu, const float* bQu, const float* Fa, const float* bFa, const float* Kua,
                             const float* Qua, const float* bQua, float* out, float p_topic, uint32_t seed, int B, int U, int H,
                             int C1, int d, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, const void* fa_image,
                             const float* prev, void* stream) {
    if (!Xu || !cat_mask || !cat_idx || !c_n || !Ku || !Qu || !bQu || !Fa || !bFa || !Kua || !Qua || !bQua || !out || !save || !workspace)
        return DIGAT_ERR_ARG;
    if (B < 0 || H < 0 || U < H || C1 <= 0 || d <= 0 || p_topic < 0.f || p_topic >= 1.f) return DIGAT_ERR_ARG;
    if (d % 4 || C1 > DIGAT_MAX_NODES || H > TOPIC_MAX_H) return DIGAT_ERR_SHAPE;
    if (B == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    const UserCtxSave s = user_save_carve(sa, B, H, C1, d);
    if (!sa.ok || workspace_bytes < digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)) return DIGAT_ERR_WORKSPACE;
    void* wsplit = user_fwd_carve(w, d);
    hipStream_t st = (hipStream_t)stream;
    const int M = B * C1;
    const PremadeImage premade(fa_image);          // featureAffine.weight already split (digat_split_jobs, layout 0)
    if (fa_image) wsplit = const_cast<void*>(fa_image);
    {   // the two queries of c_n — topic-level (:126-128) and user-level (:133) — as the two segments of one launch
        GemmArgs q2 = gemm_plain(c_n, d, Qu, bQu, s.qv, d, B, d, d, 0);
        q2.w[1] = Qua; q2.bias[1] = bQua; q2.y[1] = s.qv2; q2.nsegs = 2;
        T_TRY(launch_gemm(q2, st));
    }
    T_TRY(digat_linear_bwd_input(s.qv, d, Ku, s.kq, d, B, d, d, 0, st));
    T_TRY(digat_topic_pool_fwd_train(Xu, s.kq, cat_idx, s.T, s.alpha_t, B, U, H, C1, d, st));       // scatter_softmax + scatter_sum (:129-130)
    T_TRY(t_linear_fwd(s.T, d, Fa, bFa, s.y, M, d, d, wsplit, st));                                 // featureAffine (:131)
    // relu + residual + dropout: one launch
    hipLaunchKernelGGL(relu_res_drop_fwd_kernel, dim3(grid_for((long)M * d)), dim3(256), 0, st, (const float*)s.y, (const float*)s.T, s.T2d,
                       p_topic > 0.f ? s.tmask : (uint8_t*)nullptr, (long)M * d, p_topic, seed);
    DIGAT_CHECK_LAUNCH();
    T_TRY(digat_linear_bwd_input(s.qv2, d, Kua, s.kq2, d, B, d, d, 0, st));                         // user-level attention (:133)
    return attn_pool_fwd_ld(s.T2d, (long)C1 * d, s.kq2, cat_mask, out, 0, nullptr, 0, s.alpha_u, B, C1, d, st, prev);   // out = prev + pooled (:186)
}

// dXu [B,U,d] is WRITTEN (history rows: the pooling's gradient; topic rows: zero), dc_n [B,d] written
int digat_user_ctx_bwd(const float* dout, const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n,
                       const float* Ku, const float* Qu, const float* Fa, const float* Kua, const float* Qua, float p_topic,
                       const void* save, size_t save_bytes, float* dXu, float* dc_n, float* dKu, float* dQu, float* dbQu,
                       float* dFa, float* dbFa, float* dKua, float* dQua, float* dbQua, int B, int U, int H, int C1, int d,
                       int accumulate_params, void* workspace, size_t workspace_bytes, const void* fa_bwd_image, void* stream) {
    if (!dout || !Xu || !cat_mask || !cat_idx || !c_n || !Ku || !Qu || !Fa || !Kua || !Qua || !save || !dXu || !dc_n || !dKu || !dQu ||
        !dbQu || !dFa || !dbFa || !dKua || !dQua || !dbQua || !workspace) return DIGAT_ERR_ARG;
    if (B <= 0 || H < 0 || U < H || C1 <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || C1 > DIGAT_MAX_NODES || H > TOPIC_MAX_H) return DIGAT_ERR_SHAPE;
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    const UserCtxSave s = user_save_carve(sa, B, H, C1, d);
    if (!sa.ok || workspace_bytes < digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)) return DIGAT_ERR_WORKSPACE;
    const UserCtxBwdWs o = user_bwd_carve(w, B, C1, d);
    float *dT2d = o.dT2d, *dT2 = o.dT2, *dy = o.dy, *dkq2 = o.dkq2, *dqv2 = o.dqv2, *dkq = o.dkq, *dqv = o.dqv;
    const size_t t = (size_t)B * C1 * d;
    void* wsplit = o.wsplit;
    const int M = B * C1;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate_params ? 1 : 0;
    const PremadeImage premade(fa_bwd_image);      // featureAffine.weight already split for the input gradient (digat_split_jobs, layout 1)
    if (fa_bwd_image) wsplit = const_cast<void*>(fa_bwd_image);
    TnGroup dws(o.wws, o.wb, st);                  // dFa's long product goes out at once; the four short ones together at the end
    // user-level attention over the (dropped) topic representations
    T_TRY(digat_attn_pool_bwd(s.T2d, (long)C1 * d, s.kq2, cat_mask, s.alpha_u, dout, dT2d, (long)C1 * d, dkq2, B, C1, d, 0, st));
    // T2 = relu(y) + T,  y = T Fa^T + bFa:  dT = dT2 + dy Fa; dT2 = dropout'(dT2d) and dy = dT2 [y > 0] in one launch (round 6)
    hipLaunchKernelGGL(drop_relu_bwd_kernel, dim3(grid_for((long)t)), dim3(256), 0, st, (const float*)dT2d,
                       p_topic > 0.f ? (const uint8_t*)s.tmask : (const uint8_t*)nullptr, p_topic > 0.f ? 1.f / (1.f - p_topic) : 1.f,
                       (const float*)s.y, dT2, dy, (long)t);
    DIGAT_CHECK_LAUNCH();
    T_TRY(dws.add(dy, d, s.T, d, dFa, dbFa, M, d, d, acc));
    T_TRY(t_linear_bwd_input(dy, Fa, dT2, M, d, d, 1, wsplit, st));                                 // dT2 now holds dT
    // topic pooling: history rows of dXu, and the folded query
    T_TRY(topic_pool_bwd_zero(Xu, s.kq, cat_idx, s.alpha_t, dT2, dXu, dkq, B, U, H, C1, d, st));      // every row of dXu is written there
    // the two query chains from c_n
    T_TRY(digat_linear_f32(dkq, d, Ku, nullptr, dqv, d, B, d, d, st));
    T_TRY(dws.add(s.qv, d, dkq, d, dKu, nullptr, B, d, d, acc));
    T_TRY(dws.add(dqv, d, c_n, d, dQu, dbQu, B, d, d, acc));
    T_TRY(digat_linear_bwd_input(dqv, d, Qu, dc_n, d, B, d, d, 0, st));
    T_TRY(digat_linear_f32(dkq2, d, Kua, nullptr, dqv2, d, B, d, d, st));
    T_TRY(dws.add(s.qv2, d, dkq2, d, dKua, nullptr, B, d, d, acc));
    T_TRY(dws.add(dqv2, d, c_n, d, dQua, dbQua, B, d, d, acc));
    T_TRY(digat_linear_bwd_input(dqv2, d, Qua, dc_n, d, B, d, d, 1, st));
    return dws.flush();
}

}  // extern "C"
