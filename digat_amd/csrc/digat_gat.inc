// digat_gat.inc — the vanilla-GAT update layer of the reference's ablation encoders (SURVEY §8f-3:
// graphEncoders.py:493-519 wo_interaction, :641-651 News_graph_wo_inter, :788-798 User_graph_wo_inter):
//   h = X W^T + b ;  e_ij = leaky_relu_0.2(a1.h_j + a2.h_i) ;  -1e9 where the adjacency is 0 ;  alpha = softmax_j ;
//   out = relu(alpha h) + X
// The score is separable, so it costs two dot products per node; the aggregation is the Eq. 8 aggregation kernel.
// Included at the end of digat_kernels.hip.

// s1[node] = a1 . h[node], s2[node] = a2 . h[node]: one wave per node, lanes span the channels
__global__ void __launch_bounds__(256) gat_node_scores_kernel(const float* h, const float* a1, const float* a2, float* s1, float* s2,
                                                              long nodes, int d4) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long node = (long)blockIdx.x * 4 + wave;
    if (node >= nodes) return;
    const float4* row = reinterpret_cast<const float4*>(h) + node * d4;
    const float4* A1 = reinterpret_cast<const float4*>(a1);
    const float4* A2 = reinterpret_cast<const float4*>(a2);
    float p1 = 0.f, p2 = 0.f;
    for (int c4 = lane; c4 < d4; c4 += 64) {
        const float4 v = row[c4], x = A1[c4], y = A2[c4];
        p1 = fmaf(x.w, v.w, fmaf(x.z, v.z, fmaf(x.y, v.y, fmaf(x.x, v.x, p1))));
        p2 = fmaf(y.w, v.w, fmaf(y.z, v.z, fmaf(y.y, v.y, fmaf(y.x, v.x, p2))));
    }
    p1 = wave_sum(p1);
    p2 = wave_sum(p2);
    if (lane == 0) { s1[node] = p1; s2[node] = p2; }
}

// alpha[b][i][:] for one (b, i) per wave; n <= 128: two neighbours per lane
// (s_pre, when set, keeps the sums before leaky_relu / the mask for the backward's leaky_relu')
__global__ void __launch_bounds__(256) gat_alpha_kernel(const float* s1, const float* s2, const uint8_t* A, float* alpha, float* s_pre,
                                                        long rows, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rho = (long)blockIdx.x * 4 + wave;            // b * n + i
    if (rho >= rows) return;
    const long b = rho / n;
    const float si = s2[rho];
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        v[h] = -INFINITY;
        if (j < n) {
            const float e = s1[b * n + j] + si;                                        // a1 + a2 (:499, a1 broadcast over i, a2 over j)
            if (s_pre) s_pre[rho * n + j] = e;
            v[h] = A[rho * n + j] ? (e > 0.f ? e : 0.2f * e) : -1e9f;                  // leaky_relu, then masked_fill(graph == 0, -1e9)
        }
    }
    const float m = wave_max(fmaxf(v[0], v[1]));
    const float e0 = lane < n ? expf(v[0] - m) : 0.f;
    const float e1 = lane + 64 < n ? expf(v[1] - m) : 0.f;
    const float inv = wave_sum(e0 + e1);
    if (lane < n) alpha[rho * n + lane] = e0 / inv;
    if (lane + 64 < n) alpha[rho * n + lane + 64] = e1 / inv;
}

// inference workspace: h [B,n,d], the two node scores [B,n] each, alpha [B,n,n]
struct GatWs { float *h, *s1, *s2, *alpha; };
static GatWs gat_carve(Arena& w, int B, int n, int d) {
    const size_t bn = (size_t)B * n;
    return GatWs{w.take<float>(bn * d), w.take<float>(bn), w.take<float>(bn), w.take<float>(bn * n)};      // braces: taken left to right
}

// the aggregation's route: d <= 1024 (eq8_agg_route's upto_1024), asked before the first launch of an entry
static Eq8AggRoute gat_agg_route(int B, int n, int d) { return eq8_agg_route(B, n, d, true, EQ8_UNGUARDED); }

extern "C" {

size_t digat_gat_workspace_bytes(int B, int n, int d) { Arena a; gat_carve(a, B, n, d); return a.used; }

int digat_gat_fwd(const float* X, const uint8_t* A, const float* W, const float* bW, const float* a1, const float* a2,
                  float* out, int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream) {
    if (!X || !A || !W || !a1 || !a2 || !out || !workspace || B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES || gat_agg_route(B, n, d).status) return DIGAT_ERR_SHAPE;      // before any launch
    Arena w(workspace, workspace_bytes);
    const GatWs o = gat_carve(w, B, n, d);
    if (!w.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_gemm(gemm_plain(X, d, W, bW, o.h, d, B * n, d, d, 0), st, DIGAT_KERNEL_PROJ);
    if (rc) return rc;
    const long nodes = (long)B * n;
    hipLaunchKernelGGL(gat_node_scores_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, st, (const float*)o.h, a1, a2, o.s1, o.s2, nodes, d / 4);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(gat_alpha_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, st, (const float*)o.s1, (const float*)o.s2, A, o.alpha, (float*)nullptr, nodes, n);
    DIGAT_CHECK_LAUNCH();
    return launch_agg(agg_args(o.alpha, o.h, X, out, B, n, d), gat_agg_route(B, n, d), st);
}

}  // extern "C"

// ---- training (graphEncoders.py:493-519 with dropout live) ---------------------------------------------------
// backward of the separable score: with ds[i][j] the gradient at a1.h_j + a2.h_i (from xattn_ds_kernel),
//   du_j = sum_i ds_ij, dv_i = sum_j ds_ij;  dh_j += du_j a1 + dv_j a2;  da1 = sum_j du_j h_j;  da2 = sum_i dv_i h_i.
// One workgroup per row b, sums in index order (bit-reproducible); da partials [B][2d] are reduced over b by colsum_kernel.
struct GatScoreBwdArgs { const float* ds; const float* h; const float* a1; const float* a2; float* dh; float* da_part; int B, n, d; };
__global__ void __launch_bounds__(256) gat_score_bwd_kernel(const GatScoreBwdArgs g) {
    __shared__ float du[DIGAT_MAX_NODES], dv[DIGAT_MAX_NODES];
    const int n = g.n, d = g.d, b = blockIdx.x, tid = threadIdx.x;
    const float* D = g.ds + (long)b * n * n;
    for (int t = tid; t < 2 * n; t += 256) {
        float s = 0.f;
        if (t < n) { for (int i = 0; i < n; ++i) s += D[i * n + t]; du[t] = s; }
        else { const int i = t - n; for (int j = 0; j < n; ++j) s += D[i * n + j]; dv[i] = s; }
    }
    __syncthreads();
    const float* Hb = g.h + (long)b * n * d;
    float* dHb = g.dh + (long)b * n * d;
    for (int c = tid; c < d; c += 256) {
        const float x1 = g.a1[c], x2 = g.a2[c];
        float p1 = 0.f, p2 = 0.f;
        for (int j = 0; j < n; ++j) {
            const float hv = Hb[(long)j * d + c];
            dHb[(long)j * d + c] += fmaf(du[j], x1, dv[j] * x2);
            p1 = fmaf(du[j], hv, p1);
            p2 = fmaf(dv[j], hv, p2);
        }
        g.da_part[(long)b * 2 * d + c] = p1;
        g.da_part[(long)b * 2 * d + d + c] = p2;
    }
}

// save: h, alpha (before dropout), the scores before leaky_relu / the mask, the attention dropout's keep bytes
struct GatSave { float *h, *alpha, *s_pre; uint8_t* amask; };
static GatSave gat_save_carve(Arena& a, int B, int n, int d) {
    const size_t nn = (size_t)B * n * n;
    return GatSave{a.take<float>((size_t)B * n * d), a.take<float>(nn), a.take<float>(nn), a.take<uint8_t>(nn)};
}
// forward workspace: the two node scores [B,n] each, alpha after dropout, split scratch
struct GatFwdWs { float *s1, *s2, *adrop; void* wsplit; };
static GatFwdWs gat_fwd_carve(Arena& w, int B, int n, int d) {
    const size_t bn = (size_t)B * n;
    return GatFwdWs{w.take<float>(bn), w.take<float>(bn), w.take<float>(bn * n), w.take<char>(wsplit_scratch(d))};
}
// backward workspace: dZ, dh [B,n,d], ds [B,n,n], the rows' [da1 | da2] partials [B,2d], dW scratch, split scratch
struct GatBwdWs { float *dZ, *dh, *ds, *dap; void* wws; size_t wb; void* wsplit; };
static GatBwdWs gat_bwd_carve(Arena& w, int B, int n, int d) {
    const size_t nd = (size_t)B * n * d;
    GatBwdWs o;
    o.dZ = w.take<float>(nd); o.dh = w.take<float>(nd); o.ds = w.take<float>((size_t)B * n * n);
    o.dap = w.take<float>((size_t)B * 2 * d);
    o.wb = digat_linear_bwd_weight_workspace(B * n, d, d);
    o.wws = w.take<char>(o.wb); o.wsplit = w.take<char>(wsplit_scratch(d));
    return o;
}

extern "C" {

size_t digat_gat_train_save_bytes(int B, int n, int d) { Arena a; gat_save_carve(a, B, n, d); return a.used; }
size_t digat_gat_train_workspace_bytes(int B, int n, int d) {          // one buffer serves both directions
    Arena fwd, bwd;
    gat_fwd_carve(fwd, B, n, d); gat_bwd_carve(bwd, B, n, d);
    return larger(fwd, bwd);
}

// X: the layer's input AFTER its input dropout (:495; the residual uses the dropped input, :501); out = relu(drop_p(alpha) h) + X
int digat_gat_fwd_train(const float* X, const uint8_t* A, const float* W, const float* bW, const float* a1, const float* a2, float* out,
                        float p_alpha, uint32_t seed, int B, int n, int d, void* save, size_t save_bytes, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!X || !A || !W || !bW || !a1 || !a2 || !out || !save || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0 || p_alpha < 0.f || p_alpha >= 1.f) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES || gat_agg_route(B, n, d).status) return DIGAT_ERR_SHAPE;      // before any launch
    if (B == 0) return DIGAT_OK;
    Arena sa(save, save_bytes), w(workspace, workspace_bytes);
    const GatSave s = gat_save_carve(sa, B, n, d);
    if (!sa.ok || workspace_bytes < digat_gat_train_workspace_bytes(B, n, d)) return DIGAT_ERR_WORKSPACE;
    const GatFwdWs o = gat_fwd_carve(w, B, n, d);
    hipStream_t st = (hipStream_t)stream;
    const long nodes = (long)B * n;
    T_TRY(t_linear_fwd(X, d, W, bW, s.h, (int)nodes, d, d, o.wsplit, st));
    hipLaunchKernelGGL(gat_node_scores_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, st, (const float*)s.h, a1, a2, o.s1, o.s2, nodes, d / 4);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(gat_alpha_kernel, dim3((unsigned)((nodes + 3) / 4)), dim3(256), 0, st, (const float*)o.s1, (const float*)o.s2, A, s.alpha,
                       s.s_pre, nodes, n);
    DIGAT_CHECK_LAUNCH();
    const float* aggalpha = s.alpha;
    if (p_alpha > 0.f) {
        T_TRY(digat_dropout_fwd(s.alpha, o.adrop, s.amask, (int64_t)B * n * n, p_alpha, seed, stream));
        aggalpha = o.adrop;
    }
    return launch_agg(agg_args(aggalpha, s.h, X, out, B, n, d), gat_agg_route(B, n, d), st);
}

// dX [B,n,d], dW [d,d], dbW [d], da1 da2 [d]: all written (not accumulated)
int digat_gat_bwd(const float* dOut, const float* out, const float* X, const uint8_t* A, const float* W, const float* a1, const float* a2,
                  float p_alpha, const void* save, size_t save_bytes, float* dX, float* dW, float* dbW, float* da1, float* da2,
                  int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dOut || !out || !X || !A || !W || !a1 || !a2 || !save || !dX || !dW || !dbW || !da1 || !da2 || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || n <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (d % 4 || n > DIGAT_MAX_NODES || gat_agg_route(B, n, d).status) return DIGAT_ERR_SHAPE;      // what the forward refuses
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return zero_floats(st, {{dW, (size_t)d * d}, {dbW, (size_t)d}, {da1, (size_t)d}, {da2, (size_t)d}});
    Arena sa(const_cast<void*>(save), save_bytes), w(workspace, workspace_bytes);
    const GatSave s = gat_save_carve(sa, B, n, d);
    if (!sa.ok || workspace_bytes < digat_gat_train_workspace_bytes(B, n, d)) return DIGAT_ERR_WORKSPACE;
    const GatBwdWs o = gat_bwd_carve(w, B, n, d);
    float *dZ = o.dZ, *dh = o.dh, *dap = o.dap;
    const size_t nd = (size_t)B * n * d;
    hipLaunchKernelGGL(relu_res_mask_kernel, dim3(grid_for((long)nd)), dim3(256), 0, st, dOut, out, X, dZ, (long)nd);
    DIGAT_CHECK_LAUNCH();
    const float ascale = p_alpha > 0.f ? 1.f / (1.f - p_alpha) : 1.f;
    const uint8_t* am = p_alpha > 0.f ? s.amask : nullptr;
    T_TRY(launch_aggT(AggTArgs{s.alpha, am, ascale, dZ, dh, B, n, d, (long)d}, st));                 // dh = alpha'^T dZ
    // ds: dalpha' = dZ h^T through (dropout,) softmax, mask, leaky_relu'
    T_TRY(launch_ds(DsArgs{dZ, s.h, s.alpha, s.s_pre, A, am, ascale, o.ds, B, n, d}, st));
    {   // the separable score: dh += du a1 + dv a2; da1, da2 partials
        GatScoreBwdArgs t{o.ds, s.h, a1, a2, dh, dap, B, n, d};
        hipLaunchKernelGGL(gat_score_bwd_kernel, dim3(B), dim3(256), 0, st, t);
        DIGAT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(colsum_kernel, dim3((d + 63) / 64), dim3(256), 0, st, (const float*)dap, (long)2 * d, da1, B, d, 0, (const int*)nullptr, 0);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_kernel, dim3((d + 63) / 64), dim3(256), 0, st, (const float*)(dap + d), (long)2 * d, da2, B, d, 0, (const int*)nullptr, 0);
    DIGAT_CHECK_LAUNCH();
    const int M = B * n;
    if (hipMemcpyAsync(dX, dOut, nd * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return DIGAT_ERR_LAUNCH;      // the residual
    T_TRY(t_linear_bwd_input(dh, W, dX, M, d, d, 1, o.wsplit, st));
    return t_linear_bwd_weight(dh, X, d, dW, dbW, M, d, d, o.wws, o.wb, st);
}

}  // extern "C"
