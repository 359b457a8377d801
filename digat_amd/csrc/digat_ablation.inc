// digat_ablation.inc — device entries of the ablation encoders' scoring pass (graphEncoders._Ablation.inference_grouped):
// the user context on node features that the rows of an impression SHARE, and the assembly of those node features.
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

// What the context kernels index per ROW, written per row from the groups' tensors: row b's group index held inside [0, G) (no
// later read through it can leave the groups' buffers), the group's H category indices and its C1 category-mask bytes.
// B (H + C1 + 1) small elements — 1.6 MB at 4 096 rows, H = 50 — against the B U d floats of node features that are NOT copied.
__global__ void __launch_bounds__(256) group_rows_kernel(const int32_t* __restrict__ row_group, const int64_t* __restrict__ cat_idx,
                                                         const uint8_t* __restrict__ cat_mask, long B, int G, int H, int C1,
                                                         int32_t* __restrict__ rg_out, int64_t* __restrict__ idx_out,
                                                         uint8_t* __restrict__ mask_out) {
    const int per = H + C1 + 1;
    for (long b = blockIdx.x; b < B; b += gridDim.x) {
        const int g = min(max(row_group[b], 0), G - 1);
        for (int r = threadIdx.x; r < per; r += 256) {
            if (r < H) idx_out[b * H + r] = cat_idx[(long)g * H + r];
            else if (r < H + C1) mask_out[b * C1 + (r - H)] = cat_mask[(long)g * C1 + (r - H)];
            else rg_out[b] = g;
        }
    }
}

// Xu[r] = [user_news_embedding[src] (H rows) | topic_node_embedding (C rows)] with src = r (row_group == NULL: one graph per
// group) or row_group[r] held inside [0, G) (one graph per ROW, written expanded: no [G,U,d] intermediate, no index_select).
// One workgroup per graph and grid stride; rows are d4 float4: 16-byte loads and stores on aligned addresses.
__global__ void __launch_bounds__(256) user_nodes_grouped_kernel(const float4* __restrict__ ue, const float4* __restrict__ topic,
                                                                 const int32_t* __restrict__ row_group, float4* __restrict__ Xu,
                                                                 long rows, long G, int H, int C, int d4) {
    const int hist = H * d4, per_row = (H + C) * d4;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long src = row_group ? min(max((long)row_group[r], 0L), G - 1) : r;
        const float4* in = ue + src * hist;
        float4* out = Xu + r * per_row;
        for (int i = threadIdx.x; i < per_row; i += 256) out[i] = i < hist ? in[i] : topic[i - hist];
    }
}

struct UserCtxGroupedWs { UserCtxWs ctx; int32_t* rg; int64_t* idx; uint8_t* mask; };
static UserCtxGroupedWs user_ctx_grouped_carve(Arena& a, int B, int H, int C1, int d) {
    UserCtxGroupedWs w;
    w.ctx = user_ctx_carve(a, B, C1, d);
    w.rg = a.take<int32_t>((size_t)B);
    w.idx = a.take<int64_t>((size_t)B * H);
    w.mask = a.take<uint8_t>((size_t)B * C1);
    return w;
}

extern "C" size_t digat_user_ctx_grouped_workspace_bytes(int B, int G, int U, int H, int C1, int d) {
    (void)G; (void)U;
    if (B < 0 || H < 0 || C1 < 0 || d < 0) return 0;
    Arena a;
    user_ctx_grouped_carve(a, B, H, C1, d);
    return a.used;
}

extern "C" int digat_user_ctx_fwd_grouped(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const int32_t* row_group,
                                          const float* c_n, const float* Ku, const float* Qu, const float* bQu, const float* Fa,
                                          const float* bFa, const float* Kua, const float* Qua, const float* bQua, const float* addend,
                                          float* out, int B, int G, int U, int H, int C1, int d, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    if (!Xu || !cat_mask || !cat_idx || !c_n || !Ku || !Qu || !Fa || !Kua || !Qua || !out || !workspace) return DIGAT_ERR_ARG;
    if (B < 0 || H < 0 || U < H || C1 <= 0 || d <= 0) return DIGAT_ERR_ARG;
    if (B > 0 && (!row_group || G <= 0)) return DIGAT_ERR_ARG;
    if (d % 4 || C1 > DIGAT_MAX_NODES || H > TOPIC_MAX_H) return DIGAT_ERR_SHAPE;
    Arena ar(workspace, workspace_bytes);
    const UserCtxGroupedWs w = user_ctx_grouped_carve(ar, B, H, C1, d);
    if (!ar.ok) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope prof(DIGAT_KERNEL_GLUE, (double)B * (8.0 * H + C1 + 4.0) * 2, st);
        hipLaunchKernelGGL(group_rows_kernel, dim3((unsigned)(B < 2048 ? B : 2048)), dim3(256), 0, st, row_group, cat_idx, cat_mask, (long)B, G,
                           H, C1, w.rg, w.idx, w.mask);
        DIGAT_CHECK_LAUNCH();
    }
    // the launches of digat_user_ctx_fwd, argument for argument: only the topic pooling's node base moves (TopicArgs.group)
    return user_ctx_run(Xu, w.mask, w.idx, w.rg, c_n, Ku, Qu, bQu, Fa, bFa, Kua, Qua, bQua, addend, out, B, U, H, C1, d, w.ctx, st);
}

extern "C" int digat_user_nodes_build(const float* ue, const float* topic, const int32_t* row_group, float* Xu, long rows, long G, int H,
                                      int C, int d, void* stream) {
    if (rows < 0 || G < 0 || H < 0 || C < 0 || d <= 0) return DIGAT_ERR_ARG;
    if (rows == 0) return DIGAT_OK;
    if (!Xu || (H > 0 && !ue) || (C > 0 && !topic) || G == 0 || (!row_group && rows != G)) return DIGAT_ERR_ARG;
    if (d % 4 || H + C <= 0 || H + C > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    if ((((uintptr_t)ue | (uintptr_t)topic | (uintptr_t)Xu) & 15) != 0) return DIGAT_ERR_ARG;        // float4 rows
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(DIGAT_KERNEL_GLUE, (double)rows * (H + C) * d * 8.0, st);
    // a graph is (H + C) d / 4 float4 — 26 per thread at U = 67, d = 400; 8 workgroups per CU keep the stores of all 256 CUs in flight
    hipLaunchKernelGGL(user_nodes_grouped_kernel, dim3((unsigned)(rows < 2048 ? rows : 2048)), dim3(256), 0, st, (const float4*)ue,
                       (const float4*)topic, row_group, (float4*)Xu, rows, G, H, C, d / 4);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
