// digat_sag.inc — semantic-augmented-graph construction (SURVEY §8f-4), construct_SAG.py from embeddings to news graphs:
//   * generate_cos_similarities (:112-162): for every news of a category, the cosine of its title / content embedding with
//     every corpus title / content embedding (four [n, m] matrices), their mean, and torch.topk(k = top_M + 1) of each.
//     The reference loops over the n news, five topk calls each; here the embeddings are row-normalised once, the four
//     matrices are ONE GEMM  [title ; content] x [corpus_title ; corpus_content]^T  on the matrix cores (the bf16x6 kernel
//     above 2048 rows: fp32-grade products), and a selection kernel keeps the k largest of every row.
//   * generate_similariy_info + generate_similar_news_list + aggregate (:217-446) for the kind aggregate reads, the average:
//     behind the same GEMM, sag_lists_kernel selects a title group's k best corpus groups and walks them for every news of
//     the group (skip its own group, keep M' = k - 1), writing the [news_num, top_M] lists the walk below reads.
//   * generate_news_graph (:449-485): breadth-first expansion of every news over its similar-news list; integer work,
//     one thread per news (the walk itself is sequential: <= news_node_num nodes, <= top_M edges each).
// Included at the end of digat_kernels.hip.

// out[r] = x[r] / max(||x[r]||_2, eps)  (F.cosine_similarity normalises each operand before the dot product); rows
// [rows, rows_padded) are written as zeros (GEMM padding).  One wave per row.
__global__ void __launch_bounds__(256) sag_normalize_kernel(const float* x, float* out, long rows, long rows_padded, int dim, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * 4 + wave;
    if (r >= rows_padded) return;
    float* o = out + r * dim;
    if (r >= rows) {
        for (int c = lane; c < dim; c += 64) o[c] = 0.f;
        return;
    }
    const float* v = x + r * dim;
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = fmaf(v[c], v[c], ss);
    ss = wave_sum(ss);
    const float nrm = fmaxf(sqrtf(ss), eps);
    for (int c = lane; c < dim; c += 64) o[c] = v[c] / nrm;
}

struct SagTopkArgs {
    const float* S; long ld;        // [2*nc, ld]: rows [0,nc) title queries, [nc,2nc) content queries; columns [0,mp) corpus titles, [mp,2mp) corpus contents
    int nc, m, mp, k;
    long row0, n;                   // global index of chunk row 0; total news (output stride)
    float* values; int* indices;    // [5][n][k]
};

__device__ __forceinline__ bool sag_better(float v, int j, float w, int i) { return v > w || (v == w && j < i); }

// The K best of a thread's column slice, sorted descending in registers: (v, j) enters when it beats the last one kept.
template <int K>
__device__ __forceinline__ void sag_keep(float (&val)[K], int (&idx)[K], float v, int j) {
    if (v > val[K - 1]) {
        val[K - 1] = v; idx[K - 1] = j;
#pragma unroll
        for (int t = K - 1; t > 0; --t)
            if (val[t] > val[t - 1]) {
                const float fv = val[t]; val[t] = val[t - 1]; val[t - 1] = fv;
                const int fj = idx[t]; idx[t] = idx[t - 1]; idx[t - 1] = fj;
            }
    }
}

// One round of the workgroup arg-max over every thread's best entry (ties: lower column first).  Returns the thread that
// held the winner, which drops it from its list; (v, j) is the winner in every thread.  Two barriers; red_* are [4].
template <int K>
__device__ __forceinline__ int sag_pop_best(float (&val)[K], int (&idx)[K], float* red_v, int* red_j, int* red_t, float& v, int& j) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = tid;
    v = val[0]; j = idx[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float w = __shfl_xor(v, off);
        const int wj = __shfl_xor(j, off), wt = __shfl_xor(t, off);
        if (sag_better(w, wj, v, j)) { v = w; j = wj; t = wt; }
    }
    if (lane == 0) { red_v[wave] = v; red_j[wave] = j; red_t[wave] = t; }
    __syncthreads();
    v = red_v[0]; j = red_j[0]; t = red_t[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (sag_better(red_v[w], red_j[w], v, j)) { v = red_v[w]; j = red_j[w]; t = red_t[w]; }
    __syncthreads();
    if (tid == t) {
#pragma unroll
        for (int s = 0; s < K - 1; ++s) { val[s] = val[s + 1]; idx[s] = idx[s + 1]; }
        val[K - 1] = -INFINITY; idx[K - 1] = 0x7fffffff;
    }
    return t;
}

// One workgroup per (news, kind); kind 0..4 = title-title, content-content, title-content, content-title, mean of the four
// (the order construct_SAG.py:117-162 returns them in).  Every thread keeps the K best of its column slice sorted in
// registers; k rounds of a workgroup arg-max then emit the row's k best in descending order (ties: lower column first).
template <int K>
__global__ void __launch_bounds__(256) sag_topk_kernel(const SagTopkArgs a) {
    __shared__ float red_v[4];
    __shared__ int red_j[4], red_t[4];
    const int i = blockIdx.x, kind = blockIdx.y, tid = threadIdx.x;
    const float* tt = a.S + (long)i * a.ld;
    const float* tc = tt + a.mp;
    const float* ct = a.S + (long)(a.nc + i) * a.ld;
    const float* cc = ct + a.mp;
    const float* single = kind == 0 ? tt : (kind == 1 ? cc : (kind == 2 ? tc : ct));
    float val[K];
    int idx[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { val[t] = -INFINITY; idx[t] = 0x7fffffff; }
    for (int j = tid; j < a.m; j += 256) {
        float v;
        if (kind < 4) v = single[j];
        else v = (((tt[j] + cc[j]) + tc[j]) + ct[j]) * 0.25f;            // :159, (tt + cc + tc + ct) / 4
        sag_keep<K>(val, idx, v, j);
    }
    float* ov = a.values + ((long)kind * a.n + a.row0 + i) * a.k;
    int* oj = a.indices + ((long)kind * a.n + a.row0 + i) * a.k;
    for (int round = 0; round < a.k; ++round) {
        float v;
        int j;
        if (sag_pop_best<K>(val, idx, red_v, red_j, red_t, v, j) == tid) { ov[round] = v; oj[round] = j; }
    }
}

// generate_similar_news_list (:303-320), the average kind, fused behind the selection: one workgroup per query group of the
// chunk.  The k best corpus groups by the mean of the four cosines (sag_topk_kernel's kind 4, same arithmetic and order) stay
// in LDS; thread t then serves members t, t + 256, ... of the group: walk the k entries in order, skip a corpus group that
// holds the news itself, write (first member of the corpus group, cosine) and stop at M' = k - 1 entries (with M' = 0 the stop
// test never fires, as in the reference, and the one entry is written unless skipped).  Every news row has one writer.
struct SagListsArgs {
    const float* S; long ld;        // as SagTopkArgs
    int nc, m, mp, k, top_M;        // top_M: row stride of sim_index / sim_cos
    long row0;                      // query group of chunk row 0
    const int* group_start; const int* group_member;        // CSR over the query groups: news rows
    const int* corpus_start; const int* corpus_member;      // CSR over the corpus groups: news rows, first = representative
    int* sim_index; float* sim_cos; int* sim_len;
};

template <int K>
__global__ void __launch_bounds__(256) sag_lists_kernel(const SagListsArgs a) {
    __shared__ float red_v[4];
    __shared__ int red_j[4], red_t[4];
    __shared__ float win_v[32];
    __shared__ int win_j[32];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* tt = a.S + (long)i * a.ld;
    const float* tc = tt + a.mp;
    const float* ct = a.S + (long)(a.nc + i) * a.ld;
    const float* cc = ct + a.mp;
    float val[K];
    int idx[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { val[t] = -INFINITY; idx[t] = 0x7fffffff; }
    for (int j = tid; j < a.m; j += 256)
        sag_keep<K>(val, idx, (((tt[j] + cc[j]) + tc[j]) + ct[j]) * 0.25f, j);
    for (int round = 0; round < a.k; ++round) {
        float v;
        int j;
        if (sag_pop_best<K>(val, idx, red_v, red_j, red_t, v, j) == tid) { win_v[round] = v; win_j[round] = j; }
    }
    __syncthreads();
    const int stop = a.k - 1;                                                // M' = min(top_M, m - 1)
    const long g = a.row0 + i;
    for (int p = a.group_start[g] + tid; p < a.group_start[g + 1]; p += 256) {
        const int x = a.group_member[p];
        int* oi = a.sim_index + (long)x * a.top_M;
        float* oc = a.sim_cos + (long)x * a.top_M;
        int cnt = 0;
        for (int e = 0; e < a.k; ++e) {
            if ((unsigned)win_j[e] >= (unsigned)a.m) break;                  // fewer than k comparable cosines (NaN embeddings): no such group
            const int cs = a.corpus_start[win_j[e]], ce = a.corpus_start[win_j[e] + 1];
            bool self = false;
            for (int q = cs; q < ce; ++q) self |= a.corpus_member[q] == x;   // :312, news_ID not in corpus_news_IDs
            if (self) continue;
            oi[cnt] = a.corpus_member[cs];
            oc[cnt] = win_v[e];
            if (++cnt == stop) break;                                        // :318
        }
        a.sim_len[x] = cnt;
    }
}

// One thread per news: the breadth-first walk of construct_SAG.py:449-485.  sim_index / sim_cos [news_num, top_M] hold each
// news's similar-news list (corpus news indices, cosines) with sim_len entries.  Outputs are zero-filled before the launch.
#define SAG_MAX_NODES 256
__global__ void __launch_bounds__(64) sag_news_graph_kernel(const int* sim_index, const float* sim_cos, const int* sim_len, long news_num,
                                                            int top_M, int hop, int nn, float threshold,
                                                            int* node_ID, uint8_t* graph, uint8_t* mask, int* overflow) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= news_num) return;
    mask[i * nn] = 1;                                          // :455 (row 0, the padding news, included)
    if (i == 0) return;                                        // :456 range(1, news_num)
    int* ids = node_ID + i * nn;
    uint8_t* g = graph + i * nn * nn;
    uint8_t* mk = mask + i * nn;
    unsigned char depth[SAG_MAX_NODES];
    depth[0] = 0;
    ids[0] = (int)i;
    int head = 0, rear = 1;
    while (head < rear) {
        const int dh = depth[head];
        if (dh == hop) { ++head; continue; }                   // :464-466
        const long cur = ids[head];
        const int len = sim_len[cur];
        for (int e = 0; e < len; ++e) {
            if (dh > 0 && (sim_cos[cur * top_M + e] < threshold || e == top_M - 1)) break;      // :470
            const int nb = sim_index[cur * top_M + e];
            int pos = -1;
            for (int p = 0; p < rear; ++p)
                if (ids[p] == nb) { pos = p; break; }
            if (pos < 0) {
                if (rear >= nn) { *overflow = 1; return; }     // the reference would index past news_node_num here
                ids[rear] = nb; mk[rear] = 1;
                g[head * nn + rear] = 1; g[rear * nn + head] = 1;
                depth[rear] = (unsigned char)(dh + 1);
                ++rear;
            } else {
                g[head * nn + pos] = 1; g[pos * nn + head] = 1;
            }
        }
        ++head;
    }
}

static long sag_pad_corpus(long m) { return (m + 119) / 120 * 120; }       // 2*mp is a multiple of 240: three-strip GEMM tiles
static long sag_chunk_rows(long n) { return n < 4096 ? n : 4096; }

// The cosine matrices of one category, chunk by chunk: normalise the corpus once and split it for the GEMM, then for every
// chunk of <= 4096 query rows normalise [title ; content], run the one GEMM into S [2*nc, 2*mp] and hand S to ``select``
// (S, mp, nc, first row of the chunk), which launches the selection kernel that consumes it.  Workspace as
// digat_sag_cos_topk_workspace_bytes lays it out.
template <class Select>
static int sag_cos_chunks(const float* title, const float* content, long n, const float* corpus_title, const float* corpus_content,
                          long m, int dim, void* workspace, hipStream_t st, Select select) {
    const long mp = sag_pad_corpus(m), nc_max = sag_chunk_rows(n);
    char* ws = (char*)workspace;
    float* Cn = (float*)ws;            ws += align_up((size_t)2 * mp * dim * 4, 256);
    float* Qn = (float*)ws;            ws += align_up((size_t)2 * nc_max * dim * 4, 256);
    void* wsplit = ws;                 ws += align_up(digat_split_weights_bytes((int)(2 * mp), dim), 256);
    float* S = (float*)ws;
    const float eps = 1e-8f;           // torch.nn.CosineSimilarity() default
    hipLaunchKernelGGL(sag_normalize_kernel, dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, st, corpus_title, Cn, (long)m, mp, dim, eps);
    DIGAT_CHECK_LAUNCH();
    hipLaunchKernelGGL(sag_normalize_kernel, dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, st, corpus_content, Cn + mp * dim, (long)m, mp, dim, eps);
    DIGAT_CHECK_LAUNCH();
    int rc = launch_split(Cn, Cn, Cn, (int)(2 * mp), 1, dim, wsplit, st);
    if (rc) return rc;
    for (long r0 = 0; r0 < n; r0 += nc_max) {
        const long nc = n - r0 < nc_max ? n - r0 : nc_max;
        hipLaunchKernelGGL(sag_normalize_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, title + r0 * dim, Qn, nc, nc, dim, eps);
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(sag_normalize_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, content + r0 * dim, Qn + nc * dim, nc, nc, dim, eps);
        DIGAT_CHECK_LAUNCH();
        GemmArgs g = gemm_plain(Qn, dim, Cn, nullptr, S, 2 * mp, (int)(2 * nc), (int)(2 * mp), dim, 0);
        g.wsplit = (const unsigned short*)wsplit;
        rc = launch_gemm(g, st, DIGAT_KERNEL_LINEAR);
        if (rc) return rc;
        select(S, mp, nc, r0);
        DIGAT_CHECK_LAUNCH();
    }
    return DIGAT_OK;
}

extern "C" {

size_t digat_sag_cos_topk_workspace_bytes(int64_t n, int64_t m, int dim) {
    const long mp = sag_pad_corpus(m), nc = sag_chunk_rows(n);
    return align_up((size_t)2 * mp * dim * 4, 256) + align_up((size_t)2 * (nc > 0 ? nc : 1) * dim * 4, 256)
           + align_up(digat_split_weights_bytes((int)(2 * mp), dim), 256) + align_up((size_t)2 * (nc > 0 ? nc : 1) * 2 * mp * 4, 256);
}

int digat_sag_cos_topk(const float* title, const float* content, int64_t n, const float* corpus_title, const float* corpus_content,
                       int64_t m, int dim, int k, float* values, int32_t* indices, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!title || !content || !corpus_title || !corpus_content || !values || !indices || !workspace || n < 0 || m <= 0 || dim <= 0 || k <= 0)
        return DIGAT_ERR_ARG;
    if (k > m || k > 32 || dim % 16 || 2 * sag_pad_corpus(m) > 0x7fffffffL / dim) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < digat_sag_cos_topk_workspace_bytes(n, m, dim)) return DIGAT_ERR_WORKSPACE;
    if (n == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    return sag_cos_chunks(title, content, n, corpus_title, corpus_content, m, dim, workspace, st,
                          [&](const float* S, long mp, long nc, long r0) {
        SagTopkArgs a{S, 2 * mp, (int)nc, (int)m, (int)mp, k, r0, (long)n, values, indices};
        const dim3 grid((unsigned)nc, 5);
        if (k <= 4) hipLaunchKernelGGL(sag_topk_kernel<4>, grid, dim3(256), 0, st, a);
        else if (k <= 8) hipLaunchKernelGGL(sag_topk_kernel<8>, grid, dim3(256), 0, st, a);
        else if (k <= 16) hipLaunchKernelGGL(sag_topk_kernel<16>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(sag_topk_kernel<32>, grid, dim3(256), 0, st, a);
    });
}

size_t digat_sag_similar_lists_workspace_bytes(int64_t n, int64_t m, int dim) { return digat_sag_cos_topk_workspace_bytes(n, m, dim); }

int digat_sag_similar_lists(const float* title, const float* content, int64_t n, const float* corpus_title, const float* corpus_content,
                            int64_t m, int dim, int top_M, const int32_t* group_start, const int32_t* group_member,
                            const int32_t* corpus_start, const int32_t* corpus_member, int32_t* sim_index, float* sim_cos,
                            int32_t* sim_len, int64_t news_num, void* workspace, size_t workspace_bytes, void* stream) {
    if (!title || !content || !corpus_title || !corpus_content || !group_start || !group_member || !corpus_start || !corpus_member
        || !sim_index || !sim_cos || !sim_len || !workspace || n < 0 || m <= 0 || dim <= 0 || top_M <= 0 || news_num <= 0)
        return DIGAT_ERR_ARG;
    const int k = (int)(top_M < m - 1 ? top_M : m - 1) + 1;                       // :292, M' + 1
    if (k > 32 || dim % 16 || 2 * sag_pad_corpus(m) > 0x7fffffffL / dim) return DIGAT_ERR_SHAPE;
    if (workspace_bytes < digat_sag_similar_lists_workspace_bytes(n, m, dim)) return DIGAT_ERR_WORKSPACE;
    if (n == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    return sag_cos_chunks(title, content, n, corpus_title, corpus_content, m, dim, workspace, st,
                          [&](const float* S, long mp, long nc, long r0) {
        SagListsArgs a{S, 2 * mp, (int)nc, (int)m, (int)mp, k, top_M, r0, group_start, group_member, corpus_start, corpus_member,
                       sim_index, sim_cos, sim_len};
        const dim3 grid((unsigned)nc);
        if (k <= 4) hipLaunchKernelGGL(sag_lists_kernel<4>, grid, dim3(256), 0, st, a);
        else if (k <= 8) hipLaunchKernelGGL(sag_lists_kernel<8>, grid, dim3(256), 0, st, a);
        else if (k <= 16) hipLaunchKernelGGL(sag_lists_kernel<16>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(sag_lists_kernel<32>, grid, dim3(256), 0, st, a);
    });
}

int digat_sag_news_graph(const int32_t* sim_index, const float* sim_cos, const int32_t* sim_len, int64_t news_num, int top_M, int hop,
                         int news_node_num, float threshold, int32_t* news_node_ID, uint8_t* news_graph, uint8_t* news_graph_mask,
                         int32_t* overflow, void* stream) {
    if (!sim_index || !sim_cos || !sim_len || !news_node_ID || !news_graph || !news_graph_mask || !overflow || news_num < 0 || top_M <= 0 || hop < 0)
        return DIGAT_ERR_ARG;
    if (news_node_num <= 0 || news_node_num > SAG_MAX_NODES || hop > 255) return DIGAT_ERR_SHAPE;
    if (news_num == 0) return DIGAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t nn = (size_t)news_node_num;
    if (hipMemsetAsync(news_node_ID, 0, (size_t)news_num * nn * 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    if (hipMemsetAsync(news_graph, 0, (size_t)news_num * nn * nn, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    if (hipMemsetAsync(news_graph_mask, 0, (size_t)news_num * nn, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    if (hipMemsetAsync(overflow, 0, 4, st) != hipSuccess) return DIGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(sag_news_graph_kernel, dim3((unsigned)((news_num + 63) / 64)), dim3(64), 0, st, sim_index, sim_cos, sim_len,
                       (long)news_num, top_M, hop, news_node_num, threshold, news_node_ID, news_graph, news_graph_mask, overflow);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
