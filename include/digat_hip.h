/*
 * digat_hip.h — C ABI of the MI355X (gfx950) DIGAT dual-graph interaction hot path.
 *
 * The reference (Veason-silverbullet/DIGAT) has no FFI: its boundary for this path is the Python
 * class contract of graphEncoders.DIGAT (graphEncoders.py:48-198), selected by
 * `--graph_encoder=DIGAT` (model.py:18-19).  This header is the boundary a native implementation
 * of that class binds to; every entry point names the reference function it replaces.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to contiguous row-major data, 16-byte aligned;
 *     fp32 unless stated; adjacency / masks are one byte per element (torch.bool), 0 = absent;
 *     category indices are int64 (MIND_corpus.py:149);
 *   - nn.Linear weights are [out, in] exactly as in the reference's state_dict;
 *   - d (news_embedding_dim) must be a multiple of 4; graph sizes n <= DIGAT_MAX_NODES;
 *   - asynchronous on `stream` (a hipStream_t passed as void*), no allocation, no host sync:
 *     scratch comes from the caller (`workspace`, size from the matching *_workspace_bytes);
 *   - inputs are never written; outputs may alias the `addend` argument where one exists;
 *   - returns DIGAT_OK (0) or a DIGAT_ERR_* code, never throws.  Eval-mode semantics
 *     (dropout = identity), i.e. what DIGAT.inference / model.eval() computes;
 *   - threading: calls on DIFFERENT streams may be in flight together — from one host thread or several — as long as each stream
 *     has its own workspace and is driven by one thread at a time (digat_amd.util.score_rows alternates three).  Everything a
 *     call's behaviour depends on travels WITH the call (digat_params.flags: Eq. 8 variant, operand format, side stream, live-row
 *     lists); the library keeps no mutable process-wide switch.  Per-caller-stream side streams live in a mutex-guarded table.
 *     Exceptions, both diagnostics: the launch profiler (digat_profile_*: one measuring thread) and digat_set_train_precision
 *     (set once per training run).
 *   - no environment variable changes what the library computes or which kernels it runs.  The development knobs of earlier
 *     rounds (A/B switches, the wrong-result timing ablations, the LDS-staged Eq. 8 variants) are gone from the sources: their
 *     measurements are in docs/REJECTED.md, their code in git history.  Phase timers are compile-time options
 *     (-DDIGAT_GEMM_TIMERS, -DDIGAT_SPARSE_TIMERS, -DDIGAT_CF_TIMERS through tools/exp/build_variant.sh).
 */
#ifndef DIGAT_HIP_H
#define DIGAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 6): digat_xattn_fwd_train / digat_xattn_bwd / digat_user_ctx_fwd_train / digat_user_ctx_bwd take a ready-made split image
 * (or NULL) before `stream`; the Eq. 8 pair takes the layer's input dropout (p_in, seed_in).  3: digat_params grew featureAffine_fsplit; digat_news_ctx_bwd / digat_user_ctx_bwd took
 * `accumulate_params` in round 5 and entry points were added without a bump: a loader built for one version must refuse a library
 * of another (digat_amd/_lib.py does) rather than shift arguments. */
#define DIGAT_ABI_VERSION 4
#define DIGAT_MAX_NODES 128
#define DIGAT_MAX_DEPTH 16

enum {
    DIGAT_OK = 0,
    DIGAT_ERR_ARG = 1,        /* null pointer / negative size */
    DIGAT_ERR_SHAPE = 2,      /* d % 4 != 0, n > DIGAT_MAX_NODES, depth > DIGAT_MAX_DEPTH ... */
    DIGAT_ERR_WORKSPACE = 3,  /* workspace too small */
    DIGAT_ERR_LAUNCH = 4      /* the HIP runtime refused a launch */
};

int digat_version(void);
const char* digat_error_string(int code);

/* ---- nn.Linear on the matrix cores: y[M,N] = x[M,K] @ w[N,K]^T + b[N]  (b may be NULL) --------
 * Replaces the aten::addmm / mm calls of graphEncoders.py:146-149,166-169 (exact fp32:
 * v_mfma_f32_16x16x4_f32).  ldx / ldy are row strides in floats. */
int digat_linear_f32(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                     int M, int N, int K, void* stream);

/* The same product on the bf16 / fp16 matrix cores: every fp32 operand is split exactly into three bf16
 * pieces and the six significant partial products are summed in the fp32 accumulator (format DIGAT_GEMM_BF16X6), or into
 * two scaled fp16 pieces with three products (DIGAT_GEMM_F16X3; range and accuracy: see the enum below).  `wsplit`
 * (digat_split_weights_bytes(N, K) bytes, enough for either format) receives the split weights as ready-made LDS images
 * in the format the caller names; the library remembers the format of every image it has split (by address) until
 * digat_forget_split_image(wsplit) — call it before the buffer is freed or reused for anything else — and refuses a launch
 * that names the other one (DIGAT_ERR_ARG).  N % 80 == 0, K % 8 == 0; any M (from 2048 rows up the strip-mined tiled kernel,
 * below the split-image [B,d] kernel — same split operands, same accuracy). */
size_t digat_split_weights_bytes(int rows, int K);
int digat_forget_split_image(const void* wsplit);      /* 0 = forgotten, DIGAT_ERR_ARG = not an image the library knows */
int digat_split_proj_weights(const float* W, const float* F1, const float* F2, int d, void* wsplit, int format, void* stream);
int digat_split_weights(const float* W, int N, int K, void* wsplit, int format, void* stream);    /* one [N,K] matrix */
int digat_linear_f32x3(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                       int M, int N, int K, void* wsplit, int format, void* stream);
/* The same with what the encoder's row-list launches add (M >= 2048 or m_dispatch >= 2048: the strip-mined kernel).  w1 non-NULL:
 * a second segment y1 = x w1^T + b1 (wsplit holds both: digat_split_weights_bytes(2 nseg, K)); rowidx / nrows_dev (device): only
 * rows rowidx[0 .. *nrows_dev) of x / y are processed; e0 non-NULL: y = relu(.) + e0; radd non-NULL (needs w1): y1 += radd[row /
 * rows_per_b]; m_dispatch != 0: choose the kernel as if M were this; ragged: 0, or 1 / 2 to ask for ragged 240-column tiles where
 * N is no multiple of 240 (1: full-width tiles dispatched first, 2: row-tile-major) — the results do not depend on it, bit for bit. */
int digat_linear_rows_f32x3(const float* x, int64_t ldx, const float* w0, const float* w1, const float* b0, const float* b1,
                            float* y0, float* y1, int64_t ldy, int M, int nseg, int K, void* wsplit, int format,
                            const int* rowidx, const int* nrows_dev, const float* e0, int64_t lde0,
                            const float* radd, int rows_per_b, int m_dispatch, int ragged, void* stream);
/* Any GEMM launch of the library, for the tests that hold each kernel alone to an fp64 product: `args` is a GemmArgs
 * (digat_amd/csrc/digat_gemm_plan.h), args_bytes its size (anything else: DIGAT_ERR_ARG, a mirror of the struct has drifted); kind:
 * DIGAT_KERNEL_PROJ or DIGAT_KERNEL_LINEAR.  wsplit_scratch non-NULL (digat_split_weights_bytes_format(nsegs nseg, K, format) bytes):
 * the weight segments are split into it in args->format and the launch reads that image; NULL: args->wsplit as given.
 * *kernel_out receives the GemmKernel the launch plan chose, for refused launches too.  Returns the launch's status. */
int digat_gemm_launch(const void* args, size_t args_bytes, int kind, void* wsplit_scratch, int* kernel_out, void* stream);

/* ---- a1 / a2: DIGAT.compute_news_graph_embeddings / compute_user_graph_embeddings -------------
 * graphEncoders.py:143-154 / :163-174 (Eq. 8).  X [B,n,d], A [B,n,n] bytes, ctx [B,d] (the OTHER
 * graph's context); W [d,d]+bW, F1 (ffn1, neighbour j), F2 (ffn2, centre i), F3 [d,d]+b3, a [d]
 * (the [1,d] weight of *_graph_attention_a).  out [B,n,d] = relu(alpha @ h) + X.
 * alpha_out [B,n,n] is optional (NULL to skip). */
size_t digat_xattn_workspace_bytes(int B, int n, int d);
int digat_xattn_fwd(const float* X, const uint8_t* A, const float* ctx,
                    const float* W, const float* bW, const float* F1, const float* F2,
                    const float* F3, const float* b3, const float* a,
                    float* out, float* alpha_out, int B, int n, int d,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same without alpha_out and with the Eq. 8 variant named (DIGAT_XATTN_DENSE or DIGAT_XATTN_SPARSE, below): the sparse
 * kernel visits only the adjacency entries (graphs with a few entries per node; n > 16, d <= 1024), results equal to
 * fp32 summation order. */
int digat_xattn_fwd_mode(const float* X, const uint8_t* A, const float* ctx,
                         const float* W, const float* bW, const float* F1, const float* F2,
                         const float* F3, const float* b3, const float* a,
                         float* out, int B, int n, int d, int mode,
                         void* workspace, size_t workspace_bytes, void* stream);

/* One Eq. 8 layer on the reduced-precision operand path of BASELINE configs[4], directly callable (tests, micro-benchmarks):
 * the projection GEMM on the split image `wsplit` (digat_split_proj_weights(W, F1, F2, d, wsplit, format, ...)) stores P' = K3 + K1
 * and Q = K2 as bf16 (pq = 1, DIGAT_PQ_BF16) or as block-scaled e4m3 rows (pq = 2, DIGAT_PQ_FP8: the layout documented there),
 * pq = 0: fp32; the sparse Eq. 8 kernel reads them.  Needs B n >= 2048, n > 16, d % 80 == 0, d <= 1024 (DIGAT_ERR_SHAPE otherwise);
 * workspace as digat_xattn_fwd.  (graphEncoders.py:143-154 / :163-174; README.md:62-66) */
int digat_xattn_fwd_lowprec(const float* X, const uint8_t* A, const float* ctx,
                            const float* W, const float* bW, const float* F1, const float* F2,
                            const float* F3, const float* b3, const float* a, const void* wsplit, int format,
                            float* out, int B, int n, int d, int pq,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The Eq. 8 pairwise part alone, on already-projected inputs: h = X W^T + bW, Q = X F2^T and
 * Pr = (ctx F3^T + b3) + X F1^T, i.e. K3 + K1 already summed in the reference's left-to-right order:
 * score -> leaky_relu(0.2) -> -1e9 mask -> softmax_j (written to alpha [B,n,n], required)
 * -> out = relu(alpha @ h) + X.  Two launches: the score kernel bench.py prices against the HBM
 * roofline, and the aggregation on the matrix cores. */
int digat_xattn_pairwise_fwd(const float* Pr, const float* Q, const float* h, const float* X,
                             const float* a, const uint8_t* A,
                             float* out, float* alpha, int B, int n, int d, void* stream);

/* ---- a3: DIGAT.compute_news_graph_context  (graphEncoders.py:109-114, layers.py:199-206) ------
 * X [B,N,d], mask [B,N] bytes; Kc/Qc/bQc = candidate_attention.{K.weight,Q.weight,Q.bias},
 * Wg [d,2d]/bg = news_graph_W.  out [B,d] = addend + context (addend may be NULL or == out). */
size_t digat_news_ctx_workspace_bytes(int B, int N, int d);
int digat_news_ctx_fwd(const float* X, const uint8_t* mask,
                       const float* Kc, const float* Qc, const float* bQc,
                       const float* Wg, const float* bg,
                       const float* addend, float* out, int B, int N, int d,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- a4 (+a7): DIGAT.compute_user_graph_context  (graphEncoders.py:123-134) -------------------
 * Xu [B,U,d] (first H nodes = history), cat_mask [B,C1] bytes, cat_idx [B,H] int64 in [0,C1),
 * c_n [B,d].  C1 = category_num + 1.  Contains the torch_scatter scatter_softmax / scatter_sum
 * replacement (topic pooling).  out [B,d] = addend + context. */
size_t digat_user_ctx_workspace_bytes(int B, int U, int H, int C1, int d);
int digat_user_ctx_fwd(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n,
                       const float* Ku, const float* Qu, const float* bQu,
                       const float* Fa, const float* bFa,
                       const float* Kua, const float* Qua, const float* bQua,
                       const float* addend, float* out, int B, int U, int H, int C1, int d,
                       void* workspace, size_t workspace_bytes, void* stream);

/* digat_user_ctx_fwd for rows that SHARE node features (the ablation encoders' scoring pass: the user graph of an impression does
 * not depend on the candidate there, graphEncoders._Ablation.inference_grouped).  Xu [G,U,d], cat_mask [G,C1] and cat_idx [G,H]
 * are given per GROUP; row_group [B] int32 maps each row to its group (any mapping with values in [0, G): not only ascending
 * runs; a value outside is held inside, so that no read leaves the groups' buffers); c_n, addend and out are [B,d] per row.
 * Bit-identical to digat_user_ctx_fwd on the expanded tensors: the [B,d] query chain, the featureAffine GEMM and the SDPA pooling
 * are the same launches on the same rows, the topic pooling reads row b's nodes at Xu + row_group[b] U d.  No [B,U,d] copy of the
 * node features is made (the workspace holds per-row copies of the category indices and mask bytes: B (8 H + C1 + 4) bytes).
 * addend may be NULL or == out.  B == 0 returns without a launch.  Errors as digat_user_ctx_fwd, and DIGAT_ERR_ARG for a null
 * row_group or G <= 0 with B > 0.  No allocation, no host synchronisation. */
size_t digat_user_ctx_grouped_workspace_bytes(int B, int G, int U, int H, int C1, int d);
int digat_user_ctx_fwd_grouped(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const int32_t* row_group,
                               const float* c_n,
                               const float* Ku, const float* Qu, const float* bQu,
                               const float* Fa, const float* bFa,
                               const float* Kua, const float* Qua, const float* bQua,
                               const float* addend, float* out, int B, int G, int U, int H, int C1, int d,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The INITIAL user context of an encoder pass alone (round 8): c_u = compute_user_graph_context on the INPUT history rows, as the
 * GEMM F x = ue Fa^T followed by one launch (user_ctx0_kernel) — featureAffine is linear and a present category's pooling weights
 * sum to one, so it is applied to the few history rows in front of the pooling instead of to the B C1 pooled rows behind it; the
 * pooled topics never reach memory.  ue [G,H,d] with row_group [B] int32 (row b reads group row_group[b]; values must lie in
 * [0, G)), or [B,H,d] with row_group == NULL (G is ignored).  kq_topic, kq_user [B,d]: the two folded queries K^T (Q c_n + bQ);
 * cat_mask [B,C1], cat_idx [B,H] per row; Fa [d,d], bFa [d]; fa_wsplit: digat_split_weights(Fa, d, d, ., format) output in
 * `format` (DIGAT_GEMM_BF16X6 / _F16X3), or NULL for the exact fp32 product; addend NULL, [B,d] or == out; out [B,d].
 * scratch: rows H d floats (rows = G or B), wholly written before it is read.  A row of the result has the same bits in a grouped
 * and a per-row call and at every B and G.  Shapes: H in [1,64], d % 4 == 0, d <= 1024, C1 <= 64, H <= 52 or d <= 512, and
 * (C1 d + ...) 4 bytes of LDS within 64 KB (DIGAT_ERR_SHAPE otherwise: digat_user_ctx_fwd serves those).  B == 0 returns
 * without a launch.  No allocation, no host synchronisation. */
int digat_user_ctx0_fwd(const float* ue, const int32_t* row_group, int G, const float* kq_topic, const float* kq_user,
                        const uint8_t* cat_mask, const int64_t* cat_idx, const float* Fa, const float* bFa,
                        const void* fa_wsplit, int format, const float* addend, float* out, int B, int H, int C1, int d,
                        void* scratch, size_t scratch_bytes, void* stream);

/* The user graph's node features Xu = [user_news_embedding (H rows) | topic_node_embedding (C rows)] (graphEncoders.py:191) in one
 * launch: ue [G,H,d], topic [C,d].  row_group == NULL: Xu [G,U,d], one graph per group (rows must equal G).  row_group [rows]
 * int32: Xu [rows,U,d], graph r built from group row_group[r] (held inside [0, G)) — the expanded tensor written directly.
 * d % 4 == 0 and 16-byte-aligned pointers (DIGAT_ERR_SHAPE / DIGAT_ERR_ARG otherwise); rows == 0 returns without a launch. */
int digat_user_nodes_build(const float* ue, const float* topic, const int32_t* row_group, float* Xu, long rows, long G, int H,
                           int C, int d, void* stream);

/* topic pooling alone: out [B,C1,d] = scatter_sum(scatter_softmax(a) * hist) with
 * a_t = hist_t . kq / sqrt(d); kq [B,d] = (c_n Qu^T + bQu) Ku.  (graphEncoders.py:126-130) */
int digat_topic_pool_fwd(const float* Xu, const float* kq, const int64_t* cat_idx, float* out,
                         int B, int U, int H, int C1, int d, void* stream);

/* The inference launchers of the context stage alone, for tests that hold one kernel at a time to a reference: arguments are
 * checked and forwarded one for one.  No workspace, no allocation, no host synchronisation; B == 0 returns without a launch.
 *
 * digat_pool_fwd: ScaledDotProductAttention pooling on a folded query (layers.py:199-206 with (K x).q = x.(K^T q)) through the
 * dispatch inference takes — the register-resident kernels up to n = 68, d = 512, the two-pass kernel beyond (digat_attn_pool_fwd
 * always runs the latter).  feat: row b's n nodes at feat + b ld_b, d floats apart (ld_b % 4 == 0); kq [B,d]; mask [B,n] bytes;
 * addend NULL or [B,d]; out [B,d].  A masked node weighs exactly 0 and its row is not read into any sum, unless every node of the
 * row is masked (uniform weights).  n <= DIGAT_MAX_NODES, d % 4 == 0 (DIGAT_ERR_SHAPE).
 *
 * digat_topic_pool_lists_fwd: digat_topic_pool_fwd with what only the encoder passes.  Xu: row b's H history rows at
 * Xu + (row_group ? row_group[b] : b) ld_b; row_group NULL or [B] int32; live NULL or [B, live_ld] bytes (live_ld >= H): history
 * row t with live[b live_ld + t] == 0 is taken as a zero row, whatever bits it holds; hlast NULL or [B] int32, with live only
 * (DIGAT_ERR_ARG otherwise): every history row t >= hlast[b] is dead and is not requested.  cat_idx [B,H] per row; out [B,C1,d].
 *
 * digat_user_ctx_fused_fwd: compute_user_graph_context as the one launch of the folded inference path (digat_params.
 * featureAffine_fsplit), from the two folded queries kq_topic, kq_user [B,d].  image: digat_split_ctx_fused_weights(Fa, d, ...);
 * bFa [d]; cat_mask [B,C1]; range_flag NULL or one device word (see digat_params.range_flag); the rest as above.
 * DIGAT_ERR_SHAPE outside 1 <= H <= 52, C1 <= 20, 192 < d <= 448, d % 8 == 0. */
int digat_pool_fwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, const float* addend, float* out,
                   int B, int n, int d, void* stream);
int digat_topic_pool_lists_fwd(const float* Xu, int64_t ld_b, const float* kq, const int64_t* cat_idx, const int32_t* row_group,
                               const uint8_t* live, int live_ld, const int32_t* hlast, float* out,
                               int B, int H, int C1, int d, void* stream);
int digat_user_ctx_fused_fwd(const float* Xu, int64_t ld_b, const int32_t* row_group, const uint8_t* live, int live_ld,
                             const int32_t* hlast, const float* kq_topic, const float* kq_user, const int64_t* cat_idx,
                             const uint8_t* cat_mask, const float* addend, float* out, const void* image, const float* bFa,
                             uint32_t* range_flag, int B, int H, int C1, int d, void* stream);

/* ---- a5: DIGAT.forward / DIGAT.inference  (graphEncoders.py:177-198) ---------------------------
 * Parameter block: the reference's state_dict tensors by name (prefix graph_encoder. in Model). */
/* Eq. 8 of the USER graph inside the encoder entry points (digat_params.flags, bits 0-1).  MIND user graphs hold ~4 entries
 * per adjacency row; xattn_sparse_kernel visits only those (score, softmax and aggregation in one launch), the dense pair
 * (tile score kernel + MFMA aggregation) streams whole rows.  AUTO: both are launched and a device-side count of the
 * adjacency entries (<= 20 per node on average: sparse) lets one of them return at its first instruction — no host
 * synchronisation; results differ between the two only by fp32 summation order.  Callers that know their graphs choose. */
enum { DIGAT_XATTN_AUTO = 0, DIGAT_XATTN_DENSE = 1, DIGAT_XATTN_SPARSE = 2 };
/* digat_params.flags bit 2 (folded inference path, bf16x6 projections only): the P and Q projections of Eq. 8 — which only
 * feed the attention score — with the three leading bf16 products (hi*hi, mid*hi, hi*mid: relative error ~2^-16) instead
 * of six (~2^-24); h, which carries the values, keeps six.  A third fewer matrix instructions in the projection GEMM. */
enum { DIGAT_PROJ_PQ_X3 = 4 };
/* digat_params.flags bit 3: the NEWS graph's Eq. 8 with the sparse kernel too (news graphs of more than 16 nodes; smaller
 * ones always take the wave-per-centre small-graph kernel).  SAG news graphs are breadth-first trees plus a few cross
 * edges: 3-4 entries per node at N = 26 or 65. */
enum { DIGAT_NEWS_XATTN_SPARSE = 8 };
/* digat_params.flags bit 4 (BASELINE configs[4]; folded inference path, bf16x6 projections, sparse Eq. 8: the user graph's
 * layers >= 1 — the launches that carry most of the bytes — and news graphs of more than 16 nodes at every layer): the
 * projection GEMM stores P' = K3 + K1 and Q = K2 in bf16
 * (round to nearest even) and the Eq. 8 kernel reads them as such; the score is still accumulated in fp32, h (the values), X
 * and every output stay fp32.  This is the reference's own "faster inference" idea — a quantised K3 + K1 + K2
 * (README.md:62-66).  Ranking metrics move by < 1e-4 (tests/test_hip_lowprec.py); element-wise the contexts move by ~1e-4.
 * Bit 5: the P and Q segments with the leading bf16 product alone (2^-8 per product) instead of the number bit 2 selects. */
enum { DIGAT_PQ_BF16 = 16, DIGAT_PQ_X1 = 32 };
/* digat_params.flags bit 8 (BASELINE configs[4], "fp8 Eq.-8 inference path"; same launches as bit 4, which wins when both are
 * set): the projection GEMM stores P' = K3 + K1 and Q = K2 as BLOCK-SCALED OCP e4m3 (v_cvt_pk_fp8_f32) — one block per (row,
 * 80-column strip of the GEMM's wave tile), scale = the block's absmax / 448 as fp32, laid out per row as
 * [d codes | d / 80 scales | pad to 64 bytes] (d = 400: 448 bytes instead of 1 600) — and the Eq. 8 kernel reads 8-code pieces,
 * rescales in registers (one fma per channel: p s_p + q) and accumulates the score in fp32; h, X and every output stay fp32.
 * Requires d % 80 == 0.  Measured drift of AUC / MRR / nDCG on the trained reference-pinned dev set: tests/test_hip_lowprec.py. */
enum { DIGAT_PQ_FP8 = 256 };
/* digat_params.flags bit 6: every wsplit image of this parameter block (layers' [W|ffn1|ffn2], featureAffine) was split with
 * format DIGAT_GEMM_F16X3 (two scaled fp16 pieces, three products); clear = DIGAT_GEMM_BF16X6.  See digat_split_proj_weights. */
enum { DIGAT_PARAMS_GEMM_F16X3 = 64 };
/* digat_params.flags bit 7: which kernel runs the [B,d] linears of the folded inference path (context queries, candidate query, K3 of the
 * news graph) and digat_news_context_queries' table — set: the tiled split-operand kernel (right for passes of >= 2 048 rows), clear:
 * the split-image [B,d] kernel (right below that).  The CALLER names it, the row count does not choose: a row's bits then do not
 * depend on the batch it sits in, nor on whether its queries were computed in the batch or read from the per-news table. */
enum { DIGAT_PARAMS_BD_TILED = 128 };

typedef struct digat_layer_params {
    const float *W, *bW;      /* {g}_graph_attention_W.i.{weight,bias}    */
    const float *F1;          /* {g}_graph_attention_ffn1.i.weight        */
    const float *F2;          /* {g}_graph_attention_ffn2.i.weight        */
    const float *F3, *b3;     /* {g}_graph_attention_ffn3.i.{weight,bias} */
    const float *a;           /* {g}_graph_attention_a.i.weight  [1,d]    */
    const void  *wsplit;      /* optional: [W|ffn1|ffn2] pre-split by digat_split_proj_weights (opaque: the
                                 three bf16 pieces of every weight, arranged as LDS images per 80-row strip and
                                 32-deep K tile; digat_split_weights_bytes(3d, d) bytes).  Non-NULL runs the
                                 node projections as six bf16 MFMA products per fp32 product ("bf16x6":
                                 fp32-equivalent accuracy, 6/16 of the fp32-MFMA cost); NULL = fp32 MFMA. */
    const void  *f3_wsplit;   /* optional: ffn3.weight split by digat_split_weights(F3, d, d, ...) in the block's format: K3 = ctx F3^T + b3
                                 ([B,d] rows) then runs on the split image too (news graph; the user graph's F3 travels inside
                                 digat_params.ctx_wsplit).  NULL = fp32 MFMA */
} digat_layer_params;

typedef struct digat_params {
    int32_t d;                /* news_embedding_dim                        */
    int32_t depth;            /* graph_depth                               */
    int32_t category_num;     /* C (topic_node_embedding rows)             */
    int32_t flags;            /* bits 0-1: Eq. 8 of the user graph, DIGAT_XATTN_AUTO / _DENSE / _SPARSE; bit 2: DIGAT_PROJ_PQ_X3; bit 3: DIGAT_NEWS_XATTN_SPARSE (see below) */
    const float *topic_node_embedding;                      /* [C,d]        */
    const float *cand_K, *cand_Q, *cand_bQ;                 /* candidate_attention */
    const float *news_graph_W, *news_graph_b;               /* [d,2d], [d]  */
    const float *user_news_K, *user_news_Q, *user_news_bQ;
    const float *featureAffine_W, *featureAffine_b;
    const float *userAtt_K, *userAtt_Q, *userAtt_bQ;        /* userAttention */
    digat_layer_params news[DIGAT_MAX_DEPTH];
    digat_layer_params user[DIGAT_MAX_DEPTH];
    /* Optional (all three pairs or none; NULL = unfolded path): attention queries with the key
     * projection folded in by digat_fold_attention — Wf = K^T Q [d,d], bf = K^T bQ [d] — for
     * candidate_attention, user_news_{K,Q} and userAttention.  Weight-only preprocessing, valid
     * while the weights do not change (inference). */
    const float *cand_fold_W, *cand_fold_b;
    const float *user_news_fold_W, *user_news_fold_b;
    const float *userAtt_fold_W, *userAtt_fold_b;
    const void  *featureAffine_wsplit;   /* optional: featureAffine.weight split by digat_split_weights (same format as the layers') */
    /* Optional split images (the block's format) of the [B,d] linears of the folded inference path; NULL = fp32 MFMA for that one:
     * cand_fold_wsplit: cand_fold_W [d,d]; gate_wsplit: news_graph_W [d,2d];
     * ctx_wsplit[l], l = 0 .. depth: the three matrices applied to the news context before layer l, stacked
     * [user_news_fold_W ; userAtt_fold_W ; user[l].F3] (3d rows; the last entry, l = depth, has no F3: 2d rows are read),
     * each made by digat_split_proj_weights(user_news_fold_W, userAtt_fold_W, user[l].F3, d, ...). */
    const void  *cand_fold_wsplit, *gate_wsplit;
    const void  *ctx_wsplit[DIGAT_MAX_DEPTH + 1];
    uint32_t    *range_flag;             /* optional, DIGAT_PARAMS_GEMM_F16X3 only: one device word the fp16x3 GEMMs OR 1 into when an
                                            activation is at or beyond the format's range (|x| >= 4094 or inf; a NaN input does not raise it — it reaches the outputs as NaN, as in
                                            the reference): the caller zeroes it
                                            before a scoring run and reads it after (digat_amd/util.py re-scores in bf16x6 when set) */
    const void  *featureAffine_fsplit;   /* optional (round 6), DIGAT_PARAMS_GEMM_F16X3 only: featureAffine.weight as the lane-ordered image of
                                            digat_split_ctx_fused_weights — with it (and the folded queries) compute_user_graph_context
                                            (graphEncoders.py:123-134) runs as ONE launch: topic pooling, featureAffine and the SDPA pooling
                                            without T / T' leaving the CU (H <= 52, 192 < d <= 448, C + 1 <= 20; other shapes keep the three launches) */
} digat_params;

/* featureAffine.weight [d,d] -> the fused user-context kernel's image (fp16x3 pieces in the kernel's lane order). */
size_t digat_split_ctx_fused_bytes(int d);
int digat_split_ctx_fused_weights(const float* W, int d, void* image, void* stream);

/* (K x).(Q c + bQ) = x.(Wf c + bf): fold one ScaledDotProductAttention / user_news pair.
 * K, Q [d,d] nn.Linear weights, bQ [d] or NULL; outputs Wf [d,d] (as an nn.Linear weight), bf [d]. */
size_t digat_fold_workspace_bytes(int d);
int digat_fold_attention(const float* K, const float* Q, const float* bQ, float* Wf, float* bf, int d,
                         void* workspace, size_t workspace_bytes, void* stream);

/* news_graph_embeddings [B,N,d], news_graph [B,N,N], news_graph_mask [B,N],
 * user_news_embedding [B,H,d], user_graph [B,U,U] (U = H + C), user_category_mask [B,C+1],
 * user_category_indices [B,H] int64, news_graph_context [B,d] or NULL.
 * NULL context = DIGAT.forward in eval mode (c_n0 computed here, :180); non-NULL = DIGAT.inference.
 * Outputs: the 2-tuple (news_graph_context, user_graph_context), each [B,d]. */
size_t digat_encoder_workspace_bytes(int B, int N, int H, int C, int d, int depth);
int digat_encoder_fwd(const digat_params* params,
                      const float* news_graph_embeddings, const uint8_t* news_graph,
                      const uint8_t* news_graph_mask, const float* user_news_embedding,
                      const uint8_t* user_graph, const uint8_t* user_category_mask,
                      const int64_t* user_category_indices, const float* news_graph_context,
                      float* out_news_context, float* out_user_context,
                      int B, int N, int H,
                      void* workspace, size_t workspace_bytes, void* stream);

/* With the folded-query fields set, digat_encoder_fwd / _grouped can run the news-graph kernels of a layer (small: N nodes,
 * [B,d] linears) on an internal side stream — one per caller stream — under the user graph's Eq. 8 and join before the user
 * context is pooled.  digat_params.flags bits 9-10 choose: neither = by pass size (on below 2 048 rows, where those kernels
 * are a few waves of workgroups each; off from 2 048 rows up, where every kernel fills the chip by itself),
 * DIGAT_PARAMS_SIDE_STREAM_OFF = never, DIGAT_PARAMS_SIDE_STREAM_ON = always (right for a driver that keeps a single pass in
 * flight).  Results do not depend on it, bit for bit.
 * Bit 11, DIGAT_PARAMS_NO_LIVE_ROWS: project, score and write EVERY user-graph node in every layer.  Default (clear): nodes that
 * cannot reach an output — history padding slots, topic nodes of unread categories: only their self loop, pooled with weight 0 —
 * are found on the device and skipped (about half of a MIND user graph).  Outputs are bit-identical either way. */
enum { DIGAT_PARAMS_SIDE_STREAM_OFF = 512, DIGAT_PARAMS_SIDE_STREAM_ON = 1024, DIGAT_PARAMS_NO_LIVE_ROWS = 2048 };
/* Bit 12, DIGAT_PARAMS_PROJ_F16F8C (with bit 6 set: every other image of the block is fp16x3): the layers' `wsplit` images
 * ([W|ffn1|ffn2] of both graphs) were split with format DIGAT_GEMM_F16F8C, and every launch that reads one — the grouped, shared
 * and per-row layer-0 projections, every layer's projection GEMM, digat_news_project0 / digat_user_project0 — runs the fp8-
 * correction kernel at any row count.  Not combined with DIGAT_PROJ_PQ_X3, DIGAT_PQ_BF16 or DIGAT_PQ_FP8 (DIGAT_ERR_ARG). */
enum { DIGAT_PARAMS_PROJ_F16F8C = 4096 };
/* Bits 13-14: how the strip-mined GEMM tiles featureAffine (N = d; d = 400 is five 80-column strips, no multiple of the three a
 * 240-column tile holds).  Results do not depend on them, bit for bit (no output element's product chain changes); they exist for A/B runs.
 * Default (both clear): ragged 240-column tiles, 3 + 2 strips, the full-width tiles dispatched first.
 * DIGAT_PARAMS_RAGGED_OFF: one-strip tiles (each fetches and splits its A tile again).
 * DIGAT_PARAMS_RAGGED_ROWMAJOR: ragged tiles in row-tile-major order (long and short tiles alternate). */
enum { DIGAT_PARAMS_RAGGED_OFF = 8192, DIGAT_PARAMS_RAGGED_ROWMAJOR = 16384 };

/* The same inference for rows that SHARE users: in dev/test scoring the ~37 candidate rows of one
 * impression carry identical user tensors (util.py:57-67 expands them per row).  Here the user side is
 * passed once per group — user_news_embedding [G,H,d], user_graph [G,U,U], user_category_mask [G,C+1],
 * user_category_indices [G,H] — with row_group [B] (int32, values in [0,G), 4*G <= B) naming each row's
 * group; the news side and the context stay per row.  Layer 0's user projections then run on G*U rows
 * instead of B*U.  Results are bit-identical to digat_encoder_fwd on the expanded tensors.  Needs the
 * folded-query fields of digat_params. */
size_t digat_encoder_grouped_workspace_bytes(int B, int N, int H, int C, int d, int depth);
int digat_encoder_fwd_grouped(const digat_params* params,
                              const float* news_graph_embeddings, const uint8_t* news_graph,
                              const uint8_t* news_graph_mask, const float* user_news_embedding_groups,
                              const uint8_t* user_graph_groups, const uint8_t* user_category_mask_groups,
                              const int64_t* user_category_indices_groups, const int32_t* row_group,
                              const float* news_graph_context, float* out_news_context, float* out_user_context,
                              int B, int G, int N, int H, void* workspace, size_t workspace_bytes, void* stream);

/* Layer 0's projections of the NEWS graph ([h|P|Q] = X_n [W|ffn1|ffn2]^T of news[0]) depend on the candidate news alone, like
 * the news representations and c_n0 the reference's driver caches per news (util.py:24-44).  digat_news_project0 computes
 * them for M news graphs: Xn [M,N,d] -> hpq [3][M,N,d] (the launch the encoder itself makes; M*N >= 2048 rows for the bf16x6
 * kernel).  digat_encoder_fwd_grouped_cached takes the batch's rows of that table (news_hpq0 [3][B,N,d], gathered by the
 * caller; NULL = compute as usual) and skips the projection GEMM of layer 0 when N <= 16.  Results are bit-identical.
 * With news_index (the candidate ids; news_graph_embeddings and news_hpq0 are then the whole per-news tables, news_rows rows) the
 * rows are read IN PLACE: by the graph-in-LDS kernel for N <= 16, and — round 4 — by the sparse Eq. 8 kernel for larger news graphs
 * when digat_params.flags has DIGAT_NEWS_XATTN_SPARSE (N = 26, 65: the layer-0 projection GEMM of B N rows, the largest launch of a
 * MIND-large step, goes away; K3 joins in the kernel in the GEMM epilogue's order: the bits of the in-batch launch). */
int digat_news_project0(const digat_params* params, const float* Xn, float* hpq, int M, int N, void* stream);
/* The USER graph's layer-0 projections are row-wise too: those of a history node depend on that news alone, those of a topic
 * node on nothing.  digat_user_project0: X [M,d] -> hpq [3][M,d] with user[0]'s [W|ffn1|ffn2] (for the news table, M = number
 * of news; for the topic table, X = topic_node_embedding, M = C).  The cached entry takes the groups' history rows
 * hist_hpq0 [3][G,H,d] (gathered by the caller with the history ids) and topic_hpq0 [3][C,d] — both or neither — and assembles
 * the groups' [h|P|Q] from them instead of running the projection GEMM (used when B*U >= 2048: below that the in-batch
 * launch is another kernel).  Bit-identical. */
int digat_user_project0(const digat_params* params, const float* X, float* hpq, int M, void* stream);
/* The first link of the [B,d] chain — the topic query, the user-attention query and the user graph's layer-0 K3, all three linear
 * maps of the candidate's cached news context c_n0 (graphEncoders.py:126,133,169 with news_graph_context given, :189) — depends on
 * the news alone.  digat_news_context_queries: c_n [M,d] -> out [3][M,d] (the encoder's own launch, row by row; folded path), kept
 * per news next to c_n0; the cached entry takes the batch's rows ctxq0 [3][B,d] (or NULL) and skips that launch.  Bit-identical. */
int digat_news_context_queries(const digat_params* params, const float* c_n, float* out, int M, void* stream);
/* news_index [B] int64 (or NULL) with news_rows: the per-news tables are read IN PLACE — news_graph_embeddings is then the table
 * [news_rows, N, d] and news_hpq0 the table [3][news_rows, N, d], row b using their row news_index[b] — instead of the caller
 * gathering the batch's rows (130 MB of copies per 1024-row batch at N = 10).  Needs news_graph_context, news_hpq0 and N <= 16
 * (layer 0 of the news graph is then the only reader of the node table).  Bit-identical. */
int digat_encoder_fwd_grouped_cached(const digat_params* params,
                                     const float* news_graph_embeddings, const uint8_t* news_graph, const uint8_t* news_graph_mask,
                                     const float* user_news_embedding_g, const uint8_t* user_graph_g,
                                     const uint8_t* user_category_mask_g, const int64_t* user_category_indices_g,
                                     const int32_t* row_group, const float* news_graph_context, const float* news_hpq0,
                                     const float* hist_hpq0, const float* topic_hpq0, const float* ctxq0,
                                     const int64_t* news_index, int64_t news_rows,
                                     float* out_news, float* out_user, int B, int G, int N, int H,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* H1: Model.inference's last line (model.py:89): logits[b] = sum_c user_ctx[b,c] * news_ctx[b,c]. */
int digat_row_logits(const float* news_ctx, const float* user_ctx, float* logits, int B, int d, void* stream);

/* ---- training: native forward/backward pairs for every op on the path ----------------------------
 * The reference trains by autograd through DIGAT.forward (trainer.py:98-102).  digat_amd/training.py
 * composes the same forward from these primitives (each an autograd.Function); Eq. 8's backward
 * recomputes relu'(K3+K1+K2) from the saved projections instead of saving [B,n,n,d].  All reductions
 * are ordered (no atomics), so gradients are run-to-run reproducible.  `accumulate` != 0 adds into the
 * destination. */
int digat_linear_bwd_input(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx,
                           int M, int N, int K, int accumulate, void* stream);
/* The same on the bf16 matrix cores (bf16x6: fp32-grade).  W^T is split into `wsplit` (digat_split_weights_bytes(K, N)
 * bytes) by every call — the weights change every optimiser step.  M >= 2048, K % 80 == 0, N % 8 == 0, N >= 32. */
int digat_linear_bwd_input_x3(const float* dy, int64_t lddy, const float* w, float* dx, int64_t lddx,
                              int M, int N, int K, int accumulate, void* wsplit, void* stream);           /* dx[M,K] = dy[M,N] @ w[N,K] */
size_t digat_linear_bwd_weight_workspace(int M, int No, int Ni);
int digat_linear_bwd_weight(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dW, float* db,
                            int M, int No, int Ni, int accumulate, void* workspace, size_t workspace_bytes,
                            void* stream);                                                /* dW = dy^T x, db = colsum(dy) */
int digat_colsum(const float* x, int64_t ldx, float* out, int M, int N, int accumulate, void* stream);
int digat_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint32_t seed, void* stream);
int digat_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p, void* stream);
int digat_gate_fwd(const float* z, const float* l, int64_t ldl, const float* g, float* out, int B, int d, void* stream);
int digat_gate_bwd(const float* dout, const float* z, const float* l, int64_t ldl, const float* g,
                   float* dz, float* dl, float* dg, int B, int d, void* stream);
int digat_relu_res_fwd(const float* y, const float* t, float* out, int64_t n, void* stream);   /* relu(y) + t */
int digat_relu_mask(const float* dout, const float* y, float* dy, int64_t n, void* stream);    /* dout * [y > 0] */
int digat_attn_pool_fwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, float* out,
                        float* alpha_out, int B, int n, int d, void* stream);
int digat_attn_pool_bwd(const float* feat, int64_t ld_b, const float* kq, const uint8_t* mask, const float* alpha,
                        const float* dout, float* dfeat, int64_t ldd_b, float* dkq, int B, int n, int d,
                        int accumulate_dfeat, void* stream);
int digat_topic_pool_fwd_train(const float* Xu, const float* kq, const int64_t* cat_idx, float* out, float* alpha_out,
                               int B, int U, int H, int C1, int d, void* stream);
int digat_topic_pool_bwd(const float* Xu, const float* kq, const int64_t* cat_idx, const float* alpha, const float* dT,
                         float* dXu, float* dkq, int B, int U, int H, int C1, int d, void* stream);
int digat_xattn_project(const float* X, const float* r, const float* W, const float* bW, const float* F1,
                        const float* F2, float* h, float* Pr, float* Q, int B, int n, int d, void* stream);
/* ... with the bf16x6 kernel: [W|ffn1|ffn2] is split into `wsplit` (digat_split_weights_bytes(3 d, d) bytes) first.
 * B*n >= 2048, d % 80 == 0. */
int digat_xattn_project_x3(const float* X, const float* r, const float* W, const float* bW, const float* F1, const float* F2,
                           float* h, float* Pr, float* Q, int B, int n, int d, void* wsplit, void* stream);
int digat_xattn_pairwise_fwd_train(const float* Pr, const float* Q, const float* h, const float* X, const float* a,
                                   const uint8_t* A, float* out, float* alpha, float* s_pre, float* alpha_drop,
                                   uint8_t* amask, float p, uint32_t seed, int B, int n, int d, void* stream);
size_t digat_xattn_pairwise_bwd_workspace(int B, int n, int d);
int digat_xattn_pairwise_bwd(const float* dOut, const float* out, const float* Xres, const float* Pr, const float* Q,
                             const float* h, const float* a, const uint8_t* A, const float* alpha, const float* s_pre,
                             const uint8_t* amask, float p, float* dPr, float* dQ, float* dh, float* da,
                             int accumulate_da, int B, int n, int d, void* workspace, size_t workspace_bytes,
                             void* stream);
int digat_sum_nodes(const float* dP, float* dr, int B, int n, int d, void* stream);          /* dr[b] = sum_j dP[b,j] */

/* BASELINE configs[4], training half.  1: the >= 2048-row GEMMs of the training path (Eq. 8 projections, featureAffine,
 * their input and weight gradients) run with ONE bf16 product per fp32 product — bf16 mixed precision: fp32 master weights and
 * activations, bf16 matrix-core operands, fp32 accumulation; 0 (default): the fp32-grade six-product split.  The [B,d] linears
 * (and their weight gradients) and every reduction stay fp32.  Returns the previous setting. */
int digat_set_train_precision(int bf16);

/* The operand format of the >= 2048-row matrix-core GEMMs (node projections, featureAffine): DIGAT_GEMM_BF16X6 = every fp32
 * value as three bf16 pieces, six products — as accurate as an fp32 fma chain, no range limit; DIGAT_GEMM_F16X3 = two fp16
 * pieces (22-23 significant bits), three products on v_mfma_f32_16x16x32_f16: 0.7x the time.  The weights are scaled by 2^10 and
 * the activations by 2^4 on their way in (exact; undone in the epilogue) so that the low pieces of ordinary values are normal
 * fp16 numbers: against fp64 its mean and largest errors are at or below an fp32 fma chain's (tests/test_hip_lowprec.py) for
 * |w| < 63 and 1e-4 < |x| < 4094; far below the lower bound the pieces are subnormal (an absolute floor of 2^-24 per term);
 * at the upper bound the high piece saturates (precision degrades to ~2^-15, then inf) — the kernel reports that through
 * digat_params.range_flag.
 * There is NO process-wide setting: the format is a property of a split image.  It is chosen by whoever splits the weights
 * (the `format` argument of digat_split_*), the encoder entry points are told through digat_params.flags & DIGAT_PARAMS_GEMM_F16X3 (bit 6 = 64; NOT the enum value DIGAT_GEMM_F16X3 = 1)
 * (every wsplit image of one digat_params has the same format), and the library remembers the format of every image it has
 * split: a launch that names the other format returns DIGAT_ERR_ARG instead of misreading the image.  The training entries
 * (digat_*_fwd_train, digat_*_bwd, digat_linear_bwd_input_x3, digat_xattn_project_x3) and the MSA encoder split their weights in
 * DIGAT_GEMM_BF16X6: gradients have no lower bound (1e-6 and below is ordinary) and fp16 pieces of such values are subnormal or
 * zero; bf16 pieces keep fp32's exponent range.  Two host threads on two streams may therefore run an fp16x3 evaluation and a
 * training step at the same time. */
enum { DIGAT_GEMM_BF16X6 = 0, DIGAT_GEMM_F16X3 = 1 };
/* DIGAT_GEMM_F16F8C ("fp16-fp8c", BASELINE configs[4] on the fp8 matrix cores; images of the Eq. 8 node projections
 * [W|ffn1|ffn2] only): fp16x3's three products with the two corrections, x_hi w_lo and x_lo w_hi, on the block-scaled
 * v_mfma_scale_f32_16x16x128_f8f6f4 — operands OCP e4m3 with one E8M0 (power-of-two) scale per 32 consecutive K values, the
 * largest magnitude of a block mapped to at most 448 — and the leading x_hi w_hi on v_mfma_f32_16x16x32_f16 as in fp16x3 (same
 * 2^10 / 2^4 scaling, same range limits, same range flag).  Each correction is ~2^-11 of the result and carries e4m3's 2^-4
 * relative step, so the product's relative error is ~2^-15 of the row scale (fp16x3: below an fp32 fma chain's); outputs stay
 * fp32.  Image: per (80-column strip, 128-deep K tile; K zero-padded to a multiple of 128) the fp16 w_hi plane, the e4m3 planes of
 * q(w_hi) and q(w_lo) and their scale bytes, 41 984 bytes (csrc/digat_gemm.inc, section 1e):
 * digat_split_weights_bytes_format(rows, K, DIGAT_GEMM_F16F8C) bytes, NOT digat_split_weights_bytes (which is too small for
 * K <= 96).  Any M; row lists; no bf16 / e4m3 output segments (digat_xattn_fwd_lowprec: pq = 0 only). */
enum { DIGAT_GEMM_F16F8C = 2 };
/* bytes of a split image of a [rows, K] weight (or of a stack of them: rows = the stacked rows) in `format`; formats 0 and 1
 * give exactly digat_split_weights_bytes(rows, K).  0 for an unknown format. */
size_t digat_split_weights_bytes_format(int rows, int K, int format);

/* The step's head and tail around the encoder (round 6): the backward of digat_row_logits (model.py:75: logits = sum_d user_ctx news_ctx)
 * and the loss of trainer.py:100 — mean over the B impressions of -log_softmax(logits [B,K])[:, 0] — with its gradient d loss / d logits
 * [B,K] (written by the same launch: the caller scales it by the loss's incoming gradient). */
int digat_row_logits_bwd(const float* dlogits, const float* news_ctx, const float* user_ctx, float* dnews, float* duser, int B, int d,
                         void* stream);
int digat_click_loss(const float* logits, int B, int K, float* loss, float* dlogits, void* stream);

/* The optimiser's step (trainer.py:30, :103-105: clip_grad_norm_ + Adam) as three launches: the squared gradient norm per chunk, its
 * total, and one pass over (p, g, m, v) that applies the clipping coefficient min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no
 * clipping) and torch.optim.Adam's update (coupled weight decay per tensor; bias corrections from `step` >= 1).  `tensors`: an array
 * of digat_opt_tensor in DEVICE memory; chunk c covers the digat_opt_chunk() elements of tensor chunk_tensor[c] from chunk_off[c];
 * scratch: nchunks + 1 floats.  The gradients are read, not rewritten. */
typedef struct digat_opt_tensor { float* p; const float* g; float* m; float* v; int64_t n; float weight_decay; int32_t pad; } digat_opt_tensor;
int digat_opt_chunk(void);
int digat_clip_adam_step(const void* tensors, const int32_t* chunk_tensor, const int64_t* chunk_off, int nchunks, float* scratch, float max_norm,
                         float lr, float beta1, float beta2, float eps, int step, void* stream);

/* ---- training: the three functions of the path as one forward and one backward call each ----------------
 * Composed on the C++ side from the primitives above (digat_train_abi.inc); digat_amd/training.py wraps each pair in one
 * autograd.Function.  `save` is a caller-owned buffer carrying what the backward needs from the forward (private layout,
 * *_save_bytes); `workspace` is scratch (*_workspace_bytes, the same size for both directions).  Dropout: the library's
 * counter-hash generator with the caller's seed; p = 0 disables it.  Gradients are WRITTEN (not accumulated) and
 * bit-reproducible (ordered reductions).
 *
 * a1 / a2 (graphEncoders.py:143-154, :163-174).  X is the layer input AFTER its input dropout drop_{p/2} (the residual uses
 * the dropped input); out = relu(drop_p(alpha) h) + X.  The backward recomputes relu'(K3+K1+K2) from the saved projections. */
/* Split images made ahead (round 6).  The matrix-core products of these entries read their weights as bf16x6 images; by default
 * every call splits its own (the weights change every optimiser step): 20 split launches per 64 x 5-row step.  digat_split_jobs
 * writes any number of images (<= 24) in ONE launch — once per step, after the optimiser's update — and the entries take the
 * image of THEIR weights in THEIR layout through the *_image arguments (NULL: split inside, as before).  An image is only a
 * function of the weight values: the caller keeps it valid (same weights, not freed) until the calls that read it have been
 * enqueued on the same stream.
 *   layout 0: y = x [w0 | w1 | w2]^T, the forward product of nn.Linear weights [rows, cols] (w1 = w2 = NULL: one matrix);
 *   layout 1: dx = dy w0, the input gradient ([dy0 | dy1 | dy2] [w0; w1; w2] with three matrices). */
typedef struct digat_split_job {
    const float *w0, *w1, *w2;   /* [rows, cols] each; w1, w2 both NULL or both given */
    int32_t rows, cols, layout, reserved;
    void* image;                 /* digat_split_job_bytes(rows, cols, layout, 1 or 3) bytes */
} digat_split_job;
size_t digat_split_job_bytes(int rows, int cols, int layout, int matrices);
int digat_split_jobs(const digat_split_job* jobs, int njobs, void* stream);

size_t digat_xattn_train_save_bytes(int B, int n, int d);
size_t digat_xattn_train_workspace_bytes(int B, int n, int d);
/* proj_image: NULL, or the layout-0 image of (W, F1, F2); bwd_image: NULL, or their layout-1 image.
 * p_in > 0 (round 6): X is the layer input BEFORE its input dropout; the entry applies drop_{p_in} with seed_in itself (the dropped
 * input and its keep bytes travel in `save`), out = relu(drop_p(alpha) h) + drop(X), and the backward's dX is the gradient of the
 * UNDROPPED X — the keep bytes are applied in the epilogue of the input-gradient product, no dropout launch.  p_in = 0: X is used
 * as given (callers that drop their input themselves).  The backward takes the same p_in.
 * xattn_mode (graphs of more than 16 nodes; both directions take the same value): which kernels evaluate Eq. 8 — a choice of speed
 * only, the function is the same.  DIGAT_TRAIN_XATTN_AUTO: decided on the device per batch from a sample of the adjacency (the
 * entry-wise kernels when it holds at most ~20 entries per node, the all-pairs kernels otherwise; the launches of the side not
 * taken return at once); _SPARSE: the entry-wise kernels (a wave per centre / per node over the adjacency's entries), _DENSE: the
 * all-pairs kernels — unguarded: a caller that knows its corpus saves the decision and the empty launches.
 * xattn_mode is a HINT: each direction follows it where its own kernels fit (csrc/digat_xattn_plan.h: eq8_train_fwd_route,
 * eq8_train_bwd_route).  Graphs of at most 16 nodes ignore it (one fused forward launch; the entry-wise backward).  The entry-wise
 * forward takes d <= 1024, the entry-wise backward d <= 512: for 512 < d <= 1024 a forward that ran entry-wise is followed by the
 * all-pairs backward whatever the mode, and beyond d = 1024 the entry refuses the shape.  Every combination computes the same
 * function from the same saved tensors, so the two directions need not agree. */
enum { DIGAT_TRAIN_XATTN_AUTO = 0, DIGAT_TRAIN_XATTN_SPARSE = 1, DIGAT_TRAIN_XATTN_DENSE = 2 };
int digat_xattn_fwd_train(const float* X, const uint8_t* A, const float* ctx, const float* W, const float* bW, const float* F1,
                          const float* F2, const float* F3, const float* b3, const float* a, float* out, float p_alpha,
                          uint32_t seed, float p_in, uint32_t seed_in, int B, int n, int d, void* save, size_t save_bytes, void* workspace,
                          size_t workspace_bytes, const void* proj_image, int xattn_mode, void* stream);
int digat_xattn_bwd(const float* dOut, const float* out, const float* X, const uint8_t* A, const float* ctx, const float* W,
                    const float* F1, const float* F2, const float* F3, const float* a, float p_alpha, float p_in, const void* save,
                    size_t save_bytes, float* dX, float* dctx, float* dW, float* dbW, float* dF1, float* dF2, float* dF3,
                    float* db3, float* da, int B, int n, int d, void* workspace, size_t workspace_bytes, const void* bwd_image,
                    int xattn_mode, void* stream);
/* a3 (graphEncoders.py:109-114): out = gate(drop_{p_gate}(W_g [l ; g] + b_g), l, g), l = X[:,0], g = candidate_attention(X, l). */
size_t digat_news_ctx_train_save_bytes(int B, int N, int d);
size_t digat_news_ctx_train_workspace_bytes(int B, int N, int d);
int digat_news_ctx_fwd_train(const float* X, const uint8_t* mask, const float* Kc, const float* Qc, const float* bQc,
                             const float* Wg, const float* bg, float* out, float p_gate, uint32_t seed, int B, int N, int d,
                             void* save, size_t save_bytes, void* workspace, size_t workspace_bytes,
                             const float* prev /* NULL, or [B,d]: out = prev + context (graphEncoders.py:185; d prev = dout) */, void* stream);
/* accumulate_params != 0: the PARAMETER gradients (dKc, dQc, dbQc, dWg, dbg) are added to what their buffers hold instead of
 * overwriting it — the context functions' weights are shared by the depth + 1 calls of a step (graphEncoders.py:177-187: one
 * candidate_attention / news_graph_W for every layer), so a caller can sum a step's gradients in one set of buffers inside the
 * weight-gradient launches themselves (training.py's StepSink) instead of one element-wise add per weight and call.  dX is always
 * written. */
int digat_news_ctx_bwd(const float* dout, const float* X, const uint8_t* mask, const float* Kc, const float* Qc, const float* Wg,
                       float p_gate, const void* save, size_t save_bytes, float* dX, float* dKc, float* dQc, float* dbQc,
                       float* dWg, float* dbg, int B, int N, int d, int accumulate_params, void* workspace, size_t workspace_bytes,
                       void* stream);
/* a4 (+a6, a7) (graphEncoders.py:123-134): topic pooling (scatter_softmax + scatter_sum), featureAffine + relu + residual,
 * drop_{p_topic}, userAttention.  dXu [B,U,d]: history rows get the pooling's gradient, topic rows zero. */
size_t digat_user_ctx_train_save_bytes(int B, int U, int H, int C1, int d);
size_t digat_user_ctx_train_workspace_bytes(int B, int U, int H, int C1, int d);
int digat_user_ctx_fwd_train(const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n, const float* Ku,
                             const float* Qu, const float* bQu, const float* Fa, const float* bFa, const float* Kua,
                             const float* Qua, const float* bQua, float* out, float p_topic, uint32_t seed, int B, int U, int H,
                             int C1, int d, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes,
                             const void* fa_image /* NULL, or the layout-0 image of Fa */,
                             const float* prev /* NULL, or [B,d]: out = prev + context (graphEncoders.py:186) */, void* stream);
int digat_user_ctx_bwd(const float* dout, const float* Xu, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n,
                       const float* Ku, const float* Qu, const float* Fa, const float* Kua, const float* Qua, float p_topic,
                       const void* save, size_t save_bytes, float* dXu, float* dc_n, float* dKu, float* dQu, float* dbQu,
                       float* dFa, float* dbFa, float* dKua, float* dQua, float* dbQua, int B, int U, int H, int C1, int d,
                       int accumulate_params /* as digat_news_ctx_bwd: the eight parameter gradients; dXu, dc_n are always written */,
                       void* workspace, size_t workspace_bytes, const void* fa_bwd_image /* NULL, or the layout-1 image of Fa */, void* stream);

/* ---- H2: ranking + metrics of the dev/test driver  (util.py:70-80, evaluate.py:32-89) -------------------
 * scores [R] f32 in impression-major row order; impression_start [I+1] int64 (row offsets; impression i owns
 * rows [start[i], start[i+1])).  ranks [R] int32 receives the 1-based rank of every candidate after a STABLE
 * descending sort of its impression's scores (what util.py:73-79 writes to the rank file).  With labels [R]
 * (bytes, non-zero = clicked) and per_impression [I,4] f64 it also writes AUC, MRR, nDCG@5, nDCG@10 of every
 * impression on 1/rank scores (evaluate.py:45-60), and with mean4 [4] their means over the I impressions
 * (evaluate.py:85-89).  labels / per_impression / mean4 may be NULL (ranks only). */
int digat_rank_metrics(const float* scores, const uint8_t* labels, const int64_t* impression_start, int num_impressions,
                       int32_t* ranks, double* per_impression, double* mean4, void* stream);

/* The rank file of util.py:74-84 as bytes, formatted on the HOST (no GPU work): "<impression id> [r1,r2,...]" per line for ids
 * 1 .. impressions ("[]" for an id without rows), lines joined by '\n', no trailing newline.  ranks [R] int64 (1-based ranks in
 * row order), starts [impressions + 1] int64 row ranges.  Returns the number of bytes written, or — when out is NULL or cap is too
 * small — the capacity needed. */
int64_t digat_format_rank_file(const int64_t* ranks, const int64_t* starts, int64_t impressions, char* out, int64_t cap);

/* ---- segmented top-k: which k elements of every segment, in order (digat_amd.util.recommend) ----------------------
 * scores [rows] f32; seg_start [segments + 1] int64, non-decreasing, on the DEVICE (segment s owns rows [start[s], start[s+1]);
 * values outside [0, rows] are held inside it).  Within a segment elements are ordered by score descending, ties by position
 * ascending (the order of digat_rank_metrics and of list.sort(reverse=True)); -0.0 == +0.0; a NaN orders after every number,
 * -inf included, NaNs among themselves by position.  ids [rows] int64 or NULL (NULL: the position inside the segment is
 * returned).  skip [segments, skip_len] int64 or NULL / 0: an element whose id occurs in its segment's skip row is left out
 * (skip without ids: DIGAT_ERR_ARG); repeated ids inside a segment are distinct elements.
 * out_count [segments] = min(k, elements left); slots j < count of out_scores / out_ids [segments, k] hold the j-th element's
 * original score bits and its id (or position), slots j >= count hold -inf and -1: every output byte is written, for empty
 * segments too.  1 <= k <= 128, 0 <= skip_len <= 256 and non-null required pointers (DIGAT_ERR_ARG otherwise, before any
 * launch); rows / DIGAT_TOPK_CHUNK + segments < 2^31 (DIGAT_ERR_SHAPE); a short workspace is DIGAT_ERR_WORKSPACE (it may hold
 * anything on entry); segments == 0 returns DIGAT_OK.  Stream-ordered: two launches on `stream`, sized by rows and segments
 * alone (one workgroup per chunk of DIGAT_TOPK_CHUNK elements, then one per segment); no allocation, no host synchronisation,
 * no read of seg_start on the host. */
#define DIGAT_TOPK_CHUNK 16384
size_t digat_topk_segments_workspace_bytes(int64_t rows, int64_t segments, int k);
int digat_topk_segments(const float* scores, const int64_t* seg_start, int64_t rows, int64_t segments, const int64_t* ids,
                        const int64_t* skip, int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- inner-product retrieval: the k best rows of a table per user vector, without the score matrix (digat_amd.nrms.recommend) ---
 * users [G, d] f32, news [N, d] f32; pool [P] int64 row ids of news, or NULL = rows 0 .. N-1 in order (then P must equal N).
 * score(g, p) = the fp32 fmaf chain over c = 0 .. d-1 from 0 of users[g][c] * news[pool[p]][c], on the fp32 matrix cores: its bits
 * depend on the two vectors and d alone — not on G, N, P, the pool order, the tile, or which of the two entries computed it.
 * digat_dot_topk is digat_topk_segments over G segments of equal length P without the scores in memory: for user g the elements
 * are the pool positions whose id is not in skip[g] ([G, skip_len] int64, or NULL / 0) and lies in [0, N) (any other id is no
 * element, and no read leaves the arrays); order: topk_key of the score descending, ties by pool position, NaNs last,
 * -0.0 == +0.0; repeated ids are distinct elements.  out_count [G] = min(k, elements); slots j < count of out_scores / out_ids
 * [G, k] hold the j-th element's score bits and pool id (the row number when pool is NULL), slots j >= count hold -inf and -1:
 * every output byte is written.  1 <= k <= 128, 0 <= skip_len <= 256, d > 0, non-null required pointers, sizes >= 0, an
 * 8-byte-aligned workspace (DIGAT_ERR_ARG otherwise); ceil(G / DIGAT_DOT_TOPK_USERS) * ceil(P / DIGAT_DOT_TOPK_CHUNK) < 2^31
 * (DIGAT_ERR_SHAPE); a short workspace is DIGAT_ERR_WORKSPACE (it may hold anything on entry) — all before any launch.  G == 0
 * returns DIGAT_OK without a launch; P == 0 sets every count to 0.  Workspace: 8 k bytes per (user, chunk of
 * DIGAT_DOT_TOPK_CHUNK pool positions).  Stream-ordered: two launches on `stream` (one workgroup per tile of
 * DIGAT_DOT_TOPK_USERS users and chunk, walking sub-tiles of DIGAT_DOT_TOPK_SUB positions; then one per user); no allocation,
 * no host synchronisation, no read of device memory on the host.
 * digat_dot_scores: the same product stored as out [G, P] — the yardstick of the fused entry, and the way to the matrix for
 * callers who want it (a position whose id is outside [0, N) reads a zero row). */
#define DIGAT_DOT_TOPK_CHUNK 2048
#define DIGAT_DOT_TOPK_USERS 64
#define DIGAT_DOT_TOPK_SUB 64
size_t digat_dot_topk_workspace_bytes(int64_t users, int64_t pool, int k);
int digat_dot_topk(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t* skip,
                   int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes,
                   void* stream);
int digat_dot_scores(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, float* out,
                     void* stream);

/* ---- long shortlists: the two selections above for lists of up to 1024 entries (digat_amd.nrms.shortlist) ------------------------
 * digat_shortlist_segments is digat_topk_segments' contract to the letter with 1 <= m <= DIGAT_SHORTLIST_MAX_K in place of
 * 1 <= k <= 128: elements, order (topk_key descending, ties by position, NaNs last, -0.0 == +0.0), ids, skip rows (skip_len <= 256,
 * skip needs ids), the seg_start held inside [0, rows] and made non-decreasing (a malformed array gives wrong numbers, no access
 * outside the arrays), outputs [segments, m] with -inf / -1 at and beyond out_count, every output byte written, the refusals and
 * their order, segments == 0 returning DIGAT_OK.  For m <= 128 its outputs are digat_topk_segments', bit for bit.  Workspace: 8 m
 * bytes per chunk slot (rows / DIGAT_TOPK_CHUNK + segments of them; it may hold anything on entry).  Stream-ordered: two launches
 * sized by rows and segments alone (one workgroup per chunk of DIGAT_TOPK_CHUNK elements — none when rows <= 1024 —, then one per
 * segment, which orders its winners by a sort in LDS); no allocation, no host synchronisation, no read of seg_start on the host.
 * digat_dot_shortlist is digat_dot_topk's contract with that bound: elements (pool ids in [0, N), not in skip[g]), scores (the bits
 * digat_dot_scores stores), order, outputs and refusals are its.  The users are walked in slabs of slab_users (<= 0: 256; any
 * positive value is legal and the results do not depend on it): per slab digat_dot_scores' kernel stores [slab, P] scores in the
 * workspace and the selection runs over them as slab segments of length P, so the workspace — slab * P * 4 bytes, rounded up to
 * 256, plus 8 m bytes per (slab user, chunk of DIGAT_TOPK_CHUNK pool positions) — depends on slab_users and not on G.  The shape
 * limits (DIGAT_ERR_SHAPE) hold per slab.  G == 0 returns DIGAT_OK without a launch; P == 0 sets every count to 0; neither needs a
 * workspace.  Stream-ordered: up to three launches per slab, their number and sizes given by G, P and slab_users alone; no
 * allocation, no host synchronisation, no read of device memory on the host. */
#define DIGAT_SHORTLIST_MAX_K 1024
size_t digat_shortlist_segments_workspace_bytes(int64_t rows, int64_t segments, int m);
int digat_shortlist_segments(const float* scores, const int64_t* seg_start, int64_t rows, int64_t segments, const int64_t* ids,
                             const int64_t* skip, int skip_len, int m, float* out_scores, int64_t* out_ids, int32_t* out_count,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t digat_dot_shortlist_workspace_bytes(int64_t G, int64_t P, int m, int64_t slab_users);
int digat_dot_shortlist(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                        const int64_t* skip, int skip_len, int m, int64_t slab_users, float* out_scores, int64_t* out_ids,
                        int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- quantised first stage: the three inner-product entries above on int8 codes (digat_amd.nrms.build_index, recommend(index=)) ----
 * digat_quantize_rows_i8: x [R, d] f32 -> q [R, dq] int8 and scale [R] f32, per row and symmetric: amax = max |x|,
 * scale = amax / 127.0f, q[c] = clamp(rint(x[c] / scale), -127, 127) — fp32 divisions correctly rounded, rint to nearest even, so numpy
 * float32 gives the same bytes —, q[d .. dq) = 0.  dq must be d rounded up to 16 (DIGAT_ERR_ARG otherwise); 0 < d <=
 * DIGAT_QDOT_MAX_D (beyond: DIGAT_ERR_SHAPE).  scale == 0 (a zero row, an amax that underflows): codes 0.  A row with a NaN or an
 * infinity: codes 0 and scale NaN — its scores are NaN and order last.  R == 0 returns DIGAT_OK without a launch.
 * qu [G, dq], qn [N, dq] int8 (16-byte aligned; rows of dq bytes with zeros from d on), su [G], sn [N] f32; pool, G, N, P, skip,
 * skip_len, k / m, slab_users, the outputs and the workspace are those of digat_dot_scores, digat_dot_topk and digat_dot_shortlist.
 * score(g, p) = ((float)acc * su[g]) * sn[id]: acc the int32 sum over the channels of qu[g][c] * qn[id][c] (v_mfma_i32_16x16x64_i8),
 * converted exactly (|acc| <= 127^2 d < 2^24), then two fp32 multiplications from left to right.  Its bits depend on the two code rows
 * and the two scales alone — not on G, N, P, the pool order, the tile, or which of the three entries computed it.
 * digat_qdot_scores stores out [G, P] (+0.0 at a position whose id is outside [0, N)); digat_qdot_topk (1 <= k <= 128) and
 * digat_qdot_shortlist (1 <= m <= DIGAT_SHORTLIST_MAX_K) are digat_dot_topk's and digat_dot_shortlist's contracts to the letter on
 * these scores: elements, order (topk_key descending, ties by pool position, NaNs last), skip rows, fill, count, workspace sizes
 * (the _workspace_bytes below return what their fp32 twins return), launches and the order of the refusals, where the operand test
 * is: null qu / su / qn / sn, negative sizes, d <= 0, pool == NULL with P != N, dq != d rounded up to 16, or codes not 16-byte
 * aligned: DIGAT_ERR_ARG; d > DIGAT_QDOT_MAX_D or too many workgroups: DIGAT_ERR_SHAPE. */
#define DIGAT_QDOT_MAX_D 1024
int digat_quantize_rows_i8(const float* x, int64_t R, int d, int dq, int8_t* q, float* scale, void* stream);
int digat_qdot_scores(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N, int64_t P,
                      int d, int dq, float* out, void* stream);
size_t digat_qdot_topk_workspace_bytes(int64_t users, int64_t pool, int k);
int digat_qdot_topk(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N, int64_t P,
                    int d, int dq, const int64_t* skip, int skip_len, int k, float* out_scores, int64_t* out_ids, int32_t* out_count,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t digat_qdot_shortlist_workspace_bytes(int64_t G, int64_t P, int m, int64_t slab_users);
int digat_qdot_shortlist(const int8_t* qu, const float* su, const int8_t* qn, const float* sn, const int64_t* pool, int64_t G, int64_t N,
                         int64_t P, int d, int dq, const int64_t* skip, int skip_len, int m, int64_t slab_users, float* out_scores,
                         int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- retrieval evaluation: the rank of given targets in a user's whole ordered pool (digat_amd.nrms.retrieval_metrics) ---------
 * users, news, pool, G, N, P, d, skip, skip_len: digat_dot_topk's, and so are the elements of user g (the pool positions whose id
 * lies in [0, N) and is not in skip[g]; repeated ids are distinct elements, skip rows may repeat ids), their scores (the bits
 * digat_dot_scores stores) and their order (topk_key descending, ties by pool position, NaNs last, -0.0 == +0.0).
 * target_pos [T] int64: pool positions; target_start [G + 1] int64, non-decreasing from 0 to T, on the DEVICE: user g owns targets
 * [start[g], start[g+1]) — none, one or many, repeated positions allowed (values are held inside [0, T] and made non-decreasing
 * before use: a malformed array gives wrong numbers, no access outside the arrays).
 * out_rank [T] int32 = the number of elements of the target's user that order before the target, or -1 when the target is no
 * element of its user (position outside [0, P), id outside [0, N), id skipped); out_scores [T] f32 = the target's score bits, or a
 * NaN where the rank is -1: every output byte is written.  For any k <= 128, 0 <= rank < k exactly when digat_dot_topk's list of
 * that user holds the element at slot rank; the ranks of all elements of a user are a permutation of 0 .. elements - 1.
 * DIGAT_ERR_ARG: a null required pointer (pool, skip and — for T == 0 — workspace may be NULL), a negative size, d <= 0, skip_len
 * outside [0, 256], pool == NULL with P != N, a workspace that is not 8-byte aligned; DIGAT_ERR_SHAPE:
 * ceil(G / DIGAT_DOT_TOPK_USERS) * ceil(P / DIGAT_DOT_TOPK_CHUNK) or T at or beyond 2^31; DIGAT_ERR_WORKSPACE: a short workspace
 * (it may hold anything on entry) — all before any launch.  T == 0 or G == 0 returns DIGAT_OK without a launch (nobody owns a
 * target when G == 0: nothing is written); P == 0 makes every rank -1.  Workspace: 4 bytes per target.  Stream-ordered: three
 * launches on `stream` (one thread per target; one workgroup per tile of DIGAT_DOT_TOPK_USERS users for the targets' own scores; one
 * per tile and chunk of DIGAT_DOT_TOPK_CHUNK positions, which returns at once for a tile without targets); no allocation, no host
 * synchronisation, no read of device memory on the host. */
size_t digat_dot_rank_workspace_bytes(int64_t users, int64_t pool, int64_t targets);
int digat_dot_rank(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d, const int64_t* skip,
                   int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, int32_t* out_rank, float* out_scores,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- retrieval training: softmax loss of given targets over a user's whole pool, and its gradients (digat_amd.nrms.retrieval_step) ---
 * users, news, pool, G, N, P, d, skip, skip_len, target_pos, target_start, T: digat_dot_rank's, and so are the elements of user g, their
 * scores (the bits digat_dot_scores stores), the clamping of target_start and the meaning of "ranked": the target is an element of its
 * user.  x(g, p) = scale * score(g, p).
 * Forward: out_lse [G] = log of the sum of exp(x(g, p)) over g's elements (-inf when g has none; the maximum is always subtracted);
 * out_loss [T] = lse[g(t)] - x(g(t), pos[t]) for a ranked target, 0 otherwise; out_target_score [T] = digat_dot_rank's out_scores (score
 * bits, a NaN where not ranked).  Every output byte is written whatever target_start holds (G == 0: out_loss and out_target_score).
 * Backward, given lse [G] (the forward's) and grad_loss [T] (ignored where the target is not ranked): with c[g] = the sum of grad_loss
 * over g's ranked targets in ascending t and C(g, p) = c[g] exp(x(g, p) - lse[g]) - (the grad_loss of g's ranked targets at p, subtracted
 * in ascending t) on elements, 0 elsewhere,
 *   d_users [G, d] = scale * sum_p C(g, p) news[id(p), :]          d_rows [P, d] = scale * sum_g C(g, p) users[g, :]
 * — d_rows has one row per POOL POSITION: scattering it over repeated ids is the caller's.  A user with c[g] == 0 never meets its lse
 * (no NaN from lse = -inf).  Every byte of d_users and d_rows is written.  No floating-point atomics: every sum's order is fixed by the
 * shapes and the targets, two calls give the same bits.
 * DIGAT_ERR_ARG, DIGAT_ERR_SHAPE and DIGAT_ERR_WORKSPACE as digat_dot_rank, before any launch; the backward takes d <= 512
 * (DIGAT_ERR_SHAPE beyond: its 64 x d block of accumulators lives in registers), the forward any d.
 * Workspace (one query for both; it may hold anything on entry), every region rounded up to 256 bytes:
 *   20 T  +  8 G ceil(P / DIGAT_DOT_TOPK_CHUNK)  +  4 G  +  4 tiles  +  256 d min(tiles ceil(P / DIGAT_DOT_TOPK_CHUNK), 256 + tiles),
 * tiles = ceil(G / DIGAT_DOT_TOPK_USERS): nothing the size of the [G, P] matrix — of it there is one (reference, sum) pair per user and
 * chunk —; 0 for a negative argument or d <= 0.
 * Stream-ordered: four launches forward, six backward, sized by G, P, T and d alone; no allocation, no host synchronisation, no read of
 * device memory on the host. */
size_t digat_pool_softmax_workspace_bytes(int64_t users, int64_t pool, int64_t targets, int d);
int digat_pool_softmax_fwd(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                           const int64_t* skip, int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, float scale,
                           float* out_loss, float* out_lse, float* out_target_score, void* workspace, size_t workspace_bytes, void* stream);
int digat_pool_softmax_bwd(const float* users, const float* news, const int64_t* pool, int64_t G, int64_t N, int64_t P, int d,
                           const int64_t* skip, int skip_len, const int64_t* target_pos, const int64_t* target_start, int64_t T, float scale,
                           const float* lse, const float* grad_loss, float* d_users, float* d_rows, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- listwise distillation: softmax over a user's own list held against a target distribution (digat_amd.evaluate.list_softmax) ---
 * users [G, d] f32, rows [P, d] f32, ids [G, M] int64, count [G] int32 (NULL: M), teacher [G, M] f32, scale, temperature > 0.  Slot
 * (g, j) is an element when j < clamp(count[g], 0, M) and 0 <= ids[g, j] < P; a repeated id in one list is two elements.  score(g, j) is
 * the fp32 fmaf chain over the d channels (the bits digat_dot_scores stores), x = scale * score.  tau = teacher / temperature where the
 * slot is an element and teacher is finite; an element whose teacher is -inf, +inf or NaN has target mass 0.  q = softmax(tau) over the
 * elements with mass, p = softmax(x) over all elements.
 * Forward: out_lse [G] = log of the sum of exp(x) over g's elements (-inf without one; the maximum is always subtracted); out_loss [G] =
 * KL(q || p) = lse_x - lse_tau + sum_j q_j (tau_j - x_j), and out_valid [G] = 1 — loss 0 and valid 0 for a list without an element or
 * without an element with mass; out_scores [G, M] = the score bits at elements, a NaN elsewhere.  Every output byte is written whatever
 * count holds.  The reductions run in fp64 and are rounded once; a list's outputs depend on that list alone.
 * Backward, given the forward's lse [G] and scores [G, M] and grad_loss [G]: coef(g, j) = grad_loss[g] scale (p_j - q_j) on elements of
 * valid lists, exactly 0 elsewhere (written to the workspace),
 *   d_users [G, d] = sum_j coef(g, j) rows[ids[g, j], :]      d_rows [P, d] = sum over the elements with ids[g, j] == p of coef(g, j) users[g, :]
 * in ascending (g, j).  entry_keys [E] int64 is the CALLER's: the values ids[g, j] (G M) + (g M + j) of all E elements, sorted ascending
 * (they are distinct: any correct sort gives the same array) — the rows kernel looks its row's entries up in it and never follows a key
 * outside that row's range.  d_rows == NULL skips that launch and needs no keys.  Every byte of d_users and of a given d_rows is written,
 * zeros included.  No floating-point atomics: two calls give the same bits.
 * DIGAT_ERR_ARG: a null required pointer (count; d_rows; entry_keys without d_rows or with E == 0 may be NULL), G < 0, P < 0,
 * temperature not a positive finite number, E outside [0, G M], a workspace that is not 4-byte aligned; DIGAT_ERR_SHAPE: M outside
 * [1, DIGAT_SHORTLIST_MAX_K], d outside [1, DIGAT_LIST_SOFTMAX_MAX_D], G M >= 2^31, P > 2^31; DIGAT_ERR_WORKSPACE: a short workspace —
 * all before any launch.  G == 0 launches nothing forward.  Workspace (backward only; it may hold anything on entry): 4 G M bytes
 * rounded up to 256; 0 for a negative argument.
 * Stream-ordered: one launch forward (one workgroup per list), two backward; no allocation, no host synchronisation, no read of device
 * memory on the host. */
#define DIGAT_LIST_SOFTMAX_MAX_D 512
size_t digat_list_softmax_workspace_bytes(int64_t lists, int m);
int digat_list_softmax_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* teacher, int64_t G,
                           int64_t P, int M, int d, float scale, float temperature, float* out_loss, float* out_lse, int32_t* out_valid,
                           float* out_scores, void* stream);
int digat_list_softmax_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* teacher, int64_t G,
                           int64_t P, int M, int d, float scale, float temperature, const float* lse, const float* scores,
                           const float* grad_loss, const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- pairwise nDCG loss (LambdaRank) over a user's own list (digat_amd.evaluate.list_pairwise / pairwise_scores) ------------------
 * users [G, d] f32, rows [P, d] f32, ids [G, M] int64, count [G] int32 (NULL: M), gain [G, M] f32, discount [M] f64 (the CALLER's table
 * D(rank): evaluate.ndcg_discount — the kernels take no logarithm for it), scale.  Elements and score(g, j) are digat_list_softmax_fwd's;
 * x = fl32(scale * score), widened to double.  digat_list_pairwise_scores_fwd takes scores [G, M] f32 as given, with no users, rows or
 * ids: a slot is an element when j < clamp(count[g], 0, M) and its score is no NaN.  An element is LABELLED when its gain is finite
 * and >= 0 and its x is no NaN; anything else takes part in nothing.  Among the labelled elements r_i = how many order before i under
 * (x descending, slot ascending), t_i = the same under (gain descending, slot ascending).  idcg = sum gain_i discount[t_i],
 * dcg = sum gain_i discount[r_i]; out_valid [G] = idcg > 0, out_ndcg [G] = dcg / idcg.  For every ordered pair of labelled elements
 * with gain_i > gain_j: w_ij = ((gain_i - gain_j) |discount[r_i] - discount[r_j]|) / idcg — a constant — and, with t = x_i - x_j,
 *   out_loss [G]      = sum_pairs w_ij (max(-t, 0) + log1p(exp(-|t|)))
 *   out_lambda [G, M] = scale (- sum_{j: gain_i > gain_j} w_ij / (1 + exp(x_i - x_j)) + sum_{j: gain_j > gain_i} w_ji / (1 + exp(x_j - x_i)))
 * = d loss[g] / d score(g, i).  loss, ndcg and lambda are 0 for an invalid list, lambda is exactly 0 at every slot that is no labelled
 * element; out_scores [G, M] = the score bits at elements, a NaN elsewhere.  Every output byte is written whatever count holds.  All
 * pair arithmetic and all sums run in fp64, in an order fixed by M, count, ids and gain, and are rounded to fp32 once; a list's outputs
 * depend on that list alone; the two forward entries give the same bits when the second is fed the first's out_scores.
 * Backward, given the forward's lambda [G, M] and grad_loss [G]: coef(g, j) = fl32(grad_loss[g] lambda[g, j]) at elements, 0 elsewhere
 * (written to the workspace); d_users [G, d] and d_rows [P, d] are digat_list_softmax_bwd's two sums over coef, in its order, with its
 * entry_keys [E] (the caller's sorted ids[g, j] (G M) + (g M + j) of all E elements); d_rows == NULL skips that launch and needs no
 * keys.  Every byte of d_users and of a given d_rows is written.  No floating-point atomics: two calls give the same bits.
 * DIGAT_ERR_ARG: a null required pointer (count; rows when P == 0; d_rows; entry_keys without d_rows or with E == 0 may be NULL), G < 0, P < 0, E outside
 * [0, G M], a workspace that is not 4-byte aligned; DIGAT_ERR_SHAPE: M outside [1, DIGAT_SHORTLIST_MAX_K], d outside
 * [1, DIGAT_LIST_SOFTMAX_MAX_D], G M >= 2^31, P > 2^31; DIGAT_ERR_WORKSPACE: a short workspace — all before any launch.  G == 0
 * launches nothing forward; P == 0 leaves every slot without an element.  Workspace (backward only; it may hold anything on entry):
 * 4 G M bytes rounded up to 256; 0 for a negative argument.
 * Stream-ordered: one launch forward (one workgroup per list), two backward; no allocation, no host synchronisation, no read of device
 * memory on the host. */
size_t digat_list_pairwise_workspace_bytes(int64_t lists, int m);
int digat_list_pairwise_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, const float* gain,
                            const double* discount, int64_t G, int64_t P, int M, int d, float scale, float* out_loss, float* out_ndcg,
                            int32_t* out_valid, float* out_scores, float* out_lambda, void* stream);
int digat_list_pairwise_scores_fwd(const float* scores, const int32_t* count, const float* gain, const double* discount, int64_t G, int M,
                                   float scale, float* out_loss, float* out_ndcg, int32_t* out_valid, float* out_lambda, void* stream);
int digat_list_pairwise_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                            const float* lambda, const float* grad_loss, const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- diversified top-k: greedy maximal-marginal-relevance selection over a short list (digat_amd.evaluate.mmr_select) ---------
 * Per user g a list: ids [G, M] int64, scores [G, M] f32, count [G] int32 (the entries in use, held inside [0, M]; NULL: M) — the
 * triple digat_topk_segments and digat_dot_topk write.  vectors [N, d] f32, rows taken as they are (callers pass unit rows).
 * Position p of list g is an ELEMENT when p < count[g] and 0 <= ids[g][p] < N; anything else is no element and no read leaves the
 * arrays.  Repeated ids are distinct elements.  sim(i, j) = the fp32 fmaf chain over c = 0 .. d-1 from 0 of the two elements'
 * rows: the bits digat_dot_scores gives for them, symmetric.
 * Selection, t = 0 .. k-1, every element starting with pen = 0: an element is eligible when it is not selected yet and — with
 * max_per_category = q > 0 — fewer than q selected elements share its category[id] (category [N] int32; q == 0: no cap, category
 * is not read and may be NULL).  value = lam * score - mu * pen in fp32, both products and the difference rounded (never an fma);
 * mu is the caller's (float)1 - lam.  The winner is the eligible element with the largest topk_key(value) (digat_topk_segments'
 * order: NaNs last, -0.0 == +0.0), ties to the lowest list position; then pen = fmax(pen, sim(i, winner)) for every element (a NaN
 * similarity leaves pen as it is, a negative one earns nothing).  Selection stops when nothing is eligible.
 * out_count [G] = the elements selected; slots t < count of out_ids / out_scores [G, k] hold the t-th winner's id and its INPUT
 * score bits, slots t >= count hold -1 and -inf: every output byte is written.
 * DIGAT_ERR_ARG: a null ids / scores / vectors / out pointer, G < 0, N < 0, q < 0, q > 0 without category, lam outside [0, 1] (a
 * NaN included); DIGAT_ERR_SHAPE: k outside [1, 128], M outside [1, 128], d outside [1, 2^24], G >= 2^31 — all before any launch.
 * G == 0 returns DIGAT_OK without a launch.  Stream-ordered: one launch on `stream`, one workgroup per user, the Gram of a list
 * never leaves LDS; no allocation, no host synchronisation, no read of device memory on the host.  The workspace is not used
 * (digat_mmr_select_workspace_bytes returns 0; workspace may be NULL). */
size_t digat_mmr_select_workspace_bytes(int64_t users, int m, int k);
int digat_mmr_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const float* vectors, int64_t N, int d,
                     const int32_t* category, int max_per_category, float lam, float mu, int k, int64_t* out_ids, float* out_scores,
                     int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- list quality: what finished lists look like (digat_amd.evaluate.list_quality) -------------------------------------------
 * Per list g: ids [G, k] int64 and count [G] int32 (NULL: k) — what digat_mmr_select, digat_topk_segments and digat_dot_topk write;
 * N news rows.  Position p is an ELEMENT when p < clamp(count[g], 0, k) and 0 <= ids[g][p] < N (digat_mmr_select's rule); a repeated
 * id is one element per position it holds; no read leaves the arrays.  Every output is [G]; the optional parts go by their input:
 *   out_elements (always): the number of elements.
 *   vectors [N, d] f32 -> out_sim_sum (f64) and out_sim_max (f32), over the element pairs p < q of sim(p, q), digat_mmr_select's
 *     Gram (the bits of digat_dot_scores, symmetric): the sum of the entries widened to double — 0.0 with fewer than two elements;
 *     the order of the additions is fixed by the list alone, so a list's value is the same bits from run to run and in any batch;
 *     no float atomics — and their fmax (NaNs are passed over; -inf with fewer than two elements or NaNs alone; a maximum of zero is
 *     +0.0): exact bits.
 *   category [N] int32, any values -> out_categories and out_category_max: the distinct category[id] over the elements, and the
 *     elements of the most frequent one; both 0 without elements.
 *   base_ids [G, kb] int64 with base_count [G] (NULL: kb; elements by the same rule) -> out_overlap: the element positions whose
 *     id is the id of some element position of base list g.
 *   exposure [N] int32, read and written: exposure[id] += 1 per element position, integer atomics (order-free, exact).  The counts
 *     ACCUMULATE across calls: the caller zeroes the array, and keeping the counts inside int32 (fewer than 2^31 element positions
 *     per id between two zeroings) is the caller's concern — nothing here checks it.
 * A part whose input is NULL is not computed and its outputs must be NULL; with the input, its outputs are required.
 * DIGAT_ERR_ARG: a null ids / out_elements, an input without its outputs or outputs without their input, base_count without
 * base_ids, vectors with d < 1, G < 0, N < 0; DIGAT_ERR_SHAPE: k outside [1, 128], kb outside [1, 128] (with base_ids), d > 2^24,
 * G >= 2^31 — all before any launch.  G == 0 returns DIGAT_OK without a launch.  Stream-ordered: one launch on `stream`, one
 * workgroup per list, the Gram never leaves LDS (without vectors none is formed and no dynamic LDS is asked for); no allocation,
 * no host synchronisation, no read of device memory on the host.  The workspace is not used
 * (digat_list_quality_workspace_bytes returns 0; workspace may be NULL). */
size_t digat_list_quality_workspace_bytes(int64_t lists, int k, int kb);
int digat_list_quality(const int64_t* ids, const int32_t* count, int64_t G, int k, int64_t N, const float* vectors, int d,
                       const int32_t* category, const int64_t* base_ids, const int32_t* base_count, int kb, int32_t* exposure,
                       int32_t* out_elements, double* out_sim_sum, float* out_sim_max, int32_t* out_categories, int32_t* out_category_max,
                       int32_t* out_overlap, void* workspace, size_t workspace_bytes, void* stream);

/* ---- calibrated top-k: greedy history-proportional category re-rank of a shortlist (digat_amd.evaluate.calibrated_select) ------
 * Per list g: ids [G, M] int64, scores [G, M] f32, count [G] int32 (NULL: M) — what digat_shortlist_segments / digat_dot_shortlist
 * write, 1 <= M <= DIGAT_CALIBRATE_MAX_LIST; category [N] int32; target [G, C] f32, 1 <= C <= DIGAT_CALIBRATE_MAX_CATEGORIES.
 * Position p is an ELEMENT when p < clamp(count[g], 0, M) and 0 <= ids[g][p] < N (digat_mmr_select's rule; a repeated id is one
 * element per position; no read leaves the arrays).  An element whose category[id] lies outside [0, C) is uncategorised: its gain
 * is 0 and it is never counted.  p_c = (double)target[g][c] where that is finite and > 0, else 0; nothing is normalised.
 * Selection, t = 0 .. k-1, T = t + 1, n_c = the picked elements of category c: in float64, every operation rounded,
 *   q~_c(n) = ((1 - alpha) n) / T + alpha p_c,   gain64_c = p_c (log q~_c(n_c + 1) - log q~_c(n_c))   (0 where p_c = 0),
 * gain32_c = (float)gain64_c; an element's value = lam * score + mu * gain32[category] in fp32, both products and the sum rounded
 * (never an fma); the winner is the unpicked element with the largest value in digat_topk_segments' order (NaNs last,
 * -0.0 == +0.0), ties to the lowest position.  Selection stops when no element is left.  This is the greedy step of
 * lam sum(score) - mu KL(p || q~) with the term common to all candidates dropped.
 * out_count [G] = the elements picked; slots t < count of out_ids / out_scores [G, k] hold the t-th winner's id and its INPUT score
 * bits, slots t >= count hold -1 and -inf; out_kl [G] = (float) sum over c with p_c > 0 of p_c (log p_c - log q~_c(n_c)) at
 * T = max(count, 1), summed in float64 in an order fixed by C alone.  Every output byte is written.  The logarithm is the device
 * library's float64 log: against another correctly implemented log a gain32 may differ by one fp32 step.
 * lam = 1 (mu = 0) and an all-zero target row give the plain top-k of the list, bit for bit.
 * DIGAT_ERR_ARG: a null ids / scores / category / target / out pointer, G < 0, N < 0, lam outside [0, 1], alpha outside (0, 1)
 * (NaNs included); DIGAT_ERR_SHAPE: k outside [1, 128], M outside [1, 1024], C outside [1, 64], G >= 2^31 — all before any launch.
 * G == 0 returns DIGAT_OK without a launch.  Stream-ordered: one launch on `stream`, one workgroup per list (one wave for
 * M <= 128, four beyond), the list in registers; no atomics: the same bits from run to run and in any batch; no allocation, no host synchronisation, no
 * read of device memory on the host.  The workspace is not used (digat_calibrated_select_workspace_bytes returns 0; workspace may
 * be NULL). */
#define DIGAT_CALIBRATE_MAX_LIST 1024
#define DIGAT_CALIBRATE_MAX_CATEGORIES 64
size_t digat_calibrated_select_workspace_bytes(int64_t lists, int m, int c, int k);
int digat_calibrated_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const int32_t* category,
                            int64_t N, const float* target, int C, float lam, float mu, double alpha, int k, int64_t* out_ids,
                            float* out_scores, int32_t* out_count, float* out_kl, void* workspace, size_t workspace_bytes, void* stream);

/* ---- stochastic lists: Plackett-Luce slates with their propensities (digat_amd.evaluate.pl_sample / pl_log_prob) ----------------
 * Per list g: scores [G, M] f32, count [G] int32 (NULL: M) — what digat_shortlist_segments / digat_dot_shortlist write,
 * 1 <= M <= DIGAT_PL_MAX_LIST.  Position p is LIVE when p < clamp(count[g], 0, M) and scores[g][p] is finite (an infinity or a NaN
 * carries no mass and is never drawn; no read leaves the arrays).  inv_t = 1.0 / (double)temperature, computed by the caller.
 * digat_pl_sample draws, per list and sample s = 0 .. samples-1, a slate of n_out = min(k, live positions) positions without
 * replacement from softmax(scores / temperature), 1 <= k <= DIGAT_PL_MAX_K.  In float64, every operation rounded (never an fma):
 *   a_p = (double)x_p * inv_t;   the 64-bit counter e = (stream_g << 32) | ((first_sample + s) << 10 | p) and the word
 *   w = hash32((uint32)e * 0x9E3779B9 + hash32(seed + (uint32)(e >> 32))) — digat_bootstrap_sums' construction —;
 *   u = (w + 0.5) 2^-32 (exact);   key_p = a_p + (-log(-log(u))).
 * stream_g = the low 32 bits of streams[g] (NULL: g).  The slate is the live positions in descending key order, equal keys by
 * ascending position.  Its probability: a_max = the largest live a, w_p = exp(max(a_p - a_max, DIGAT_PL_CLAMP)),
 * Z_t = the sum of w over the live positions not picked before step t, step[t] = max(a_pick(t) - a_max, DIGAT_PL_CLAMP) - log(Z_t),
 * logp = the sum of the steps in slate order.  Z_t is a suffix sum: the unpicked positions reduced in an order fixed by M, then the
 * picked weights added back from the end of the slate — no subtraction.
 * out_picks [G, samples, k] int32: positions, -1 at or beyond n_out; out_n [G] = n_out; out_logp [G, samples] f64 (0 for an empty
 * slate); out_step [G, samples, k] f32 (0 at or beyond n_out).  Every output byte is written.
 * digat_pl_log_prob is the probability stage alone — the same device function — for GIVEN slates picks [G, samples, k]: a slate
 * ends in front of its first entry that is negative, >= M, not live or a repeat of an earlier one.  On digat_pl_sample's picks,
 * scores, count and inv_t it returns digat_pl_sample's out_logp and out_step bit for bit.
 * A draw depends on (seed, stream, sample, position) alone and every order of addition on (M, count, the slate): the same bits from
 * run to run, for a list alone or in a batch, and from a call split by first_sample.  The logarithms and exp are the device
 * library's float64 ones: against another implementation correct to 1 ulp a key moves by a few 2^-52 max(1, |key|)
 * (evaluate.pl_sample_host reports which lists have no nearer pair of keys) and the probabilities stay within evaluate.pl_bound.
 * DIGAT_ERR_ARG: a null scores / picks / out pointer, a misaligned pointer (4 bytes; 8 for out_logp and streams), G < 0, inv_t not
 * positive or inv_t * FLT_MAX not finite (NaNs included); DIGAT_ERR_SHAPE: k outside [1, 128], M outside [1, 1024], G >= 2^31,
 * samples < 1, first_sample < 0, first_sample + samples > DIGAT_PL_MAX_SAMPLE — all before any launch.  G == 0 returns DIGAT_OK
 * without a launch.  Stream-ordered: one workgroup per (list, sample), one launch per 2^23 lists x 65 535 samples; no atomics, no
 * allocation, no host synchronisation, no read of device memory on the host.  The workspace is not used
 * (digat_pl_sample_workspace_bytes returns 0; workspace may be NULL). */
#define DIGAT_PL_MAX_LIST 1024
#define DIGAT_PL_MAX_K 128
#define DIGAT_PL_MAX_SAMPLE (1 << 22)
#define DIGAT_PL_CLAMP (-700.0)
size_t digat_pl_sample_workspace_bytes(int64_t lists, int m, int k, int64_t samples);
int digat_pl_sample(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, uint32_t seed, int64_t samples,
                    int64_t first_sample, const int64_t* streams, int32_t* out_picks, int32_t* out_n, double* out_logp, float* out_step,
                    void* workspace, size_t workspace_bytes, void* stream);
int digat_pl_log_prob(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples, const int32_t* picks,
                      double* out_logp, float* out_step, void* workspace, size_t workspace_bytes, void* stream);

/* ---- doubly robust off-policy value: a logged slate's per-step expectation under the target (digat_amd.evaluate.pl_expect) -------
 * scores, count, G, M, k, inv_t, samples and picks [G, samples, k] are digat_pl_log_prob's, under its rules and limits; out_logp
 * [G, samples] f64 and out_step [G, samples, k] f32 are its outputs bit for bit (the same device function on the same image), and
 * out_len [G, samples] int32 is the length at which the slate was cut.  values [G, M] f32 holds a value per item of the list:
 * v_p = (double)values[g][p] where that float is finite, else 0.  For every step t below the length, with the weights w and Z_t of
 * digat_pl_sample above: out_value [G, samples, k] f32 = the float32 value used at pick t (0 where it is not finite), and
 *   out_mean [G, samples, k] f64 = fl(N_t / Z_t),   N_t = the sum of fl(w_j v_j) over the live positions not picked before step t
 * — the expectation of v under the conditional distribution step t draws from.  N_t is the suffix sum beside Z_t: the unpicked
 * positions reduced in Z_t's order, then fl(w_pick(t) v_pick(t)) added back from the end of the slate; every operation a rounded
 * float64 one, never an fma.  At and beyond the length out_mean and out_value are 0.  Every output byte is written.
 * The same bits from run to run and for a list alone or in a batch; against evaluate.pl_expect_host out_mean stays within
 * evaluate.pl_expect_bound (derived in csrc/digat_pl_expect.inc).  Errors as digat_pl_log_prob, with values and the three further
 * outputs among the pointers (8 bytes for out_mean).  Stream-ordered: one workgroup per (list, slate); no atomics, no allocation,
 * no host synchronisation; the workspace is not used (digat_pl_sample_workspace_bytes). */
int digat_pl_expect(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples, const int32_t* picks,
                    const float* values, double* out_logp, float* out_step, double* out_mean, float* out_value, int32_t* out_len,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- differentiable Plackett-Luce slate likelihood over a user's own list (digat_amd.evaluate.list_pl / pl_scores) -------------
 * users [G, d], rows [P, d], ids [G, M] int64, count [G] int32 (NULL: M) as in digat_list_softmax_fwd: slot (g, j) is an ELEMENT
 * when j < clamp(count[g], 0, M) and 0 <= ids[g, j] < P; 1 <= M <= DIGAT_SHORTLIST_MAX_K, 1 <= d <= DIGAT_LIST_SOFTMAX_MAX_D,
 * G M < 2^31.  picks [G, samples, k] int32: positions into the list, 1 <= k <= DIGAT_PL_MAX_K, samples >= 1.
 * inv_t = fl(scale * fl(1.0 / temperature)) in float64, computed by the caller: scale and temperature enter nowhere else.
 * digat_list_pl_fwd scores every list — out_scores [G, M] f32: digat_dot_scores' bits at elements, NaN elsewhere, as
 * digat_list_softmax_fwd writes them — and runs digat_pl_log_prob's probability stage on them inside the same workgroup: a position is
 * LIVE when it is an element and its score is finite, a_j = (double)score_j * inv_t, a slate ends in front of its first entry that is
 * negative, >= M, not live or a repeat; out_logp [G, samples] f64 and out_step [G, samples, k] f32 are digat_pl_log_prob's bits on
 * (out_scores, count, inv_t, picks).  Every output byte is written whatever count and picks hold.
 * The gradient holds a_max and the clamp constant (exact while no live entry sits on the clamp).  With w_j and Z_t as above,
 * H_t = sum_{u < t} 1 / Z_u and n the slate's length: dlogp/da_j = -w_j H_n (j live, not in the slate), 1 - w_j H_{t+1} (j = pick(t)),
 * 0 (j not live);  coef(g, j) = fl32(inv_t * sum_s grad_logp[g, s] * dlogp_s/da_j), exactly 0 at every slot that is not live.  A slate
 * that is empty or whose grad_logp is 0 contributes nothing.
 * digat_pl_scores_bwd writes coef [G, M] for GIVEN scores [G, M] f32 (live: p < clamp(count[g], 0, M) and the score finite), the
 * gradient of digat_pl_log_prob's out_logp in scores at inv_t = 1 / temperature.
 * digat_list_pl_bwd takes digat_list_pl_fwd's out_scores as scores, writes coef into the workspace [G, M] f32
 * (digat_list_pl_workspace_bytes) and forms digat_list_softmax_bwd's two sums from it, in its order and with its kernels:
 * d_users [G, d] = sum_j coef(g, j) rows[ids[g, j]], d_rows [P, d] (may be NULL) = the sum of coef(g, j) users[g] over the elements
 * with ids[g, j] == p; entry_keys [E] int64 as in digat_list_softmax_bwd.
 * One workgroup per list runs its slates in ascending order: every order of addition is fixed by (M, d, count, ids, the slates), no
 * floating-point atomics — the same bits from run to run and for a list alone or in a batch.  Against evaluate.list_pl_host, out_logp
 * and out_step stay within evaluate.pl_bound and coef within evaluate.list_pl_bound (derived in csrc/digat_list_pl.inc).
 * DIGAT_ERR_ARG: a null users / ids / picks / scores / grad_logp / out pointer (rows may be NULL when P == 0), a misaligned pointer
 * (4 bytes; 8 for ids, out_logp, grad_logp and entry_keys), G < 0, P < 0, inv_t not positive or inv_t * FLT_MAX not finite, E outside
 * [0, G M] or E > 0 without keys, a null workspace with G > 0; DIGAT_ERR_SHAPE: M, d, k outside their ranges, samples < 1,
 * G M >= 2^31, P > 2^31; DIGAT_ERR_WORKSPACE: fewer bytes than digat_list_pl_workspace_bytes(G, M) — all before any launch.
 * G == 0 returns DIGAT_OK without a list launch (digat_list_pl_bwd still zeroes d_rows).  Stream-ordered; no allocation, no host
 * synchronisation. */
size_t digat_list_pl_workspace_bytes(int64_t lists, int m);
int digat_list_pl_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                      const int32_t* picks, int64_t samples, int k, double inv_t, double* out_logp, float* out_step, float* out_scores,
                      void* stream);
int digat_pl_scores_bwd(const float* scores, const int32_t* count, int64_t G, int M, int k, double inv_t, int64_t samples,
                        const int32_t* picks, const double* grad_logp, float* out_grad, void* stream);
int digat_list_pl_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                      const float* scores, const int32_t* picks, int64_t samples, int k, double inv_t, const double* grad_logp,
                      const int64_t* entry_keys, int64_t E, float* d_users, float* d_rows, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- PL-Rank policy gradient of a position-weighted metric over a user's own list (digat_amd.evaluate.list_plrank / plrank_scores) --
 * Lists, elements, live positions, inv_t, a_j = (double)score_j * inv_t, w_j and Z_t are digat_list_pl_fwd's above, under its limits.
 * gain [G, M] f32: rho_j, a NaN, an infinity or a negative value counting as 0; discount [k] f64: theta_t, finite and >= 0;
 * list_weight [G] f64 (NULL: 1).  picks [G, samples, k] int32 GIVEN: every slate is cut by digat_pl_log_prob's rule (a slate cut short
 * is the metric truncated at its length; out_picks is not written and may be NULL).  picks NULL (the two forwards only): slate s of
 * list g is DRAWN as digat_pl_sample draws it — the same device function: the hash of (seed, stream, first_sample + s, position), the
 * Gumbel key, the order, the tie rule, n_out = min(k, live) — from the scores inside the kernel that formed them, and written to
 * out_picks [G, samples, k] (-1 from n_out on); streams [G] int64 (NULL: g), first_sample + samples <= DIGAT_PL_MAX_SAMPLE.
 * For a slate of length n with picks p_0 .. p_{n-1}: r_t = theta_t rho_{p_t}, PR_t = sum_{x >= t} r_x (PR_n = 0),
 * A_t = sum_{u < t} theta_u / Z_u, B_t = sum_{u < t} PR_u / Z_u, and, a_max and the clamp held constant,
 *   c(j) = w_j (rho_j A_n - B_n) (j live, not in the slate);  c(p_t) = PR_{t+1} + w_{p_t} (rho_{p_t} A_{t+1} - B_{t+1});  0 (j not live):
 * the PL-Rank-2 estimator — its mean over the policy's slates is the exact gradient in a of the EXPECTED metric sum_t theta_t rho_{y_t}.
 *   out_slate_value [G, samples] f64 = PR_0;   out_value [G] f64 = list_weight[g] * (sum_s out_slate_value[g, s]) / samples;
 *   coef [G, M] f32 = fl32(inv_t * list_weight[g] * grad_value[g] * (sum_s c_s(j)) / samples), exactly 0 at every slot that is not live.
 * An empty slate adds nothing and still counts in samples; a list whose grad_value is 0 gets zeros.  out_value is the sample mean of
 * the metric; coef is the ESTIMATOR of the gradient of its expectation, not the derivative of that sample mean.
 * digat_list_plrank_fwd scores the lists (out_scores [G, M] f32 as digat_list_pl_fwd writes them) and runs the slates in the same
 * workgroup; digat_plrank_scores_fwd is the same from GIVEN scores [G, M] f32; digat_plrank_scores_bwd writes coef [G, M] alone;
 * digat_list_plrank_bwd writes coef into the workspace (digat_list_plrank_workspace_bytes) and forms digat_list_softmax_bwd's two sums
 * d_users and d_rows (may be NULL) from it, with its kernels and entry_keys — digat_list_pl_bwd's chain.
 * One workgroup per list runs its slates in ascending order: no floating-point atomics, the same bits from run to run and for a list
 * alone or in a batch; out_picks and out_slate_value also from a call split by first_sample.  Against evaluate.plrank_host coef,
 * out_slate_value and out_value stay within evaluate.plrank_bound (derived in csrc/digat_list_plrank.inc).
 * Errors as digat_list_pl_fwd / _bwd, with gain, discount (8 bytes), list_weight (8), streams (8), out_slate_value (8), out_value (8)
 * and grad_value (8) among the pointers; a forward with neither picks nor out_picks is DIGAT_ERR_ARG; first_sample < 0 or
 * first_sample + samples > DIGAT_PL_MAX_SAMPLE is DIGAT_ERR_SHAPE — all before any launch.  G == 0 returns DIGAT_OK without a list
 * launch.  Stream-ordered; no allocation, no host synchronisation. */
size_t digat_list_plrank_workspace_bytes(int64_t lists, int m);
int digat_list_plrank_fwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                          const float* gain, const double* discount, const double* list_weight, const int32_t* picks, int64_t samples, int k,
                          double inv_t, uint32_t seed, int64_t first_sample, const int64_t* streams, int32_t* out_picks,
                          double* out_slate_value, double* out_value, float* out_scores, void* stream);
int digat_plrank_scores_fwd(const float* scores, const int32_t* count, int64_t G, int M, const float* gain, const double* discount,
                            const double* list_weight, const int32_t* picks, int64_t samples, int k, double inv_t, uint32_t seed,
                            int64_t first_sample, const int64_t* streams, int32_t* out_picks, double* out_slate_value, double* out_value,
                            void* stream);
int digat_plrank_scores_bwd(const float* scores, const int32_t* count, int64_t G, int M, const float* gain, const double* discount,
                            const double* list_weight, const int32_t* picks, int64_t samples, int k, double inv_t, const double* grad_value,
                            float* out_grad, void* stream);
int digat_list_plrank_bwd(const float* users, const float* rows, const int64_t* ids, const int32_t* count, int64_t G, int64_t P, int M, int d,
                          const float* scores, const float* gain, const double* discount, const double* list_weight, const int32_t* picks,
                          int64_t samples, int k, double inv_t, const double* grad_value, const int64_t* entry_keys, int64_t E,
                          float* d_users, float* d_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---- joint re-rank: diversity, calibration and a cap per category in one greedy pass (digat_amd.evaluate.rerank_select) ---------
 * Per list g: ids [G, M] int64, scores [G, M] f32, count [G] int32 (NULL: M), 1 <= M <= DIGAT_RERANK_MAX_LIST; vectors [N, d] f32,
 * 1 <= d <= DIGAT_LIST_SOFTMAX_MAX_D (read only when w_div != 0; NULL allowed otherwise); category [N] int32 (NULL allowed when
 * w_cal == 0, max_per_category == 0 and target is NULL); target [G, C] f32, 1 <= C <= DIGAT_CALIBRATE_MAX_CATEGORIES (NULL allowed
 * when w_cal == 0: then no element is categorised and kl is 0).  Position p is an ELEMENT when p < clamp(count[g], 0, M) and
 * 0 <= ids[g][p] < N (digat_mmr_select's rule; no read leaves the arrays).  The weights are finite and >= 0, taken as given.
 * Greedy, steps t = 0 .. k-1, every operation a rounded float32 one, never an fma: rel = w_rel s (once); a = rel - (w_div pen) if
 * w_div != 0, else rel; value = a + red if w_cal != 0, else a, where red = w_cal gain32_c is digat_calibrated_select's for an element
 * categorised in [0, C) and 0 otherwise (the same float64 q_c and logarithms at the same alpha).  The winner is the eligible element
 * with the largest digat_topk_segments key of value, ties to the lowest position; eligible: unpicked and, with max_per_category
 * q > 0, fewer than q picked elements of its raw category[id] (digat_mmr_select's cap).  After a pick: pen = fmax(pen,
 * sim(winner, .)) when w_div != 0, sim the fp32 fmaf chain over ascending channels (digat_dot_scores' bits); n_c += 1 for a
 * categorised winner.  Selection stops when nothing is eligible.  out_scores / out_ids [G, k], 1 <= k <= 128: the picked entries'
 * INPUT scores and ids, -inf / -1 from out_count[g] on; out_kl [G] as digat_calibrated_select writes it (0 without a target).
 * DIGAT_ERR_ARG: a null required pointer, G < 0, N < 0, max_per_category < 0, a weight that is negative or not finite, alpha outside
 * (0, 1); DIGAT_ERR_SHAPE: k outside [1, 128], M outside [1, DIGAT_RERANK_MAX_LIST], d outside [1, DIGAT_LIST_SOFTMAX_MAX_D] with
 * w_div != 0, C outside [1, 64] with a target, G >= 2^31 — all before any launch.  G == 0 returns DIGAT_OK without a launch.
 * Stream-ordered: one launch, one workgroup of 256 threads per list, the list in registers; M <= 128: the list's Gram in LDS
 * (digat_mmr_select's), beyond: one row of it per step formed in LDS; no Gram in memory either way (the route goes by M alone and
 * both give the same bits); no atomics: the same bits from run to run and in any batch; no allocation, no host synchronisation.  The
 * workspace is not used (digat_rerank_select_workspace_bytes returns 0; workspace may be NULL). */
#define DIGAT_RERANK_MAX_LIST 1024
size_t digat_rerank_select_workspace_bytes(int64_t lists, int m, int k);
int digat_rerank_select(const int64_t* ids, const float* scores, const int32_t* count, int64_t G, int M, const float* vectors, int64_t N, int d,
                        const int32_t* category, int max_per_category, const float* target, int C, float w_rel, float w_div, float w_cal,
                        double alpha, int k, int64_t* out_ids, float* out_scores, int32_t* out_count, float* out_kl, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- exposure-capped top-k: a stable assignment of list slots to news under per-news capacities (digat_amd.evaluate.capped_select) --
 * The one stage that works on the batch of lists: every list holds at most k entries, every news id is held at most cap[id] times,
 * and the set held is the list-optimal STABLE assignment (deferred acceptance) — unique, because both orders are strict.  It is not
 * the assignment of largest total score.  ids [G, M] int64, scores [G, M] f32, priority [G, M] f32 (NULL: the scores), count [G]
 * int32 (NULL: M), 1 <= M <= DIGAT_CAPPED_MAX_LIST, G M < 2^31, P < 2^31 news.  Pair (g, j) is an ELEMENT when j < clamp(count[g],
 * 0, M), 0 <= ids[g][j] < P, scores[g][j] is neither NaN nor -inf and priority[g][j] is no NaN; a list that names an id twice has two
 * pairs, each one in its own right.  A list orders its elements by the digat_topk_segments key of the score, descending, then slot
 * ascending; an item orders the pairs that name it by the key of the priority, descending, then g, then slot ascending.
 * Round-wise (digat_amd.evaluate.capped_select_host is the definition): rejected starts as the non-elements; in a round every list
 * demands its first k non-rejected entries, then every item walks its pairs in its order and rejects every pair from the one behind
 * its cap-th demanded pair on (cap 0: all of them), demanded or not; the first round that rejects nothing ends the loop and its
 * demand sets are the result.  Rejections are permanent; a round past the fixed point changes nothing.  Three entries share the
 * workspace of digat_capped_select_workspace_bytes(G, M) bytes (8-byte aligned; it carries the state from entry to entry, so it
 * must not be touched in between — except as said here):
 *   digat_capped_prepare  the element test and every list's order.  It leaves the item words [G M] int64, pair g M + j at index
 *       g M + j, at the START of the workspace: (id << 32) | ~key(priority) for an element, 0x7fffffffffffffff otherwise.  The CALLER
 *       sorts them (stable: equal words keep index order) and hands the permutation on.
 *   digat_capped_rounds   `rounds` rounds, two launches each.  perm [G M] int32: the pair indices in sorted word order; the
 *       segments that can bind (more pairs than capacity — no other can ever reject): seg_begin [n_seg] int32 where the news' run
 *       starts in perm, seg_cap [n_seg] int32 its capacity, seg_live [n_seg] int32 its length on entry of the first round —
 *       updated in place, hand the same array to the next call.  counter [rounds] int32, ZEROED by the caller: counter[r] += the
 *       pairs round r newly rejected (one integer atomic per wave; the sum is exact).  n_seg == 0: the lists' launch alone.
 *   digat_capped_emit     the demand sets of the state as it stands: out_ids / out_scores (the INPUT bits) / out_slots [G, k] in
 *       the list's order, -1 / -inf / -1 from out_count[g] on.  1 <= k <= 128.
 * DIGAT_ERR_ARG: a null required pointer, a negative size, a workspace that is not 8-byte aligned; DIGAT_ERR_SHAPE: M, k, G M, P or
 * n_seg beyond the limits; DIGAT_ERR_WORKSPACE: a short workspace — all before any launch.  G == 0 returns DIGAT_OK without a launch.
 * Every index read from perm / seg_* is checked against G M before it is used.  Integer and comparison work only: the same bits
 * from run to run; no cooperative launch, no grid-wide wait; no allocation, no host synchronisation (the caller reads counter). */
#define DIGAT_CAPPED_MAX_LIST 1024
size_t digat_capped_select_workspace_bytes(int64_t lists, int m);
int digat_capped_prepare(const int64_t* ids, const float* scores, const float* priority, const int32_t* count, int64_t G, int M, int64_t P,
                         void* workspace, size_t workspace_bytes, void* stream);
int digat_capped_rounds(int64_t G, int M, int k, const int32_t* perm, const int32_t* seg_begin, const int32_t* seg_cap, int32_t* seg_live,
                        int64_t n_seg, int32_t* counter, int rounds, void* workspace, size_t workspace_bytes, void* stream);
int digat_capped_emit(const int64_t* ids, const float* scores, int64_t G, int M, int k, int64_t* out_ids, float* out_scores,
                      int32_t* out_count, int32_t* out_slots, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bootstrap resampling of per-unit metric rows (digat_amd.evaluate.bootstrap_sums / metric_intervals / compare_metrics) -----
 * values [n, c] float64 row-major: one row per resampling unit (an impression, a user), one column per summed quantity;
 * sums [B, c] float64.  Replicate r = first_replicate + b makes n draws with replacement; draw j has the 64-bit counter
 * e = r n + j, the word w = hash32((uint32)e * 0x9E3779B9 + hash32(seed + (uint32)(e >> 32))) — the dropout hash's construction, the
 * seed used as given — and the unit idx = (w n) >> 32 (64-bit product; idx < n always; idx is uniform up to a bias of at most
 * n / 2^32); sums[b, :] = sum over j of values[idx_j, :].  ONE index per draw serves every column: the columns of two models side by
 * side are resampled as pairs.  evaluate.bootstrap_draws_host restates the draws bit for bit.
 * Determinism: the order in which a replicate's n terms are added is fixed by n alone — not by B, first_replicate, c, the grid or
 * the other columns — and no floating-point atomics are used, so sums[b, k] depends on column k, n, seed and r only: the same bits
 * from run to run, from a call split by first_replicate, and from the columns split over two calls.  Against the correctly rounded
 * sum of the same draws an entry is off by at most n 2^-53 sum_j |values[idx_j, k]|; integer-valued data below 2^53 is exact.
 * Limits: 1 <= n <= 2^31 - 1, 1 <= c <= DIGAT_BOOTSTRAP_MAX_COLUMNS, B >= 0, first_replicate >= 0, first_replicate + B <= 2^31
 * (every counter stays below 2^62).  DIGAT_ERR_ARG: a null or not 8-byte-aligned values / sums (an odd workspace address too),
 * n < 1, c < 1, B < 0, first_replicate < 0; DIGAT_ERR_SHAPE: n, c or first_replicate + B beyond the limits; DIGAT_ERR_WORKSPACE:
 * fewer than digat_bootstrap_workspace_bytes(n, c, B) bytes — all before any HIP call.  B == 0 returns DIGAT_OK without a launch.
 * The draws are cut into slices of DIGAT_BOOTSTRAP_SLICE; one workgroup per (slice, replicate) sums its slice in registers; with
 * more than one slice the partial sums [B, slices, c] go through the workspace (8 B ceil(n / DIGAT_BOOTSTRAP_SLICE) c bytes, it may
 * hold anything on entry; 0 bytes and workspace may be NULL for n <= DIGAT_BOOTSTRAP_SLICE) and a second launch adds a replicate's
 * slices in ascending order.  Stream-ordered: one or two launches per 65 535 replicates on `stream`; no allocation, no host
 * synchronisation, no read of device memory on the host.  digat_bootstrap_workspace_bytes returns 0 for arguments outside the limits. */
#define DIGAT_BOOTSTRAP_MAX_COLUMNS 16
#define DIGAT_BOOTSTRAP_SLICE 8192
size_t digat_bootstrap_workspace_bytes(int64_t n, int c, int64_t B);
int digat_bootstrap_sums(const double* values, int64_t n, int c, int64_t B, int64_t first_replicate, uint32_t seed, double* sums,
                         void* workspace, size_t workspace_bytes, void* stream);

/* out[u, :] = the sum of the rows start[u] .. start[u + 1] - 1 of values [rows, columns] float64, added left to right by one thread
 * per (unit, column): row-level values turned into resampling units (a user's impressions, a user's targets).  start [units + 1]
 * int64 on the device, non-decreasing from 0 to rows (the caller's concern; the kernel clamps what it reads to [0, rows], so no read
 * leaves the table); an empty unit gives 0.0.  evaluate.segment_sums_host adds in the same order: the same bits.
 * DIGAT_ERR_ARG: a null start / out (values too unless rows == 0), a pointer that is not 8-byte aligned, rows < 0, columns < 1,
 * units < 0; DIGAT_ERR_SHAPE: columns > 2^20 or units x columns > 2^38 — before any HIP call.  units == 0 returns without a launch.
 * Stream-ordered: one launch, no workspace. */
int digat_segment_sums_f64(const double* values, int64_t rows, int columns, const int64_t* start, int64_t units, double* out,
                           void* stream);

/* ---- vanilla-GAT update layer of the ablation encoders -----------------------------------------
 * graphEncoders.py:493-519 (wo_interaction), :641-651 (News_graph_wo_inter), :788-798 (User_graph_wo_inter), eval mode:
 * h = X W^T + bW; e_ij = leaky_relu_0.2(a1.h_j + a2.h_i); -1e9 where A_ij = 0; alpha = softmax_j; out = relu(alpha h) + X.
 * X, out [B,n,d]; A [B,n,n] bytes; W [d,d], bW [d] or NULL, a1, a2 [d].
 * DIGAT_ERR_SHAPE, before any launch and from all three entries: d % 4 != 0, d > 1024 or n > DIGAT_MAX_NODES. */
size_t digat_gat_workspace_bytes(int B, int n, int d);
int digat_gat_fwd(const float* X, const uint8_t* A, const float* W, const float* bW, const float* a1, const float* a2,
                  float* out, int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream);
/* The same layer in training mode (dropout live: graphEncoders.py:495 on the input is the caller's, :500 on alpha is
 * p_alpha here), one call per direction like digat_xattn_fwd_train / digat_xattn_bwd: `save` carries h, alpha, the scores
 * before leaky_relu and the dropout mask from the forward to the backward.  dX, dW, dbW, da1, da2 are written, not
 * accumulated; sums run in index order (bit-reproducible). */
size_t digat_gat_train_save_bytes(int B, int n, int d);
size_t digat_gat_train_workspace_bytes(int B, int n, int d);
int digat_gat_fwd_train(const float* X, const uint8_t* A, const float* W, const float* bW, const float* a1, const float* a2, float* out,
                        float p_alpha, uint32_t seed, int B, int n, int d, void* save, size_t save_bytes, void* workspace,
                        size_t workspace_bytes, void* stream);
int digat_gat_bwd(const float* dOut, const float* out, const float* X, const uint8_t* A, const float* W, const float* a1, const float* a2,
                  float p_alpha, const void* save, size_t save_bytes, float* dX, float* dW, float* dbW, float* da1, float* da2,
                  int B, int n, int d, void* workspace, size_t workspace_bytes, void* stream);

/* ---- semantic-augmented-graph construction: construct_SAG.py ------------------------------------
 * generate_cos_similarities (construct_SAG.py:112-162), one category: title/content [n, dim], corpus_title/corpus_content
 * [m, dim] fp32 sentence embeddings; k = min(top_M, m - 1) + 1 <= 32, dim % 16 == 0.  values / indices [5, n, k]
 * (fp32 / int32), kinds in the reference's return order: title-title, content-content, title-content (title query vs
 * corpus contents), content-title, and the mean of the four; every row sorted descending as torch.topk returns it
 * (equal values: lower corpus index first). */
size_t digat_sag_cos_topk_workspace_bytes(int64_t n, int64_t m, int dim);
int digat_sag_cos_topk(const float* title, const float* content, int64_t n, const float* corpus_title, const float* corpus_content,
                       int64_t m, int dim, int k, float* values, int32_t* indices, void* workspace, size_t workspace_bytes,
                       void* stream);
/* generate_similar_news_list (construct_SAG.py:303-320), the average kind, for one category, fused behind the same cosine
 * GEMM: the n query rows and m corpus rows are GROUPS of news with one title (news_dict_inv); group_start [n + 1] /
 * group_member and corpus_start [m + 1] / corpus_member are CSR tables of their news rows (corpus: first member = the
 * group's representative, every group non-empty).  M' = min(top_M, m - 1), k = M' + 1 <= 32.  For every member news x of
 * query group g, the k best corpus groups by the mean of the four cosines (digat_sag_cos_topk's kind 4, bit for bit) are
 * walked in order; one that holds x itself is skipped, the others append (representative, cosine) to row x of sim_index /
 * sim_cos [news_num, top_M] until M' are written (M' = 0: the stop test never fires, as in the reference, and the one entry
 * is written unless skipped); sim_len[x] = the count.  Rows of news in no group of the call are not touched.  The tables
 * are not validated here: every member row must lie in [0, news_num).  Workspace: that of digat_sag_cos_topk. */
size_t digat_sag_similar_lists_workspace_bytes(int64_t n, int64_t m, int dim);
int digat_sag_similar_lists(const float* title, const float* content, int64_t n, const float* corpus_title, const float* corpus_content,
                            int64_t m, int dim, int top_M, const int32_t* group_start, const int32_t* group_member,
                            const int32_t* corpus_start, const int32_t* corpus_member, int32_t* sim_index, float* sim_cos,
                            int32_t* sim_len, int64_t news_num, void* workspace, size_t workspace_bytes, void* stream);
/* generate_news_graph (construct_SAG.py:449-485): sim_index / sim_cos [news_num, top_M] = every news's similar-news list
 * (news indices, cosines; sim_len [news_num] entries are valid), hop, news_node_num <= 256, threshold = the reference's
 * similarity_threshold (0.5, :10).  Outputs (all rewritten): news_node_ID [news_num, nn] int32, news_graph
 * [news_num, nn, nn] bytes, news_graph_mask [news_num, nn] bytes.  *overflow (device int32) is set to 1 when a walk needs
 * more than news_node_num nodes (the reference raises IndexError there). */
int digat_sag_news_graph(const int32_t* sim_index, const float* sim_cos, const int32_t* sim_len, int64_t news_num, int top_M, int hop,
                         int news_node_num, float threshold, int32_t* news_node_ID, uint8_t* news_graph, uint8_t* news_graph_mask,
                         int32_t* overflow, void* stream);

/* ---- news encoder (upstream of the path): newsEncoders.MSA.forward in eval mode ------------------
 * newsEncoders.py:70-82 with layers.MultiHeadAttention (layers.py:50-88) and layers.Attention (:91-115).
 * title_text [T, Lw] int32 token ids (rows of word_embedding), title_mask [T, Lw] bytes (0 = padding: masked only in
 * the pooling, as in the reference), out [T, head_num * head_dim].  Lw <= 64, head_dim <= 32.  Titles of 33..64 words take up
 * to 132 096 bytes of dynamic LDS per workgroup (every shape of the contract fits the CU's 160 KiB); DIGAT_ERR_LAUNCH if the
 * runtime does not grant the size.
 * qkv_wsplit: [W_Q|W_K|W_V] split by digat_split_proj_weights-style call digat_split_msa_weights (optional: NULL =
 * fp32 MFMA path with a materialised embedding gather). */
typedef struct digat_msa_params {
    int32_t word_embedding_dim, head_num, head_dim, attention_dim;
    const float *word_embedding;                 /* word_embedding.weight [V, word_embedding_dim]            */
    const float *W_Q, *b_Q, *W_K, *W_V, *b_V;    /* multiheadSelfattention.W_{Q,K,V}.{weight,bias}            */
    const float *A1, *b1, *a2;                   /* attention.affine1.{weight,bias}, attention.affine2.weight */
    const void  *qkv_wsplit;                     /* digat_split_msa_weights output, or NULL                   */
    const void  *a1_wsplit;                      /* digat_split_weights(affine1.weight, attention_dim, hd) output, or NULL */
} digat_msa_params;
size_t digat_msa_split_bytes(int word_embedding_dim, int head_num, int head_dim);
int digat_split_msa_weights(const float* W_Q, const float* W_K, const float* W_V, int word_embedding_dim, int hd,
                            void* wsplit, void* stream);
size_t digat_msa_workspace_bytes(int T, int Lw, int word_embedding_dim, int head_num, int head_dim, int attention_dim);
int digat_msa_fwd(const digat_msa_params* params, const int32_t* title_text, const uint8_t* title_mask, float* out,
                  int T, int Lw, void* workspace, size_t workspace_bytes, void* stream);
/* The same encoder in training mode (newsEncoders.py:70-82 with dropout live), one call per direction.  p_drop is the dropout
 * on the embedded tokens (:77).  `save` carries the dropped embeddings, Q|K|V, h, the affine1 product and the pooling weights to the
 * backward; the attention scores are recomputed there.  The *_wsplit fields of params are ignored (the weights change every
 * optimiser step: they are split inside, into the workspace).  Lw <= 32, attention_dim % 4 == 0.
 * digat_msa_bwd writes (does not accumulate) row_grad [T*Lw, word_embedding_dim], rows ld_row_grad floats apart
 * (word_embedding_dim, or digat_msa_row_grad_ld(): padded to a multiple of 80 so that one matrix-core product computes it) — the
 * gradient at the embedding rows the tokens looked up — and dW_Q dW_K dW_V [hd, word_embedding_dim], db_Q db_V [hd], dA1 [attention_dim, hd], db1 da2 [attention_dim].
 * digat_embedding_bwd sums row_grad per token into table_grad [V, word_embedding_dim] (zero-filled by the caller) in a fixed
 * order — bit-reproducible, no atomics: `order` [M] = the row indices stably sorted by token, sorted_tokens [M] the tokens in that order. */
size_t digat_msa_train_save_bytes(int T, int Lw, int word_embedding_dim, int head_num, int head_dim, int attention_dim);
size_t digat_msa_train_workspace_bytes(int T, int Lw, int word_embedding_dim, int head_num, int head_dim, int attention_dim);
int digat_msa_fwd_train(const digat_msa_params* params, const int32_t* title_text, const uint8_t* title_mask, float* out, float p_drop,
                        uint32_t seed, int T, int Lw, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes,
                        void* stream);
int digat_msa_bwd(const digat_msa_params* params, const int32_t* title_text, const uint8_t* title_mask, const float* dout, float p_drop,
                  const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW_Q, float* db_Q, float* dW_K,
                  float* dW_V, float* db_V, float* dA1, float* db1, float* da2, int T, int Lw, void* workspace, size_t workspace_bytes,
                  void* stream);
int64_t digat_msa_row_grad_ld(int T, int Lw, int word_embedding_dim);
size_t digat_embedding_bwd_workspace_bytes(int64_t M, int dm);
int digat_embedding_bwd(const float* row_grad, int64_t ld_row_grad, const int32_t* order, const int32_t* sorted_tokens, int64_t M, int dm,
                        float* table_grad, void* workspace, size_t workspace_bytes, void* stream);
/* The same sum for a few thousand looked-up rows without a sorted order (the backward of torch.nn.functional.embedding on a wide
 * table, trainer.py:98-102 through the news encoder's table): ids0 [M0] / ids1 [M1] int64 (two lookups of ONE table; ids1 may be NULL
 * with M1 = 0), their row gradients g0 / g1 (row strides ld0 / ld1); table_grad [V, dm] zero-filled by the caller; an id outside
 * [0, V) receives nothing.  Two launches (and a memset of 8 V bytes): per chunk of 64 positions the first position of an id adds the
 * chunk's rows of that id in ascending order, then the first position overall adds those partial rows in ascending chunk order —
 * bit-reproducible (the only atomics are an integer min and an integer count per id).
 * dm % 4 == 0, dm <= 1024, M0 + M1 <= 2^24 (the id scans are quadratic in M: meant for M of a few thousand). */
size_t digat_embedding_bwd_unsorted_workspace_bytes(int64_t M, int dm, int64_t V);
int digat_embedding_bwd_unsorted(const int64_t* ids0, const float* g0, int64_t ld0, int64_t M0, const int64_t* ids1, const float* g1,
                                 int64_t ld1, int64_t M1, int dm, int64_t V, float* table_grad, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ---- key-masked multi-head self-attention encoder: the NRMS / NRMS-SA baselines (the reference's Appendix-B) --------------------
 * Appendix-B/layers.py:79-95 MultiHeadAttention.forward WITH its key mask and without a ReLU, then layers.Attention: the news encoder
 * (newsEncoders.py:46-58: rows of the word embedding, title mask = key mask = pooling mask) and the user encoder (userEncoders.py:44-47:
 * rows of the news representations, history mask = key mask, pooling unmasked) are one entry.
 * `table` [V, in_dim] with ids [T, L] int32 (the lookup rides on the projection's row list where its kernel takes one), or ids == NULL
 * and `table` = dense rows [T*L, in_dim].  mask [T, L] bytes, 0 = masked key: its score reads -1e9 for every query row, after the
 * scale; a sequence without a live key therefore attends uniformly over all L positions and passes no gradient to its scores.
 * out [T, head_num * head_dim].  L <= 64, head_dim <= 128 (fp32 matrix cores up to 32, a plain fp32 kernel above), in_dim % 4 == 0,
 * head_num * head_dim % 4 == 0.  The split images are digat_split_msa_weights / digat_split_weights outputs, as in digat_msa_params. */
#define DIGAT_MHSA_POOL_UNMASKED 1               /* flags: the pooling softmax runs over all L positions (the user encoder) */
typedef struct digat_mhsa_params {
    int32_t in_dim, head_num, head_dim, attention_dim;
    const float *table;                          /* [V, in_dim] looked up by ids, or the dense input rows       */
    const float *W_Q, *b_Q, *W_K, *W_V, *b_V;    /* multiheadAttention.W_{Q,K,V}.{weight,bias}                  */
    const float *A1, *b1, *a2;                   /* attention.affine1.{weight,bias}, attention.affine2.weight   */
    const void  *qkv_wsplit;                     /* digat_split_msa_weights output, or NULL                     */
    const void  *a1_wsplit;                      /* digat_split_weights(affine1.weight, attention_dim, hd) output, or NULL */
    int32_t flags, reserved;
} digat_mhsa_params;
size_t digat_mhsa_workspace_bytes(int T, int L, int in_dim, int head_num, int head_dim, int attention_dim);
int digat_mhsa_fwd(const digat_mhsa_params* params, const int32_t* ids, const uint8_t* mask, float* out, int T, int L,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Training, one call per direction.  p_in: dropout on the input rows (site 1: the counter hash of `seed` over the [T*L, in_dim]
 * elements), p_ctx: on the attention's output (site 2: `seed + 1` over the [T*L, hd] elements, applied in the attention kernel; the
 * backward regenerates its keep bits).  `save` carries the dropped input rows, Q|K|V, the attention output, the affine1 product and
 * the pooling weights; scores and attention weights are recomputed in the backward.  attention_dim % 4 == 0.  The *_wsplit fields
 * are ignored.  digat_mhsa_bwd writes (does not accumulate) row_grad [T*L, in_dim], rows ld_row_grad floats apart (in_dim, or
 * digat_msa_row_grad_ld(T, L, in_dim)) — feed it to digat_embedding_bwd; for dense input it is dX — and the weight gradients as
 * digat_msa_bwd does. */
size_t digat_mhsa_train_save_bytes(int T, int L, int in_dim, int head_num, int head_dim, int attention_dim);
size_t digat_mhsa_train_workspace_bytes(int T, int L, int in_dim, int head_num, int head_dim, int attention_dim);
int digat_mhsa_fwd_train(const digat_mhsa_params* params, const int32_t* ids, const uint8_t* mask, float* out, float p_in, float p_ctx,
                         uint32_t seed, int T, int L, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);
int digat_mhsa_bwd(const digat_mhsa_params* params, const int32_t* ids, const uint8_t* mask, const float* dout, float p_in, float p_ctx,
                   uint32_t seed, const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW_Q, float* db_Q,
                   float* dW_K, float* dW_V, float* db_V, float* dA1, float* db1, float* da2, int T, int L, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The middle stage alone.  qkv [T*L, 3*hd] (Q | K | V per row), h [T*L, hd] = dropout_{p_ctx}(softmax(mask(Q K^T / sqrt(d_k))) V), keep
 * bits of `seed` over the [T*L, hd] elements (p_ctx = 0: none); the backward takes dh (the gradient at h) and writes dqkv [T*L, 3*hd]. */
int digat_mhsa_attention_fwd(const float* qkv, const uint8_t* mask, float* h, float p_ctx, uint32_t seed, int T, int L, int head_num,
                             int head_dim, void* stream);
int digat_mhsa_attention_bwd(const float* qkv, const uint8_t* mask, const float* dh, float* dqkv, float p_ctx, uint32_t seed, int T, int L,
                             int head_num, int head_dim, void* stream);

/* ---- CNN news encoder (newsEncoders.py:29-54, layers.Conv1D :7-47, layers.Attention :91-115) ---------------------------------
 * out[t] = attention_pool(dropout_2(relu(conv1d(dropout_1(word_embedding[title_text[t]])) + b))): the convolution zero-pads
 * (taps - 1) / 2 positions at both ends of each title; padding tokens are looked up like any other.  taps odd, 1..7; `group3`
 * (windows 1, 3, 5 on a third of the kernels each) is the 5-tap convolution whose weights are zero where a branch has no tap:
 * digat_cnn_merge_group3 builds W [Kc][dm][5] and b [Kc] from the three branches.  word_embedding_dim % 4 == 0, kernel_num % 4 == 0,
 * Lw <= 64 (inference), <= 32 and attention_dim % 4 == 0 (training).
 * w_split: digat_split_cnn_weights output (digat_cnn_split_bytes bytes) — the matrix-core kernel's bf16x6 weight image; NULL, fewer
 * than 2 048 token rows or Lw < 16: a plain fp32 kernel of the same semantics.  a1_wsplit as in digat_msa_params. */
typedef struct digat_cnn_params {
    int32_t word_embedding_dim, kernel_num, taps, attention_dim;
    const float *word_embedding;                 /* word_embedding.weight [V, word_embedding_dim]            */
    const float *W, *b;                          /* conv weight [kernel_num][word_embedding_dim][taps] (torch's Conv1d layout), bias */
    const float *A1, *b1, *a2;                   /* attention.affine1.{weight,bias}, attention.affine2.weight */
    const void  *w_split;                        /* digat_split_cnn_weights output, or NULL                   */
    const void  *a1_wsplit;                      /* digat_split_weights(affine1.weight, attention_dim, kernel_num) output, or NULL */
} digat_cnn_params;
size_t digat_cnn_split_bytes(int word_embedding_dim, int kernel_num, int taps);
int digat_split_cnn_weights(const float* W, int word_embedding_dim, int kernel_num, int taps, void* w_split, void* stream);
int digat_cnn_merge_group3(const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                           int word_embedding_dim, int kernel_num, float* W, float* b, void* stream);
size_t digat_cnn_workspace_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim);
int digat_cnn_fwd(const digat_cnn_params* params, const int32_t* title_text, const uint8_t* title_mask, float* out, int T, int Lw,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Training, one call per direction.  p_drop is the rate of both dropouts; their keep bits come from the library's counter hash: site 1
 * (embedded tokens) of `seed` over the [T*Lw, word_embedding_dim] elements, site 2 (after the ReLU) of `seed + 1` over the
 * [T*Lw, kernel_num] elements.  `save` carries h (after site 2), the affine1 product and the pooling weights; the backward regenerates
 * site 1's bits.  The *_split fields of params are ignored (the weights are split inside, into the workspace).
 * digat_cnn_bwd writes (does not accumulate) row_grad [T*Lw, word_embedding_dim], rows ld_row_grad floats apart (>= word_embedding_dim,
 * a multiple of 4) — feed it to digat_embedding_bwd — and dW [kernel_num][word_embedding_dim][taps], db [kernel_num],
 * dA1 [attention_dim, kernel_num], db1 da2 [attention_dim]. */
size_t digat_cnn_train_save_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim);
size_t digat_cnn_train_workspace_bytes(int T, int Lw, int word_embedding_dim, int kernel_num, int taps, int attention_dim);
int digat_cnn_fwd_train(const digat_cnn_params* params, const int32_t* title_text, const uint8_t* title_mask, float* out, float p_drop,
                        uint32_t seed, int T, int Lw, void* save, size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);
int digat_cnn_bwd(const digat_cnn_params* params, const int32_t* title_text, const uint8_t* title_mask, const float* dout, float p_drop,
                  uint32_t seed, const void* save, size_t save_bytes, float* row_grad, int64_t ld_row_grad, float* dW, float* db, float* dA1,
                  float* db1, float* da2, int T, int Lw, void* workspace, size_t workspace_bytes, void* stream);

/* ---- runs of identical consecutive user rows (drop-in path) -------------------------------------------------------------------
 * The reference's driver hands Model.inference the user tensors EXPANDED per row — an impression's history embeddings, user graph,
 * category mask and indices repeated once per candidate (util.py:57-67, model.py:87-90) — so consecutive rows are bit-identical
 * runs.  This finds them on the device: row b belongs to the run of row b - 1 iff EVERY byte of its four user tensors is equal
 * (ue [B,H,d] f32, Au [B,U,U] u8, cat_mask [B,C1] u8, cat_idx [B,H] i64).  row_group[b] = index of row b's run (ascending, runs are
 * consecutive: the layout digat_encoder_fwd_grouped's layer 0 exploits), leaders[g] = first row of run g (int64), *n_runs = G.
 * workspace: B bytes.  DIGAT.inference reads *n_runs (one host synchronisation), gathers the leaders' user tensors and calls the
 * grouped entry when 4 G <= B: bit-identical to digat_encoder_fwd on the expanded rows. */
int digat_user_row_runs(const float* ue, const uint8_t* Au, const uint8_t* cat_mask, const int64_t* cat_idx, int B, int H, int U, int C1, int d,
                        int32_t* row_group, int64_t* leaders, int32_t* n_runs, void* workspace, size_t workspace_bytes, void* stream);

/* digat_encoder_fwd with the search for shared users INSIDE (DIGAT.inference's default; round 5): the same per-row arguments as
 * digat_encoder_fwd (graphEncoders.py:189-198) — the reference's driver expands an impression's user tensors once per candidate
 * (util.py:57-67) — and layer 0 of the user graph computed once per RUN of identical consecutive rows: the runs are found on the
 * device (every byte of the four user tensors compared with the previous row's), every count stays there (no host read), the
 * group-level data of a run lives in its leading row's slots of the full-size buffers.  Bit-identical to digat_encoder_fwd; rows
 * that share nothing cost the comparison pass (B x 85 KB read once) on top of it.  Needs the folded inference path and the sparse
 * Eq. 8 variant of the user graph (flags), else it IS digat_encoder_fwd.  c_n0 may be NULL (forward). */
size_t digat_encoder_shared_workspace_bytes(int B, int N, int H, int C, int d, int depth);
int digat_encoder_fwd_shared(const digat_params* p, const float* Xn_in, const uint8_t* An, const uint8_t* Mn, const float* ue,
                             const uint8_t* Au, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n0, float* out_news,
                             float* out_user, int B, int N, int H, void* workspace, size_t workspace_bytes, void* stream);

/* ---- batch assembly (the device-side counterpart of MIND_dataset.py's __getitem__ + collate) ------------------
 * All table gathers of one scoring batch in one launch.  Job k copies `rows` rows of `row_bytes` bytes: dst row r = src row
 * idx[r] (idx2 == NULL, inner = 1) or src row idx2[idx[r / inner] * inner + r % inner] (two-level: e.g. the representation of
 * the r % H-th history item of impression idx[r / H], idx2 = the [impressions, H] history table).  `jobs` is a HOST array
 * (njobs <= 24), copied into the launch; every pointer inside is a device pointer. */
typedef struct digat_gather_job {
    const void* src; void* dst;
    int64_t row_bytes, rows;
    const int64_t* idx; const int64_t* idx2;
    int64_t inner;
} digat_gather_job;
int digat_gather_tables(const digat_gather_job* jobs, int njobs, void* stream);

/* ---- user graphs from category indices (the device-side counterpart of MIND_corpus.py:145-176) --------------------------------
 * The user graph [U, U] (U = H + C) and the category mask [C + 1] of an impression are a pure function of its H category
 * indices: slot t is valid iff 0 <= idx[t] < C (the padding bucket C, negatives and larger values are padding; valid slots need
 * not form a prefix), present[c] iff some valid slot has idx[t] == c, and
 *   A[i][j] (i, j < H) = i == j, or both valid and idx[i] == idx[j];   A[i][H+c] = A[H+c][i] = slot i valid and idx[i] == c;
 *   A[H+a][H+b] = a == b, or present[a] and present[b];   mask[c] = present[c] for c < C, mask[C] = 0.
 * Graph g is built from row rows[g] of the [I, H] table cat_idx (any order, repeats allowed; the caller keeps rows[g] in [0, I)),
 * or from row g of a [G, H] cat_idx when rows == NULL.  graph [G, U, U] and cat_mask [G, C + 1]: every byte is written, 0 or 1.
 * entries (optional) [G]: the number of set bytes of graph g.  One launch on `stream`; no allocation, no synchronisation (safe
 * under stream capture).  DIGAT_ERR_SHAPE unless 1 <= H, 1 <= C, H + C <= DIGAT_MAX_NODES; G == 0 returns without a launch. */
int digat_user_graph_build(const int64_t* cat_idx, const int64_t* rows, long G, int H, int C, uint8_t* graph, uint8_t* cat_mask,
                           int32_t* entries, void* stream);

/* ---- training input on the device (the counterpart of MIND_dataset.py:26-47 and of its __getitem__ + collate in training) ------
 * digat_negative_sample: an epoch's samples.  Behaviour i has the clicked news click[i] and the non-clicked pool
 * pool[pool_offsets[i] .. pool_offsets[i+1]) (CSR, pool_offsets [n+1] non-decreasing) of size m; samples [n, 1+K]:
 *   samples[i][0] = click[i];   1 <= m <= K: samples[i][1+j] = pool_i[j % m] (the reference's cyclic rule);
 *   m > K: K distinct members of the pool in draw order, every ordered K-subset equally likely (a partial Fisher-Yates shuffle
 *   with exactly K draws; the multiply-shift map of a 32-bit word onto the remaining positions is biased by at most m / 2^32);
 *   m == 0: every column is click[i] (defined; the reference drops such behaviours before it samples).
 * A draw is a pure function of (seed, epoch, i, draw number) through the dropout path's counter hash, so the result does not
 * depend on the launch shape (digat_amd/train_input.py: negative_samples_host restates it bit for bit).  One launch on `stream`,
 * no allocation, no synchronisation.  DIGAT_ERR_ARG: a null pointer, n < 0, K < 1; DIGAT_ERR_SHAPE: K > 16; n == 0 returns
 * without a launch.
 * digat_train_batch_ids: the index lists of a step.  Batch row b is behaviour order[b] (order: a device pointer into the
 * epoch's permutation, B entries read) of the n behaviours impression [n], samples [n, 1+K]:
 *   imp [B] = impression[order[b]];   news [B (1+K)] = samples[order[b]][k];
 *   node_ids [B (1+K) N] = news_node_ID[news][t]  (news_node_ID [news_num, N]);   hist [B H] = history[imp][t]  (history
 *   [impressions, H]).
 * All int64.  The step's large rows are then gathered by ONE digat_gather_tables call whose jobs index with these lists.  An
 * index outside its table is clamped into it (no read leaves a table); the caller keeps them inside.  One launch; B == 0
 * returns without one.  DIGAT_ERR_ARG: a null pointer, a negative size, K < 1, an empty table with B > 0; DIGAT_ERR_SHAPE:
 * K > 16, N < 1, H < 1. */
int digat_negative_sample(const int64_t* click, const int64_t* pool_offsets, const int64_t* pool, long n, int K, uint32_t seed,
                          uint32_t epoch, int64_t* samples, void* stream);
int digat_train_batch_ids(const int64_t* order, long B, const int64_t* impression, const int64_t* samples, long n, int K,
                          const int64_t* news_node_ID, long news_num, int N, const int64_t* history, long impressions, int H,
                          int64_t* imp, int64_t* news, int64_t* node_ids, int64_t* hist, void* stream);

/* ---- measurement aid (not on the reference's surface): per-kernel HIP-event timing ---------------
 * Between start and stop every kernel launch of this library is bracketed by two events recorded
 * on the stream it is launched on.  stop() synchronises and returns, per kernel kind, the summed
 * duration [ms], the summed algorithmic work (flops for LINEAR/PROJ, bytes for the others) and the
 * launch count; the three arrays have DIGAT_KERNEL_KINDS entries (any may be NULL). */
enum {
    DIGAT_KERNEL_PROJ = 0,    /* [h|P|Q] = X [W|ffn1|ffn2]^T, the Eq. 8 node projections (MFMA) */
    DIGAT_KERNEL_LINEAR = 1,  /* every other nn.Linear (MFMA)                                    */
    DIGAT_KERNEL_XATTN = 2,   /* fused Eq. 8 score + mask + softmax -> alpha                     */
    DIGAT_KERNEL_POOL = 3,    /* ScaledDotProductAttention pooling                               */
    DIGAT_KERNEL_TOPIC = 4,   /* scatter_softmax + scatter_sum topic pooling                     */
    DIGAT_KERNEL_GLUE = 5,    /* user-node concat                                                */
    DIGAT_KERNEL_AGG = 6,     /* relu(alpha @ h) + X on the matrix cores                         */
    DIGAT_KERNEL_KINDS = 7
};
int digat_profile_start(int max_launches);
/* launches a one-thread kernel (digat_region_marker_kernel) on `stream`: a landmark in a rocprofv3 kernel trace */
int digat_profile_marker(int id, void* stream);
/* bit k set = launches of kind k are recorded (default: all).  Returns the previous mask. */
int digat_profile_set_kinds(unsigned mask);
int digat_profile_pause(int paused);   /* between start and stop: 1 = launches are not recorded, 0 = recorded again (sampling) */
/* after digat_profile_stop: rows processed / rows nominal over the row-list node-projection launches of the profiled
 * region (the encoder leaves the user-graph nodes that cannot reach its outputs out of the projections of
 * layers >= 1), or -1 if there was none */
double digat_profile_live_row_fraction(void);
int digat_profile_stop(double* ms_per_kind, double* work_per_kind, int* launches_per_kind);
/* After digat_profile_stop: the compulsory HBM bytes (operand rows in, result rows out, epilogue row operands; weights not
 * counted) of the recorded launches of the two MFMA kinds, DIGAT_KERNEL_PROJ and DIGAT_KERNEL_LINEAR, whose `work` is flops —
 * for a whole-step roofline (bench.py: roofline_step).  DIGAT_KERNEL_KINDS entries; the byte-priced kinds read 0 here. */
int digat_profile_gemm_bytes(double* bytes_per_kind);
/* After digat_profile_stop: the DIGAT_KERNEL_XATTN launches by kernel, DIGAT_XATTN_PARTS entries each (any may be NULL):
 * [0] user graph, layers >= 1 (row-list launches: xattn_sparse_twin_kernel), [1] user graph, layer 0 of grouped rows
 * (xattn_sparse_l0_kernel), [2] news graphs of <= 16 nodes with the graph in LDS (xattn_small_lds_kernel), [3] every other
 * Eq. 8 launch.  ms = summed launch durations, bytes = algorithmic HBM bytes (SURVEY 8d's bytes_B on the live rows: each
 * distinct row once), launches = count.  Replaces nothing in the reference: measurement only (bench.py roofline_xattn.parts). */
#define DIGAT_XATTN_PARTS 4
int digat_profile_xattn_parts(double* ms, double* bytes, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* DIGAT_HIP_H */
