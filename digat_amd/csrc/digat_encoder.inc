// digat_encoder.inc — the encoder's host side (included by digat_kernels.hip inside its extern "C" block): the workspace layout,
// one call (EncoderCall) with its plan (digat_encoder_plan.h: every decision of the call, made once), the folded pass as named
// stages and a schedule (FoldedPass), the unfolded path, the public entries and the per-news table entries.  No kernels.
static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// The encoder's workspace, carved by encoder_carve alone (the entries carve it, the *_workspace_bytes queries measure it).  The
// grouped and shared entries append their regions after the base layout, so every base region has one offset in all three.
struct FoldCtxWs { float *T, *T2, *glob; };      // the folded path's [B,C1,d] pooled topics + featureAffine, [B,d] news context
struct EncoderWs {
    float *Xu[2], *Xn[2];                   // user nodes [B,U,d] and news nodes [B,N,d], ping-pong
    char* xws; size_t xws_bytes;            // Eq. 8 of either graph: sized for max(N, U), carved by xattn_core at the graph's n
    XattnWs xu;                             // ... carved at n = U: layer 0 of grouped / shared rows (group_projection)
    char* cws; size_t cws_bytes;            // max(news_ctx, user_ctx): the unfolded path's context entries carve it themselves,
    FoldCtxWs fc;                           // ... the folded path lays T, T2, glob inside it
    float *kq_t, *kq_u, *r_user[2], *r_news;  // folded path: topic / user queries from c_n; K3 of the user (ping-pong) and news graphs
    char* xws_news; size_t xws_news_bytes;  // the news graph's own Eq. 8 (side stream)
    XattnWs xn;                             // ... carved at n = N
    // live nodes (cnt, off, idx, flags1) and live buckets (cnt2, off2, idx2, flags2) of the user graphs; adjacency entries per row
    // and the sparse / dense decision (flag); 1 + the last live history slot of every row (hlast)
    int *cnt, *off, *idx, *cnt2, *off2, *idx2, *entries, *flag, *hlast;
    uint8_t *flags1, *flags2;
    int *cnt_n, *off_n, *idx_n; uint8_t* flags_n;      // live nodes of the news graphs (news_live_flags_kernel)
    // layer 0 of grouped rows (xattn_sparse_l0_kernel): group starts, rows led by each row, offsets and list of the live centres
    // of the chunk-leading rows
    int *l0_gs, *l0_off; uint8_t* l0_lead; int* l0_idx;
    // twins (xattn_sparse_twin_kernel): twin words, lead flags, leads per row, offsets, list
    unsigned* tw_word; int* tw_list; uint8_t* tw_flags; int *tw_cnt, *tw_off;
    int *gl_off, *gl_idx;                   // shared runs: offsets and list of the live nodes of the run-leading rows
    int* idx32;                             // the candidate ids as 32-bit indices (layer 0 of larger news graphs from the tables)
    // ENC_GROUPED: the per-group adjacency / category arrays expanded to rows; user_live_flags_kernel's outputs per group (at
    // most B / 4 + 1 groups), expanded to rows by live_expand_kernel
    uint8_t *Au, *cm; int64_t* ci;
    uint8_t *fg, *tfg; unsigned* twg; uint8_t* bfg; int *cg, *eg, *hg, *bcg, *tcg;
    uint8_t *same, *is_leader, *lead; int* leader_of;      // ENC_SHARED: equal users, run leaders, layer-0 chunk sizes, run of every row
};
static bool encoder_carve(Arena& a, int B, int N, int H, int C, int d, int variant, EncoderWs& e) {
    const int U = H + C, C1 = C + 1, nmax = N > U ? N : U;
    const size_t b = (size_t)B, bd = b * d, bu = b * U;
    e = EncoderWs();
    for (float*& x : e.Xu) x = a.take<float>(bu * d);
    for (float*& x : e.Xn) x = a.take<float>(b * N * d);
    Arena xa = a.sub(digat_xattn_workspace_bytes(B, nmax, d));
    e.xws = xa.base; e.xws_bytes = xa.cap;
    e.xu = xattn_carve(xa, B, U, d);
    Arena ca = a.sub(max_sz(digat_news_ctx_workspace_bytes(B, N, d), digat_user_ctx_workspace_bytes(B, U, H, C1, d)));
    e.cws = ca.base; e.cws_bytes = ca.cap;
    e.fc = FoldCtxWs{ca.take<float>(b * C1 * d), ca.take<float>(b * C1 * d), ca.take<float>(bd)};
    e.kq_t = a.take<float>(bd); e.kq_u = a.take<float>(bd);
    e.r_user[0] = a.take<float>(bd); e.r_news = a.take<float>(bd); e.r_user[1] = a.take<float>(bd);
    Arena na = a.sub(digat_xattn_workspace_bytes(B, N, d));
    e.xws_news = na.base; e.xws_news_bytes = na.cap;
    e.xn = xattn_carve(na, B, N, d);
    e.cnt = a.take<int>(b); e.off = a.take<int>(b + 1); e.idx = a.take<int>(bu);
    e.cnt2 = a.take<int>(b); e.off2 = a.take<int>(b + 1); e.idx2 = a.take<int>(b * C1);
    e.entries = a.take<int>(b); e.flag = a.take<int>(64); e.hlast = a.take<int>(b);
    e.flags1 = a.take<uint8_t>(bu); e.flags2 = a.take<uint8_t>(b * C1);
    e.cnt_n = a.take<int>(b); e.off_n = a.take<int>(b + 1); e.idx_n = a.take<int>(b * N); e.flags_n = a.take<uint8_t>(b * N);
    e.l0_gs = a.take<int>(b + 64); e.l0_off = a.take<int>(b + 64); e.l0_lead = a.take<uint8_t>(b); e.l0_idx = a.take<int>(bu);
    e.tw_word = a.take<unsigned>(bu); e.tw_list = a.take<int>(bu); e.tw_flags = a.take<uint8_t>(bu);
    e.tw_cnt = a.take<int>(b + 64); e.tw_off = a.take<int>(b + 64);
    e.gl_off = a.take<int>(b + 64); e.gl_idx = a.take<int>(bu);
    e.idx32 = a.take<int>(b);
    if (variant == ENC_GROUPED) {           // appended: the grouped regions
        const size_t g = b / 4 + 1;
        e.Au = a.take<uint8_t>(bu * U); e.cm = a.take<uint8_t>(b * C1); e.ci = a.take<int64_t>(b * H);
        e.fg = a.take<uint8_t>(g * U); e.tfg = a.take<uint8_t>(g * U); e.twg = a.take<unsigned>(g * U); e.bfg = a.take<uint8_t>(g * C1);
        for (int** x : {&e.cg, &e.eg, &e.hg, &e.bcg, &e.tcg}) *x = a.take<int>(g);
    } else if (variant == ENC_SHARED) {     // appended: the shared regions
        e.same = a.take<uint8_t>(b); e.is_leader = a.take<uint8_t>(b); e.lead = a.take<uint8_t>(b); e.leader_of = a.take<int>(b);
    }
    return a.ok && xa.ok && ca.ok && na.ok;
}
static size_t encoder_ws_bytes(int B, int N, int H, int C, int d, int variant) { Arena a; EncoderWs e; encoder_carve(a, B, N, H, C, d, variant, e); return a.used; }

// One encoder call: what the public entry was given, its plan, and the workspace carved from it (encoder_fwd_impl).  Which path
// the call takes is read from `plan`, never from a pointer being null.
struct EncoderCall {
    const digat_params* p;
    const float* Xn_in; const uint8_t *An, *Mn;
    const float* ue;                        // user embeddings per row (per group: ENC_GROUPED)
    const uint8_t *Au, *cat_mask; const int64_t* cat_idx;       // per row (ENC_GROUPED: the expanded *_g arrays)
    const float* c_n0; float *out_news, *out_user;
    int B, N, H;
    void* workspace; size_t workspace_bytes; hipStream_t st;
    int variant;                            // ENC_PLAIN, ENC_GROUPED, ENC_SHARED
    const int* row_group; int G;            // the group of every row (ENC_SHARED: the row that leads its run)
    const uint8_t *Au_g, *cm_g; const int64_t* ci_g;            // ENC_GROUPED: the user side per group
    // cached per-news / per-topic tables of layer 0 and the queries of c_n0 (digat_encoder_fwd_grouped_cached)
    const float *news_hpq0, *hist_hpq0, *topic_hpq0, *ctxq0; const int64_t* news_index; int64_t news_rows;
    const uint8_t *run_leader, *run_lead;   // plan.shared: rows that lead a run, rows of the layer-0 chunk a row leads
    EncoderPlan plan;
    bool ctx0;                              // encoder_plan_ctx0: the first user context of the folded pass is GEMM + user_ctx0_kernel
    EncoderWs ws;
};
struct SideStream { hipStream_t s; hipEvent_t fork, join, early; int ok; };
// Nothing below is mutable: live-row lists and the side stream are chosen PER CALL through digat_params.flags
// (DIGAT_PARAMS_NO_LIVE_ROWS, DIGAT_PARAMS_SIDE_STREAM_OFF / _ON), so two host threads with different settings cannot flip each
// other's (round 3 had process-wide setters for them).
// Eq. 8 of a batch goes to the sparse kernel when its adjacency holds at most this many entries per node on average
// (sparse_decide_kernel, train_sparse_decide_kernel)
constexpr int SPARSE_PER_NODE = 20;
// One side stream (and its three events) per CALLER stream: consecutive batches issued on alternating caller streams
// (util.batch_streams) then overlap their side work too, and two host threads driving two streams never touch the same
// events.  A caller stream is expected to be driven by one thread at a time (include/digat_hip.h, threading contract); the
// table itself is guarded by a mutex.  Entries live for the life of the process (streams are few and long-lived).
static SideStream* side_stream(hipStream_t caller) {
    struct Entry { int dev; hipStream_t caller; SideStream side; int state; };     // state: 1 = ready, -1 = unavailable
    static Entry tab[64];
    static int used = 0;
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < used; ++i)
        if (tab[i].dev == dev && tab[i].caller == caller) return tab[i].state == 1 ? &tab[i].side : nullptr;
    if (used == 64) return nullptr;            // more caller streams than anyone has: those run single-stream
    Entry& e = tab[used++];
    e.dev = dev; e.caller = caller;
    SideStream& x = e.side;
    const bool ok = hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&x.join, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&x.early, hipEventDisableTiming) == hipSuccess;
    e.state = ok ? 1 : -1;
    return ok ? &x : nullptr;
}

// 256-thread blocks over `total4` float4 pieces, at most `cap` of them (the elementwise kernels stride over the rest)
static int grid_blocks(long total4, int cap) {
    const int blocks = (int)((total4 + 255) / 256);
    return blocks > cap ? cap : blocks;
}

// [kq_topic | kq_user | K3 of the user graph's layer `next_layer`] from a news context, one launch: the user-side queries and,
// while a layer follows, that layer's K3.  The encoder's stage and digat_news_context_queries launch exactly this, so a row of
// the per-news query table has the bits of the in-batch launch (rows are independent of the batch they sit in).
static GemmArgs ctx_queries_args(const digat_params* p, const float* c_n, int M, int next_layer, float* kq_topic, float* kq_user, float* k3) {
    const GemmFormats f = gemm_formats(p);
    const int d = p->d;
    GemmArgs g = gemm_plain(c_n, d, p->user_news_fold_W, p->user_news_fold_b, kq_topic, d, M, d, d, 0);
    g.w[1] = p->userAtt_fold_W; g.bias[1] = p->userAtt_fold_b; g.y[1] = kq_user;
    g.nsegs = 2;
    if (next_layer < p->depth) {
        g.w[2] = p->user[next_layer].F3; g.bias[2] = p->user[next_layer].b3; g.y[2] = k3;
        g.nsegs = 3;
    }
    g.wsplit = (const unsigned short*)p->ctx_wsplit[next_layer]; g.format = f.fmt; g.range_flag = f.range_flag;   // NULL: fp32 MFMA
    g.m_dispatch = bd_dispatch(p->flags);
    return g;
}

// The node projection of a layer as the encoder launches it outside xattn_core (the projections issued early, the group
// projection) and as digat_user_project0 / digat_news_project0 make it per news, once: K3 joins later, in the Eq. 8 kernel.
static GemmArgs layer_proj3_args(const digat_params* p, const digat_layer_params& l, const float* X, int M, float* h, float* P, float* Q) {
    const GemmFormats f = gemm_formats(p);
    return proj3_args(X, M, p->d, l.W, l.bW, l.F1, l.F2, h, P, Q, l.wsplit, (p->flags & DIGAT_PROJ_PQ_X3) ? 1 : 0, f.lfmt, f.range_flag);
}

// The arrays user_live_flags_kernel writes for a set of graphs: live nodes (flags, cnt), twin words and their leads (twin, tflags,
// tcnt), live buckets (bflags, bcnt), adjacency entries, 1 + the last live history slot.
struct LiveArrays { uint8_t *flags, *tflags, *bflags; unsigned* twin; int *cnt, *entries, *hlast, *bcnt, *tcnt; };
// One adjacency pass: the kernel walks `rows` graphs (rowmask: only these) and writes `out`; `expand`: those are groups (or
// run-leading rows), and live_expand_kernel hands every row its group's results.
struct LiveFlagsJob { const uint8_t *Au, *cat_mask; const int64_t* cat_idx; int rows; const uint8_t* rowmask; LiveArrays out; bool expand; };

// What the adjacency pass made for the layers.  The pass fills FoldedPass::pend; publish() copies it to FoldedPass::live once
// the caller's stream is ordered behind the pass: the initial user context, issued on the caller's stream at the same time,
// must not see the lists (only a join orders the caller's stream after the side stream).
struct LiveLists {
    const int *rowidx, *nrows;             // live nodes b*U + i in ascending order, their count (device)
    const int *bucket_idx, *nbuckets;      // live topic buckets
    const int* hist_last;                  // [B]: 1 + the last live history slot of every row
    uint8_t* flags;                        // [B,U]
    TwinLists tw;                          // twins (plan.twins)
};

// Inference fast path with folded attention queries (digat_fold_attention): per layer the [B,d]
// linears shrink from 9 launches to 4 — {topic query, user query, next layer's K3 of the user graph}
// all read the same c_n and go out as ONE three-segment launch.
// Within a layer the news-graph update and the user-graph update read only the PREVIOUS contexts
// (graphEncoders.py:194-195), so the news chain — K3, projection, score, aggregation, context pooling, gate, and
// the queries derived from the new c_n — is independent of the user graph's Eq. 8 until the user context is
// pooled.  The news kernels are small (N = 10 nodes, [B,d] linears: tens of workgroups, latency chains) and run
// on a side stream under the user graph's projection / score / aggregation, which fill the chip; fork and join
// are two events per layer (a pattern hipGraph capture accepts).
//
// One pass: the stages are the member functions, run() is the schedule — which stage goes out on which stream, behind which event.
// SHARED-USER RUNS (plan.shared): the user tensors are given per ROW, as the reference's driver hands them over (util.py:57-67),
// and consecutive rows with identical users were found on the device: row_group[b] = the ROW that leads row b's run,
// run_leader[b] = 1 for those rows, run_lead[b] = rows of the layer-0 chunk row b leads.  Layer 0's group-level data (user
// nodes, [h|P|Q], live flags) then lives in the LEADING ROW's slots of the full-size buffers, every count stays on the device
// (no host read of the number of runs), and the group-indexed kernels work as they are.  G is not used.
struct FoldedPass {
    const EncoderCall& c; const EncoderPlan& pl;
    const float* const Xg0;                // the layer-0 user nodes once per group (NULL: per row in w.Xu[0])
    SideStream* const side;                // NULL: single-stream
    const digat_params* const p; const EncoderWs& w; const hipStream_t st;
    const int B, N, H, G, d, C, L, U, C1;
    const GemmFormats f;
    const int ragged;                      // encoder_ragged (digat_encoder_plan.h): GemmArgs::ragged of the launches that ask
    // c_n_src: where the news context stands BEFORE layer 0 — c_n itself, or (depth >= 1, context given) the caller's c_n0, read
    // in place by the two consumers that precede the first update instead of being copied into c_n first
    float *const c_n, *const c_u; const float* const c_n_src;
    LiveLists pend{}, live{};
    const int* sparse_flag = nullptr;      // the device's sparse / dense decision (sparse_mode AUTO; out of the adjacency pass)
    const int *news_rowidx = nullptr, *news_nrows = nullptr; const uint8_t* news_flags = nullptr;      // live nodes of the news graphs

    FoldedPass(const EncoderCall& call, const float* Xg0_, SideStream* side_)
        : c(call), pl(call.plan), Xg0(Xg0_), side(side_), p(call.p), w(call.ws), st(call.st), B(call.B), N(call.N), H(call.H), G(call.G),
          d(call.p->d), C(call.p->category_num), L(call.p->depth), U(call.H + call.p->category_num), C1(call.p->category_num + 1),
          f(gemm_formats(call.p)), ragged(encoder_ragged(call.p->flags)), c_n(call.out_news), c_u(call.out_user), c_n_src(call.plan.c_n0_in_place ? call.c_n0 : call.out_news) {}

    // the user-side queries + (optionally) the next user-graph K3, all from c_n
    int context_queries(int next_layer, hipStream_t sq) const {
        return launch_gemm(ctx_queries_args(p, next_layer == 0 ? c_n_src : c_n, B, next_layer, w.kq_t, w.kq_u, w.r_user[next_layer & 1]), sq);
    }

    // c_u (+= addend) from the user nodes.  `lists`: the layers' outputs — the rows of dead nodes were never written, the topic
    // pooling takes them as zero.  kq_topic / kq_user: the two queries derived from the news context (the workspace ones, or —
    // initial context — the rows of the per-news table the caller gathered: ctxq0)
    int user_context(const float* Xu_cur, const float* addend, hipStream_t sq, const int* xgroup, bool lists,
                     const float* kq_topic = nullptr, const float* kq_user = nullptr) const {
        if (!kq_topic) { kq_topic = w.kq_t; kq_user = w.kq_u; }
        const uint8_t* flags = lists ? live.flags : nullptr;
        const int* hist_last = flags ? live.hist_last : nullptr;
        // ONE launch (digat_ctxfused.inc) when the weight version carries the fused image and the shape fits; T, T2 stay unused then
        if (pl.user_ctx_fused) {
            const CtxFusedArgs fa{Xu_cur, (long)U * d, xgroup, flags, U, hist_last, kq_topic, kq_user, c.cat_idx, c.cat_mask, addend, c_u,
                                  (const uint4*)p->featureAffine_fsplit, p->featureAffine_b, f.range_flag, B, H, C1, d, sqrtf((float)d)};
            return launch_user_ctx_fused(fa, sq);
        }
        float *T = w.fc.T, *T2 = w.fc.T2;
        int e = launch_topic(Xu_cur, (long)U * d, kq_topic, c.cat_idx, T, B, H, C1, d, sq, xgroup, flags, U, hist_last);
        if (e) return e;
        GemmArgs g = gemm_plain(T, d, p->featureAffine_W, p->featureAffine_b, T2, d, B * C1, d, d, 0);
        g.epi = EPI_RELU_RES; g.e0 = T; g.lde0 = d;
        g.wsplit = (const unsigned short*)p->featureAffine_wsplit;       // non-NULL: split operands on the matrix cores
        g.format = f.fmt; g.range_flag = f.range_flag;
        g.ragged = ragged;        // d = 400: 3 + 2 strips instead of five one-strip tiles that each fetch and split the A tile
        if (live.bucket_idx && gemm_takes_row_list(g)) { g.rowidx = live.bucket_idx; g.nrows_dev = live.nbuckets; }   // unmasked buckets only
        e = launch_gemm(g, sq);
        if (e) return e;
        return launch_pool(T2, (long)C1 * d, kq_user, c.cat_mask, addend, c_u, B, C1, d, sq);
    }

    // The INITIAL c_u straight from the input rows (c.ctx0; digat_ctx0.inc): F x = ue W^T over the graphs ue holds (the groups of
    // ENC_GROUPED, else every row: no list of the run leaders' history rows exists at this point of an ENC_SHARED pass), then one
    // launch per row of the batch.  ue is read in place with stride H d: nothing here waits for build_user_nodes_kernel's output.
    // F x lives in w.Xu[1], which nothing reads or writes before layer 0 of the user graph on the caller's stream — behind this
    // call — with one exception: group_projection builds the groups' nodes at its start (G U d floats, possibly on the side
    // stream, at once) when layer 0's nodes are not kept per group, so ENC_GROUPED puts F x behind them ((U + H) G d <= B U d
    // floats: 4 G <= B).  The side stream's other early work (adjacency pass, news projection) has its own regions.
    int user_context0(const float* kq_topic, const float* kq_user) const {
        if (!kq_topic) { kq_topic = w.kq_t; kq_user = w.kq_u; }
        const bool per_group = c.variant == ENC_GROUPED;
        float* const fx = w.Xu[1] + (per_group ? (size_t)G * U * d : 0);
        return launch_user_ctx0(c.ue, per_group ? G : B, (per_group || pl.shared) ? c.row_group : nullptr, kq_topic, kq_user, c.cat_idx,
                                c.cat_mask, p->featureAffine_W, p->featureAffine_b, p->featureAffine_wsplit, f.fmt, f.range_flag, ragged,
                                nullptr, c_u, fx, B, H, C1, d, st);
    }

    // c_n (+)= gate([local ; global context]) of the news nodes
    int news_context(const float* Xn_cur, hipStream_t sq, bool first) const {
        const long ldx = (long)N * d;
        float *kq = w.kq_t, *glob = w.fc.glob;     // the news context's kq reuses kq_t: the previous user context has consumed it
        GemmArgs gq = gemm_plain(Xn_cur, ldx, p->cand_fold_W, p->cand_fold_b, kq, d, B, d, d, 0);
        gq.wsplit = (const unsigned short*)p->cand_fold_wsplit; gq.format = f.fmt; gq.range_flag = f.range_flag;
        gq.m_dispatch = pl.bd_disp;
        int e = launch_gemm(gq, sq);
        if (e) return e;
        e = launch_pool(Xn_cur, ldx, kq, c.Mn, nullptr, glob, B, N, d, sq);
        if (e) return e;
        GemmArgs g = gemm_plain(Xn_cur, ldx, p->news_graph_W, p->news_graph_b, c_n, d, B, d, 2 * d, 0);
        g.k0 = d; g.a1 = glob; g.lda1 = d;
        g.epi = EPI_GATE; g.e0 = Xn_cur; g.lde0 = ldx; g.e1 = glob; g.lde1 = d; g.e2 = first ? c_n_src : c_n; g.lde2 = d;
        g.wsplit = (const unsigned short*)p->gate_wsplit; g.format = f.fmt; g.range_flag = f.range_flag;
        g.m_dispatch = 1;          // two-operand input: the split-image [B,d] kernel at every row count (the tiled one does not take it)
        return launch_gemm(g, sq);
    }

    // the one launch site of user_live_flags_kernel (and of live_expand_kernel behind it)
    int live_flags(const LiveFlagsJob& j, const LiveArrays& rows, hipStream_t sq) const {
        const bool want_entries = pl.sparse_mode == DIGAT_XATTN_AUTO, twins = pl.twins;
        const LiveArrays& o = j.out;
        hipLaunchKernelGGL(user_live_flags_kernel, dim3((j.rows + 3) / 4), dim3(256), (size_t)4 * ((U * U + 63) & ~63), sq, j.Au, j.cat_mask, j.cat_idx,
                           j.rows, U, H, C1, o.flags, o.cnt, want_entries ? o.entries : (int*)nullptr, o.hlast, o.bflags, o.bcnt,
                           twins ? o.twin : (unsigned*)nullptr, twins ? o.tflags : (uint8_t*)nullptr, twins ? o.tcnt : (int*)nullptr, j.rowmask);
        DIGAT_CHECK_LAUNCH();
        if (!j.expand) return DIGAT_OK;
        LiveExpand le;
        le.flags_g = o.flags; le.twin_g = twins ? o.twin : nullptr; le.tflags_g = o.tflags; le.bflags_g = o.bflags;
        le.cnt_g = o.cnt; le.entries_g = o.entries; le.hlast_g = o.hlast; le.bcnt_g = o.bcnt; le.tcnt_g = o.tcnt;
        le.flags = rows.flags; le.twin = twins ? rows.twin : nullptr; le.tflags = rows.tflags; le.bflags = rows.bflags;
        le.cnt = rows.cnt; le.entries = want_entries ? rows.entries : nullptr; le.hlast = rows.hlast; le.bcnt = rows.bcnt;
        le.tcnt = twins ? rows.tcnt : nullptr;
        hipLaunchKernelGGL(live_expand_kernel, dim3((B + 3) / 4), dim3(256), 0, sq, le, c.row_group, B, U, C1);
        DIGAT_CHECK_LAUNCH();
        return DIGAT_OK;
    }

    // The adjacency pass of the user graphs on `sq`: live nodes and buckets, twins, the sparse / dense decision, and the lists of
    // all of them.  Its results wait in `pend` until publish().
    int adjacency_pass(hipStream_t sq) {
        LiveArrays rows;
        rows.flags = w.flags1; rows.tflags = w.tw_flags; rows.bflags = w.flags2; rows.twin = w.tw_word;
        rows.cnt = w.cnt; rows.entries = w.entries; rows.hlast = w.hlast; rows.bcnt = w.cnt2; rows.tcnt = w.tw_cnt;
        // layer 0 of grouped rows on the chunk kernel (R rows of an impression per wave: xattn_sparse_l0_kernel): its list — the live
        // centres of the rows that lead a chunk — is made with the other two
        const uint8_t* const l0_lead = pl.shared ? c.run_lead : w.l0_lead;         // shared runs: the chunk sizes came with the runs
        ProfScope prof(DIGAT_KERNEL_GLUE, (double)B * ((double)U * U + 2.0 * C1 + H * 8.0) + (double)B * (U + C1) * 6, sq);
        if (pl.l0_chunked && !pl.shared) {
            hipLaunchKernelGGL(sparse_l0_chunks_kernel, dim3(1), dim3(1024), 0, sq, c.row_group, B, G, SPARSE_L0_ROWS, w.l0_gs, w.l0_lead);
            DIGAT_CHECK_LAUNCH();
        }
        LiveFlagsJob j{c.Au, c.cat_mask, c.cat_idx, B, nullptr, rows, false};
        if (pl.shared) {
            // the adjacency pass for the leading rows only; every other row takes its leader's results (in place)
            j.rowmask = c.run_leader; j.expand = true;
        } else if (c.variant == ENC_GROUPED) {
            // the user side is given per group: the adjacency pass once per GROUP, its results handed to the group's rows
            j.Au = c.Au_g; j.cat_mask = c.cm_g; j.cat_idx = c.ci_g; j.rows = G; j.expand = true;
            LiveArrays& o = j.out;
            o.flags = w.fg; o.tflags = w.tfg; o.bflags = w.bfg; o.twin = w.twg;
            o.cnt = w.cg; o.entries = w.eg; o.hlast = w.hg; o.bcnt = w.bcg; o.tcnt = w.tcg;
        }
        const int rc = live_flags(j, rows, sq);
        if (rc) return rc;
        if (pl.sparse_mode == DIGAT_XATTN_AUTO) {
            hipLaunchKernelGGL(sparse_decide_kernel, dim3(1), dim3(1024), 0, sq, (const int*)w.entries, B, U, SPARSE_PER_NODE, w.flag);
            DIGAT_CHECK_LAUNCH();
            sparse_flag = w.flag;
        }
        // up to five lists in two launches (every scan in one, every list in one): live nodes, live buckets, and as wanted the
        // layer-0 chunk leads, the twin leads, the live nodes of the run-leading rows
        ScanPair sp{{w.cnt, w.cnt2}, {w.off, w.off2}, {nullptr, nullptr}};
        ListPair lp{{w.flags1, w.flags2}, {w.off, w.off2}, {U, C1, U, U, U, U}, {w.idx, w.idx2}, {nullptr, nullptr}};
        int jobs = 2;
        if (pl.l0_chunked) {
            sp.cnt[jobs] = w.cnt; sp.off[jobs] = w.l0_off; sp.rowmask[jobs] = l0_lead;
            lp.flags[jobs] = w.flags1; lp.off[jobs] = w.l0_off; lp.out[jobs] = w.l0_idx; lp.rowmask[jobs] = l0_lead;
            ++jobs;
        }
        if (pl.twins) {
            sp.cnt[jobs] = w.tw_cnt; sp.off[jobs] = w.tw_off;
            lp.flags[jobs] = w.tw_flags; lp.off[jobs] = w.tw_off; lp.out[jobs] = w.tw_list;
            lp.width[jobs] = U;
            ++jobs;
        }
        if (pl.shared) {         // the live nodes of the leading rows: what layer 0's group projection makes
            sp.cnt[jobs] = w.cnt; sp.off[jobs] = w.gl_off; sp.rowmask[jobs] = c.run_leader;
            lp.flags[jobs] = w.flags1; lp.off[jobs] = w.gl_off; lp.out[jobs] = w.gl_idx; lp.rowmask[jobs] = c.run_leader;
            lp.width[jobs] = U;
            ++jobs;
        }
        hipLaunchKernelGGL(exclusive_scan2_kernel, dim3(jobs), dim3(1024), 0, sq, sp, B);
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(live_list2_kernel, dim3((B + 3) / 4, jobs), dim3(256), 0, sq, lp, B);
        DIGAT_CHECK_LAUNCH();
        pend = LiveLists{w.idx, w.off + B, w.idx2, w.off2 + B, w.hlast, w.flags1, {nullptr, nullptr, nullptr}};
        if (pl.twins) pend.tw = TwinLists{w.tw_word, w.tw_list, w.tw_off + B};
        return DIGAT_OK;
    }
    // The live lists are in force from layer 0 on: a dead node (a history padding slot, the topic node of an unread category:
    // only its self loop, pooled with weight 0) is never projected, scored or written, in ANY layer.  Its rows of the two
    // node buffers therefore hold whatever the workspace held; the one reader that walks all history rows — the topic
    // pooling — takes them as zero through the flags (a select: no bits of such a row can reach a result;
    // test_uninitialised_workspace_cannot_reach_the_outputs fills the scratch with NaN patterns).
    void publish() { live = pend; }

    int news_projection(int layer, const float* Xn_cur, hipStream_t sq) const {
        GemmArgs gp = layer_proj3_args(p, p->news[layer], Xn_cur, B * N, w.xn.h, w.xn.P, w.xn.Q);
        gp.m_dispatch = 1 << 30;       // always the large-M kernel: a row's bits then do not depend on the batch it sits in
                                       // (digat_news_project0 makes the same launch per news, once)
        if (news_rowidx && gemm_takes_row_list(gp)) { gp.rowidx = news_rowidx; gp.nrows_dev = news_nrows; }      // live nodes only (layers >= 1)
        return launch_gemm(gp, sq, DIGAT_KERNEL_PROJ);
    }

    // layer 0 of grouped rows: every row of a group has the same user nodes, so the G groups are projected once
    // ([G*U] rows instead of [B*U]).  h and Q of a group go straight to the h / Q slots of the Eq. 8 workspace and are
    // read through the group index by the aggregation / score kernels (the 37 rows of an impression share them: they
    // stay in L2); only P' = K3_b + P depends on the row and is expanded later.  Needs nothing but the inputs.
    int group_projection(hipStream_t sq) const {
        const digat_layer_params& lu = p->user[0];
        if (pl.shared) {
            // shared runs: [h|P|Q] of the LEADING rows' live nodes, in place in the full-size planes (the per-row launch of layer 0
            // restricted to the rows whose results anybody reads; K3 joins in the Eq. 8 kernel, as for the groups below)
            GemmArgs gs = layer_proj3_args(p, lu, w.Xu[0], B * U, w.xu.h, w.xu.P, w.xu.Q);
            gs.m_dispatch = B * U;
            if (pl.want_live && gemm_takes_row_list(gs)) { gs.rowidx = w.gl_idx; gs.nrows_dev = w.gl_off + B; }
            return launch_gemm(gs, sq, DIGAT_KERNEL_PROJ);
        }
        const size_t ndg = (size_t)G * U * d;
        float* Xg = pl.xu0_grouped ? const_cast<float*>(Xg0) : w.Xu[1];   // group nodes: built by the caller, or here (Xu[1] is free until layer 0 writes it)
        float* h0 = w.xu.h;
        float* P0 = h0 + ndg;                               // behind the groups' h in the h slot (2 ndg <= nd)
        float* Q0 = w.xu.Q;                                 // the groups' Q at the start of the full-size Q plane
        const int blocks = grid_blocks((long)ndg / 4, 2048);
        if (!pl.xu0_grouped) {
            hipLaunchKernelGGL(build_user_nodes_kernel, dim3(blocks), dim3(256), 0, sq, (const float4*)c.ue,
                               (const float4*)p->topic_node_embedding, (float4*)Xg, (long)G, H, C, d / 4, (const int*)nullptr);
            DIGAT_CHECK_LAUNCH();
        }
        if (pl.group_tables) {
            // [h|P|Q] of a history node depend on that news alone and those of a topic node on nothing: the caller keeps them
            // per news / per topic (digat_user_project0) and hands over the groups' history rows; the projection GEMM of the
            // groups becomes three assemblies [history rows | topic rows] (same kernel, same bits: rows are independent)
            float* dst[3] = {h0, P0, Q0};
            UserNodes3 un3;
            for (int t = 0; t < 3; ++t) {
                un3.hist[t] = (const float4*)(c.hist_hpq0 + (size_t)t * G * H * d);
                un3.topic[t] = (const float4*)(c.topic_hpq0 + (size_t)t * C * d);
                un3.dst[t] = (float4*)dst[t];
            }
            hipLaunchKernelGGL(build_user_nodes3_kernel, dim3(blocks, 3), dim3(256), 0, sq, un3, (long)G, H, C, d / 4);
            DIGAT_CHECK_LAUNCH();
            return DIGAT_OK;
        }
        GemmArgs gg = layer_proj3_args(p, lu, Xg, G * U, h0, P0, Q0);
        gg.m_dispatch = B * U;                              // the kernel the per-row path would pick: same bits
        return launch_gemm(gg, sq, DIGAT_KERNEL_PROJ);
    }

    // Layer 0 of the user graph through the group index (grouped rows, shared runs), on the caller's stream: the group projection
    // unless it went out early, then the sparse arm, the dense arm, or both with the device choosing.
    int user_layer0_grouped(const float* r_user, bool projected) const {
        const digat_layer_params& lu = p->user[0];
        const size_t ndg = pl.shared ? (size_t)B * U * d : (size_t)G * U * d;      // shared runs: full-size planes, a group's rows sit in its leading row's slots
        float* h0 = w.xu.h;
        float* P0 = h0 + ndg;                           // group_projection's layout
        float* Q0 = w.xu.Q;
        int rc = projected ? DIGAT_OK : group_projection(st);
        if (rc) return rc;
        if (pl.l0_sparse) {
            // P' = K1 (the groups' P0) + K3 (this layer's r_user) is formed inside the kernel: nothing is expanded
            // live centres only (the list of the adjacency pass), P / Q / h / X read through the group index
            const bool l0_live = pl.want_live && live.flags;
            SparseArgs sg = sparse_args(P0, Q0, h0, pl.xu0_grouped ? Xg0 : w.Xu[0], lu.a, c.Au, w.Xu[1], B, U, d / 4);
            sg.radd = r_user; sg.group = c.row_group; sg.G = G;
            sg.xgroup = (pl.xu0_grouped || pl.xu0_shared) ? 1 : 0;
            if (l0_live) { sg.live = live.flags; sg.rowidx = live.rowidx; sg.nrows_dev = live.nrows; }
            if (pl.sparse_mode == DIGAT_XATTN_AUTO) sg.run_if = sparse_flag;
            if (!l0_live && pl.xu0_grouped && pl.want_live) sg.fill_flags = (const uint8_t*)pend.flags;
            sg.fill_out = w.Xu[0];
            // R rows of an impression per wave: every neighbour row fetched serves R rows (xattn_sparse_l0_kernel; same bits)
            const Eq8L0Route l0 = (pl.l0_chunked && l0_live) ? eq8_l0_route(sparse_in(sg), pl.shared ? (B + SPARSE_L0_ROWS - 1) / SPARSE_L0_ROWS : G)
                                                             : Eq8L0Route();
            if (l0.eligible) rc = launch_sparse_l0(sg, l0.launch, pl.shared ? c.run_lead : w.l0_lead, w.l0_idx, w.l0_off + B, st);
            else rc = launch_sparse(sg, st);
        }
        if (rc || !pl.l0_dense) return rc;
        const int* skip_if = pl.l0_sparse ? sparse_flag : nullptr;      // both arms: the device's decision picks one
        const size_t nd = (size_t)B * U * d;
        float* P = w.xu.P;
        {
            ProfScope prof(DIGAT_KERNEL_GLUE, skip_if ? 0.0 : (double)nd * 4, st);
            hipLaunchKernelGGL(expand_proj_kernel, dim3(grid_blocks((long)nd / 4, 4096)), dim3(256), 0, st, (const float4*)P0, (const float4*)r_user,
                               c.row_group, (float4*)P, (long)B, U, d / 4, skip_if);
            DIGAT_CHECK_LAUNCH();
        }
        PairOpts po;
        po.group = c.row_group; po.skip_if = skip_if;
        return launch_xattn_pairwise(P, Q0, h0, w.Xu[0], lu.a, c.Au, w.Xu[1], w.xu.alpha, B, U, d, st, po);
    }

    // A per-row layer of the user graph: every layer projects, scores and writes the live nodes only (layer 0 too: see publish)
    int user_layer(int i, const float* r_user, const float* Xu_in, float* Xu_out) const {
        const digat_layer_params& lu = p->user[i];
        XattnOpts o;
        o.wsplit = lu.wsplit; o.rowidx = live.rowidx; o.nrows_dev = live.nrows; o.live = live.flags;
        o.sparse_mode = pl.sparse_mode; o.sparse_flag = sparse_flag; o.pq_x3 = pl.pq_x3; o.pq_mode = i > 0 ? pl.pq_mode : 0;
        // after the last layer only the history rows are read (the user context's topic pooling, :124):
        // the topic nodes' own Eq. 8 is not computed there (wave-per-centre sparse kernel)
        o.centre_limit = (i > 0 && i == L - 1 && pl.sparse_mode == DIGAT_XATTN_SPARSE) ? H : 0;
        o.gemm_format = f.lfmt; o.range_flag = f.range_flag;
        o.tw = (i > 0 && live.tw.word) ? &live.tw : nullptr;
        return xattn_core(Xu_in, c.Au, r_user, lu.W, lu.bW, lu.F1, lu.F2, lu.a, Xu_out, nullptr, B, U, d, w.xws, w.xws_bytes, st, o);
    }

    // K3 of the news graph, from the previous user context
    int news_k3(int i, hipStream_t sn) const {
        const digat_layer_params& ln = p->news[i];
        GemmArgs g3 = gemm_plain(c_u, d, ln.F3, ln.b3, w.r_news, d, B, d, d, 0);
        g3.wsplit = (const unsigned short*)ln.f3_wsplit; g3.format = f.fmt; g3.range_flag = f.range_flag;
        g3.m_dispatch = pl.bd_disp;
        return launch_gemm(g3, sn);
    }

    // the live nodes of the news graphs, once per pass (the graphs do not change with the layers)
    int news_live_lists(hipStream_t sn) {
        ProfScope prof(DIGAT_KERNEL_GLUE, (double)B * ((double)N * N + 6.0 * N), sn);
        hipLaunchKernelGGL(news_live_flags_kernel, dim3((B + 3) / 4), dim3(256), (size_t)4 * ((N * N + 15) & ~15), sn, c.An, c.Mn, B, N, w.flags_n, w.cnt_n);
        DIGAT_CHECK_LAUNCH();
        ScanPair sp{{w.cnt_n}, {w.off_n}, {nullptr}};
        ListPair lp{{w.flags_n}, {w.off_n}, {N, N, N, N, N, N}, {w.idx_n}, {nullptr}};
        hipLaunchKernelGGL(exclusive_scan2_kernel, dim3(1), dim3(1024), 0, sn, sp, B);
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(live_list2_kernel, dim3((B + 3) / 4, 1), dim3(256), 0, sn, lp, B);
        DIGAT_CHECK_LAUNCH();
        news_rowidx = w.idx_n; news_nrows = w.off_n + B; news_flags = w.flags_n;
        return DIGAT_OK;
    }

    // Eq. 8 of the news graph, layer i: Xn_in -> Xn_out
    int news_layer(int i, const float* Xn_in, float* Xn_out, hipStream_t sn) const {
        const digat_layer_params& ln = p->news[i];
        const bool cached = i == 0 && pl.news_cached0, indexed = i == 0 && pl.news_indexed0;
        const size_t plane = indexed ? (size_t)c.news_rows * N * d : (size_t)B * N * d;
        if (pl.news_early) {     // small graphs, projections already done (news_projection): K3 joins in the score kernel
            // layer 0 with news_index: h | P | Q and the nodes themselves are the per-news TABLES, read in place through the index
            const float* hn = cached ? c.news_hpq0 : w.xn.h;
            PairOpts po;
            po.radd = w.r_news; po.alpha_wanted = false;
            if (indexed) po.bindex = c.news_index;
            return launch_xattn_pairwise(hn + plane, hn + 2 * plane, hn, Xn_in, ln.a, c.An, Xn_out, w.xn.alpha, B, N, d, sn, po);
        }
        if (indexed) {
            // Larger news graphs, layer 0 from the per-news TABLES: [h | P | Q] of a news graph depend on the news alone, so
            // the projection GEMM of layer 0 (B N rows: at N = 26 the largest launch of a MIND-large step) is replaced by reading the
            // candidates' rows of the table IN PLACE — the sparse kernel's group indirection with the candidate id as the "group" —
            // and adding K3 in the kernel, in the GEMM epilogue's order (K3 + K1): the bits of the in-batch launch.
            hipLaunchKernelGGL(index_to_i32_kernel, dim3((B + 255) / 256), dim3(256), 0, sn, c.news_index, w.idx32, B);
            DIGAT_CHECK_LAUNCH();
            SparseArgs sgn = sparse_args(c.news_hpq0 + plane, c.news_hpq0 + 2 * plane, c.news_hpq0, Xn_in, ln.a, c.An, Xn_out, B, N, d / 4);
            sgn.radd = w.r_news; sgn.group = w.idx32; sgn.xgroup = 1;
            sgn.G = B;                      // profiling, the distinct rows behind the index: at most B candidates
            sgn.live = news_flags; sgn.rowidx = news_rowidx; sgn.nrows_dev = news_nrows;
            if (news_rowidx) sgn.prof_part = XPART_NEWS + 1;
            return launch_sparse(sgn, sn);
        }
        // larger news graphs (N = 26 / 65: the breadth-first SAG, a few entries per node) take the sparse kernel when the
        // caller says so (DIGAT_NEWS_XATTN_SPARSE); there is no device-side decision for this graph
        XattnOpts o;
        o.wsplit = ln.wsplit; o.rowidx = news_rowidx; o.nrows_dev = news_nrows; o.live = news_flags;
        o.sparse_mode = pl.news_sparse_mode;
        o.pq_x3 = pl.pq_x3;
        o.pq_mode = pl.pq_mode;       // the news graph's P' always carries K3 from the GEMM epilogue: bf16 storage applies at every layer
        o.gemm_format = f.lfmt; o.range_flag = f.range_flag;
        o.prof_part = news_rowidx ? XPART_NEWS + 1 : 0;
        return xattn_core(Xn_in, c.An, w.r_news, ln.W, ln.bW, ln.F1, ln.F2, ln.a, Xn_out, nullptr, B, N, d, w.xws_news, w.xws_news_bytes, sn, o);
    }

    static bool record(hipEvent_t e, hipStream_t s) { return hipEventRecord(e, s) == hipSuccess; }
    static bool wait(hipStream_t s, hipEvent_t e) { return hipStreamWaitEvent(s, e, 0) == hipSuccess; }

    // The schedule: which stage goes out on which stream, behind which event.
    int run() {
        int rc;
        // Work that depends on the inputs alone goes out on the side stream at once, under the initial user context: the adjacency
        // pass, the group projection of layer 0 and (small news graphs) the news projections of layer 0.
        const bool group_early = side && L > 0 && pl.by_group;
        const bool live_early = side && pl.want_scan;
        if (side && (pl.news_early || group_early || live_early)) {
            if (!record(side->fork, st) || !wait(side->s, side->fork)) return DIGAT_ERR_LAUNCH;
        }
        if (live_early) {                  // first: layer 0 may need the sparse / dense decision
            rc = adjacency_pass(side->s);
            if (rc) return rc;
        }
        if (group_early) {
            rc = group_projection(side->s);
            if (rc) return rc;
        }
        if (group_early || live_early) {
            if (!record(side->early, side->s)) return DIGAT_ERR_LAUNCH;
        }
        if (pl.news_early && !pl.news_cached0) {      // cached: the caller kept layer 0's news projections per news (digat_news_project0)
            rc = news_projection(0, c.Xn_in, side ? side->s : st);
            if (rc) return rc;
        }
        // [kq_topic | kq_user | K3 of the user graph's layer 0] are functions of the candidate's cached c_n0: a caller that keeps them
        // per news (digat_news_context_queries, next to c_n0 itself) hands over the batch's rows and the first link of the chain goes
        const size_t bd = (size_t)B * d;
        const float* const ctxq0 = pl.ctxq0 ? c.ctxq0 : nullptr;
        if (!ctxq0) {
            rc = context_queries(0, st);
            if (rc) return rc;
        }
        rc = c.ctx0 ? user_context0(ctxq0, ctxq0 ? ctxq0 + bd : nullptr)
                    : user_context(pl.xu0_grouped ? Xg0 : w.Xu[0], nullptr, st, (pl.xu0_grouped || pl.xu0_shared) ? c.row_group : nullptr, false,
                                   ctxq0, ctxq0 ? ctxq0 + bd : nullptr);        // c_u (:192)
        if (rc) return rc;
        const float* xn_cur = c.Xn_in;
        int un = 0, nn = 0;
        for (int i = 0; i < L; ++i) {
            const float* r_user = (i == 0 && ctxq0) ? ctxq0 + 2 * bd : w.r_user[i & 1];     // K3 of the user graph, from the previous c_n
            hipStream_t sn = side ? side->s : st;
            if (side && i == 0) {                      // the news chain starts from the initial c_u (caller's stream)
                if (!record(side->fork, st) || !wait(sn, side->fork)) return DIGAT_ERR_LAUNCH;
            }
            if (side && i > 0) {                       // K3 of this layer's user graph + the live lists come from the side stream
                if (!wait(st, side->join)) return DIGAT_ERR_LAUNCH;
            }
            // ---- user graph, Eq. 8 (caller's stream)
            if (i == 0 && pl.want_scan && !live_early) {           // no side stream: the lists and the sparse / dense decision first
                rc = adjacency_pass(st);
                if (rc) return rc;
            }
            if (i == 0 && side && (group_early || live_early)) {
                if (!wait(st, side->early)) return DIGAT_ERR_LAUNCH;
            }
            if (i == 0 && pl.want_live) publish();
            rc = (i == 0 && pl.by_group) ? user_layer0_grouped(r_user, group_early) : user_layer(i, r_user, w.Xu[un], w.Xu[un ^ 1]);
            if (rc) return rc;
            if (side && !record(side->fork, st)) return DIGAT_ERR_LAUNCH;      // this layer's user nodes are written
            // ---- news graph, Eq. 8 + context + the queries that follow from the new c_n (side stream)
            rc = news_k3(i, sn);
            if (rc) return rc;
            if (i == 0 && pl.news_lists) {
                rc = news_live_lists(sn);
                if (rc) return rc;
            }
            rc = news_layer(i, xn_cur, w.Xn[nn], sn);
            if (rc) return rc;
            xn_cur = w.Xn[nn]; nn ^= 1; un ^= 1;
            rc = news_context(xn_cur, sn, i == 0);     // c_n += ... (:196)
            if (rc) return rc;
            rc = context_queries(i + 1, sn);           // queries (+ next K3, into the other r_user buffer) from the UPDATED c_n
            if (rc) return rc;
            if (side && !record(side->join, sn)) return DIGAT_ERR_LAUNCH;      // the next user-graph update may start
            if (pl.news_early && i + 1 < L) {          // the next layer's news projections need only Xn
                rc = news_projection(i + 1, xn_cur, sn);
                if (rc) return rc;
            }
            // The user context of this layer feeds the next NEWS update and the result, not the next user-graph update: it runs
            // on the side stream once the caller's stream has written the user nodes, under the next layer's projection GEMM.
            if (side && !wait(sn, side->fork)) return DIGAT_ERR_LAUNCH;
            rc = user_context(w.Xu[un], c_u, sn, nullptr, true);       // c_u += ... (:197)
            if (rc) return rc;
        }
        if (side && L > 0) {
            if (!record(side->join, side->s) || !wait(st, side->join)) return DIGAT_ERR_LAUNCH;
        }
        return DIGAT_OK;
    }
};

size_t digat_encoder_workspace_bytes(int B, int N, int H, int C, int d, int depth) { (void)depth; return encoder_ws_bytes(B, N, H, C, d, ENC_PLAIN); }

// The per-row user arrays of the variant.  ENC_GROUPED: the user tensors are per group (G of them) and row_group[b] names the
// group of row b; the small per-row byte / index arrays are expanded here, so Au / cat_mask / cat_idx are per row in every
// variant and only ue [G,H,d] stays per group.  ENC_SHARED: the runs of equal users are found (and honoured if plan.shared).
static int encoder_user_rows(EncoderCall& c) {
    const digat_params* p = c.p;
    const EncoderWs& w = c.ws;
    const int B = c.B, H = c.H, d = p->d, C = p->category_num, U = H + C;
    hipStream_t st = c.st;
    if (c.variant == ENC_GROUPED) {
        // expand the small per-user byte / index arrays to rows (4.6 MB for 1024 rows of 67x67 adjacency)
        const GatherJobs jobs{{c.Au_g, c.cm_g, (const uint8_t*)c.ci_g}, {w.Au, w.cm, (uint8_t*)w.ci}, {(long)U * U, (long)(C + 1), (long)H * 8}};
        hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, st, jobs, c.row_group, (long)B);
        DIGAT_CHECK_LAUNCH();
        c.Au = w.Au; c.cat_mask = w.cm; c.cat_idx = w.ci;
    } else if (c.variant == ENC_SHARED) {
        // consecutive rows with identical users: runs found on the device (user_rows_same_kernel, shared_runs_kernel)
        ProfScope prof(DIGAT_KERNEL_GLUE, (double)B * ((double)H * d * 4 + (double)U * U + (C + 1) + 8.0 * H), st);
        hipLaunchKernelGGL(user_rows_same_kernel, dim3(B), dim3(256), 0, st, (const uint4*)c.ue, c.Au, c.cat_mask, c.cat_idx, B, (long)H * d / 4, U * U,
                           C + 1, H, w.same);
        DIGAT_CHECK_LAUNCH();
        hipLaunchKernelGGL(shared_runs_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t*)w.same, B, SPARSE_L0_ROWS, w.leader_of, w.is_leader, w.lead);
        DIGAT_CHECK_LAUNCH();
        // ue is per ROW, row_group[b] = the row that leads row b's run; runs the plan does not honour are ignored: the plain per-row path
        if (c.plan.shared) { c.row_group = w.leader_of; c.run_leader = w.is_leader; c.run_lead = w.lead; }
    }
    return DIGAT_OK;
}

// The path without folded attention queries (training-shaped weights): every context through its own entry, one stream.
static int encoder_fwd_unfolded(const EncoderCall& c) {
    const digat_params* p = c.p;
    const EncoderWs& w = c.ws;
    const int B = c.B, N = c.N, H = c.H, d = p->d, C = p->category_num, L = p->depth, U = H + C;
    hipStream_t st = c.st;
    // c_u (:192)
    int rc = digat_user_ctx_fwd(w.Xu[0], c.cat_mask, c.cat_idx, c.out_news, p->user_news_K, p->user_news_Q, p->user_news_bQ,
                                p->featureAffine_W, p->featureAffine_b, p->userAtt_K, p->userAtt_Q, p->userAtt_bQ,
                                nullptr, c.out_user, B, U, H, C + 1, d, w.cws, w.cws_bytes, st);
    if (rc) return rc;
    const float* xn_cur = c.Xn_in;
    int un = 0, nn = 0;
    const GemmFormats f = gemm_formats(p);
    XattnOpts o;
    o.gemm_format = f.lfmt; o.range_flag = f.range_flag;      // the layers' images (the only ones this loop reads)
    for (int i = 0; i < L; ++i) {
        const digat_layer_params& ln = p->news[i];
        const digat_layer_params& lu = p->user[i];
        // both graph updates read the PREVIOUS contexts (:194-195)
        rc = launch_gemm(gemm_plain(c.out_user, d, ln.F3, ln.b3, w.r_news, d, B, d, d, 0), st);
        if (rc) return rc;
        o.wsplit = ln.wsplit;
        rc = xattn_core(xn_cur, c.An, w.r_news, ln.W, ln.bW, ln.F1, ln.F2, ln.a, w.Xn[nn], nullptr, B, N, d, w.xws, w.xws_bytes, st, o);
        if (rc) return rc;
        rc = launch_gemm(gemm_plain(c.out_news, d, lu.F3, lu.b3, w.r_user[0], d, B, d, d, 0), st);
        if (rc) return rc;
        o.wsplit = lu.wsplit;
        rc = xattn_core(w.Xu[un], c.Au, w.r_user[0], lu.W, lu.bW, lu.F1, lu.F2, lu.a, w.Xu[un ^ 1], nullptr, B, U, d, w.xws, w.xws_bytes, st, o);
        if (rc) return rc;
        xn_cur = w.Xn[nn]; nn ^= 1; un ^= 1;
        // c_n += news context (:196); c_u += user context with the UPDATED c_n (:197)
        rc = digat_news_ctx_fwd(xn_cur, c.Mn, p->cand_K, p->cand_Q, p->cand_bQ, p->news_graph_W, p->news_graph_b,
                                c.out_news, c.out_news, B, N, d, w.cws, w.cws_bytes, st);
        if (rc) return rc;
        rc = digat_user_ctx_fwd(w.Xu[un], c.cat_mask, c.cat_idx, c.out_news, p->user_news_K, p->user_news_Q, p->user_news_bQ,
                                p->featureAffine_W, p->featureAffine_b, p->userAtt_K, p->userAtt_Q, p->userAtt_bQ,
                                c.out_user, c.out_user, B, U, H, C + 1, d, w.cws, w.cws_bytes, st);
        if (rc) return rc;
    }
    return DIGAT_OK;
}

// Every entry: the checks and the plan, the carve, the per-row user arrays of the variant, the user nodes and the initial news
// context, then the unfolded path or the folded pass.
static int encoder_fwd_impl(EncoderCall& c) {
    const digat_params* p = c.p;
    const bool grouped = c.variant == ENC_GROUPED;
    if (!p || !c.Xn_in || !c.An || !c.Mn || !c.ue || !c.out_news || !c.out_user || !c.workspace) return DIGAT_ERR_ARG;
    if (grouped ? (!c.Au_g || !c.cm_g || !c.ci_g || !c.row_group) : (!c.Au || !c.cat_mask || !c.cat_idx)) return DIGAT_ERR_ARG;
    const int B = c.B, N = c.N, H = c.H, G = c.G, d = p->d, C = p->category_num, U = H + C;
    EncoderPlanIn in = {};
    in.flags = p->flags; in.B = B; in.N = N; in.H = H; in.C = C; in.d = d; in.L = p->depth; in.G = G; in.variant = c.variant;
    in.folded = p->cand_fold_W && p->user_news_fold_W && p->userAtt_fold_W;
    in.c_n0 = c.c_n0; in.news_hpq0 = c.news_hpq0; in.hist_hpq0 = c.hist_hpq0; in.topic_hpq0 = c.topic_hpq0; in.ctxq0 = c.ctxq0;
    in.news_index = c.news_index; in.news_rows = c.news_rows;
    in.fsplit = p->featureAffine_fsplit; in.ctx_fused_fits = ctxfused_ok(H, C + 1, d);
    const EncoderPlan& pl = c.plan = encoder_plan(in);
    c.ctx0 = encoder_plan_ctx0(in);
    if (pl.status) return pl.status;
    Arena ar(c.workspace, c.workspace_bytes);
    if (!encoder_carve(ar, B, N, H, C, d, c.variant, c.ws)) return DIGAT_ERR_WORKSPACE;
    if (B == 0) return DIGAT_OK;
    if (pl.status_after_carve) return pl.status_after_carve;
    hipStream_t st = c.st;
    const EncoderWs& w = c.ws;
    int rc = encoder_user_rows(c);
    if (rc) return rc;
    // user graph nodes = [history | topic nodes]  (:191): once per group (3 MB instead of a 110 MB expansion that the first two
    // kernels would read back) when every reader of the layer-0 nodes can go through the group index
    float* const Xg0 = pl.xu0_grouped ? w.xu.h + 2 * (size_t)G * U * d : nullptr;      // behind the groups' h and P in the h slot (3 G <= B)
    {
        const long nrows = pl.xu0_grouped ? G : B;
        ProfScope prof(DIGAT_KERNEL_GLUE, (double)nrows * ((double)H * d * 8 + (double)C * d * 4), st);
        // shared runs: ue is per row already, and only the run-leading rows are ever read (through row_group)
        hipLaunchKernelGGL(build_user_nodes_kernel, dim3(grid_blocks(nrows * U * (d / 4), 2048)), dim3(256), 0, st, (const float4*)c.ue,
                           (const float4*)p->topic_node_embedding, (float4*)(pl.xu0_grouped ? Xg0 : w.Xu[0]), nrows, H, C, d / 4,
                           (pl.xu0_grouped || pl.shared) ? (const int*)nullptr : c.row_group, pl.shared ? c.run_leader : (const uint8_t*)nullptr);
        DIGAT_CHECK_LAUNCH();
    }
    // c_n: given (inference, :189) or computed (forward, :180); it lives in out_news from here on
    if (pl.c_n0_in_place) {                  // layer 0's news context update writes out_news from c_n0 directly
    } else if (c.c_n0) {
        if (hipMemcpyAsync(c.out_news, c.c_n0, (size_t)B * d * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return DIGAT_ERR_LAUNCH;
    } else {
        rc = digat_news_ctx_fwd(c.Xn_in, c.Mn, p->cand_K, p->cand_Q, p->cand_bQ, p->news_graph_W, p->news_graph_b,
                                nullptr, c.out_news, B, N, d, w.cws, w.cws_bytes, st);
        if (rc) return rc;
    }
    if (!pl.folded) return encoder_fwd_unfolded(c);
    return FoldedPass(c, Xg0, pl.side_wanted ? side_stream(st) : nullptr).run();
}

int digat_encoder_fwd(const digat_params* p, const float* Xn_in, const uint8_t* An, const uint8_t* Mn,
                      const float* ue, const uint8_t* Au, const uint8_t* cat_mask, const int64_t* cat_idx,
                      const float* c_n0, float* out_news, float* out_user, int B, int N, int H,
                      void* workspace, size_t workspace_bytes, void* stream) {
    EncoderCall c{};
    c.variant = ENC_PLAIN; c.p = p; c.Xn_in = Xn_in; c.An = An; c.Mn = Mn; c.ue = ue; c.Au = Au; c.cat_mask = cat_mask; c.cat_idx = cat_idx;
    c.c_n0 = c_n0; c.out_news = out_news; c.out_user = out_user; c.B = B; c.N = N; c.H = H;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.st = (hipStream_t)stream;
    return encoder_fwd_impl(c);
}

size_t digat_encoder_grouped_workspace_bytes(int B, int N, int H, int C, int d, int depth) { (void)depth; return encoder_ws_bytes(B, N, H, C, d, ENC_GROUPED); }

int digat_encoder_fwd_grouped(const digat_params* p, const float* Xn_in, const uint8_t* An, const uint8_t* Mn,
                              const float* ue_g, const uint8_t* Au_g, const uint8_t* cat_mask_g, const int64_t* cat_idx_g,
                              const int32_t* row_group, const float* c_n0, float* out_news, float* out_user,
                              int B, int G, int N, int H, void* workspace, size_t workspace_bytes, void* stream) {
    return digat_encoder_fwd_grouped_cached(p, Xn_in, An, Mn, ue_g, Au_g, cat_mask_g, cat_idx_g, row_group, c_n0, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, 0, out_news, out_user, B, G, N, H, workspace, workspace_bytes, stream);
}

int digat_encoder_fwd_grouped_cached(const digat_params* p, const float* Xn_in, const uint8_t* An, const uint8_t* Mn,
                                     const float* ue_g, const uint8_t* Au_g, const uint8_t* cat_mask_g, const int64_t* cat_idx_g,
                                     const int32_t* row_group, const float* c_n0, const float* news_hpq0,
                                     const float* hist_hpq0, const float* topic_hpq0, const float* ctxq0,
                                     const int64_t* news_index, int64_t news_rows, float* out_news,
                                     float* out_user, int B, int G, int N, int H, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    EncoderCall c{};
    c.variant = ENC_GROUPED; c.p = p; c.Xn_in = Xn_in; c.An = An; c.Mn = Mn; c.ue = ue_g; c.Au_g = Au_g; c.cm_g = cat_mask_g; c.ci_g = cat_idx_g;
    c.row_group = row_group; c.G = G; c.c_n0 = c_n0; c.out_news = out_news; c.out_user = out_user; c.B = B; c.N = N; c.H = H;
    c.news_hpq0 = news_hpq0; c.hist_hpq0 = hist_hpq0; c.topic_hpq0 = topic_hpq0; c.ctxq0 = ctxq0; c.news_index = news_index; c.news_rows = news_rows;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.st = (hipStream_t)stream;
    return encoder_fwd_impl(c);
}

// ---- shared-user runs: the per-row signature of digat_encoder_fwd, the grouped arithmetic of layer 0 --------------------------
size_t digat_encoder_shared_workspace_bytes(int B, int N, int H, int C, int d, int depth) { (void)depth; return encoder_ws_bytes(B, N, H, C, d, ENC_SHARED); }

int digat_encoder_fwd_shared(const digat_params* p, const float* Xn_in, const uint8_t* An, const uint8_t* Mn, const float* ue,
                             const uint8_t* Au, const uint8_t* cat_mask, const int64_t* cat_idx, const float* c_n0, float* out_news,
                             float* out_user, int B, int N, int H, void* workspace, size_t workspace_bytes, void* stream) {
    EncoderCall c{};
    c.variant = ENC_SHARED; c.p = p; c.Xn_in = Xn_in; c.An = An; c.Mn = Mn; c.ue = ue; c.Au = Au; c.cat_mask = cat_mask; c.cat_idx = cat_idx;
    c.c_n0 = c_n0; c.out_news = out_news; c.out_user = out_user; c.B = B; c.N = N; c.H = H;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.st = (hipStream_t)stream;
    return encoder_fwd_impl(c);
}

// ---- the per-news tables: each row is the launch the encoder makes inside a batch (ctx_queries_args, layer_proj3_args) -------
int digat_news_context_queries(const digat_params* p, const float* c_n, float* out, int M, void* stream) {
    if (!p || !c_n || !out || M < 0) return DIGAT_ERR_ARG;
    if (!p->user_news_fold_W || !p->userAtt_fold_W) return DIGAT_ERR_ARG;          // folded inference path only
    const int d = p->d;
    if (d <= 0 || d % 4) return DIGAT_ERR_SHAPE;
    if (M == 0) return DIGAT_OK;
    const size_t md = (size_t)M * d;
    return launch_gemm(ctx_queries_args(p, c_n, M, 0, out, out + md, out + 2 * md), (hipStream_t)stream);
}

int digat_user_project0(const digat_params* p, const float* X, float* hpq, int M, void* stream) {
    if (!p || !X || !hpq || M < 0 || p->depth <= 0) return DIGAT_ERR_ARG;
    const int d = p->d;
    if (d <= 0 || d % 4) return DIGAT_ERR_SHAPE;
    if (M == 0) return DIGAT_OK;
    const size_t nd = (size_t)M * d;
    GemmArgs gg = layer_proj3_args(p, p->user[0], X, M, hpq, hpq + nd, hpq + 2 * nd);      // the groups' projection launch of layer 0, row by row
    gg.m_dispatch = 1 << 30;                                               // the large-M kernel whatever M is (C topic rows)
    return launch_gemm(gg, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}

int digat_news_project0(const digat_params* p, const float* Xn, float* hpq, int M, int N, void* stream) {
    if (!p || !Xn || !hpq || M < 0 || N <= 0 || p->depth <= 0) return DIGAT_ERR_ARG;
    const int d = p->d;
    if (d <= 0 || d % 4 || (long)M * N > 0x7fffffffL / 4) return DIGAT_ERR_SHAPE;
    if (M == 0) return DIGAT_OK;
    const size_t ndn = (size_t)M * N * d;
    GemmArgs gp = layer_proj3_args(p, p->news[0], Xn, M * N, hpq, hpq + ndn, hpq + 2 * ndn);      // FoldedPass::news_projection, layer 0
    gp.m_dispatch = 1 << 30;
    return launch_gemm(gp, (hipStream_t)stream, DIGAT_KERNEL_PROJ);
}
