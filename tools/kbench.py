#!/usr/bin/env python3
"""Kernel micro-benchmarks on the GPU box (development aid, not part of the product or the tests).

  python tools/kbench.py xattn  [B n d]      Eq. 8 pairwise kernel alone (digat_xattn_pairwise_fwd)
  python tools/kbench.py linear [M N K]      fp32 MFMA linear (digat_linear_f32)
  python tools/kbench.py encoder             whole DIGAT.inference, per-kernel-kind breakdown
  python tools/kbench.py gemm [M N K]        Eq. 8 projection GEMM in fp16x3 and fp16-fp8c (137 k x 1 200 x 400: the bench's
                                             live rows), alternated; then 4 096-row scoring passes (inference_grouped) in each mode
  python tools/kbench.py cnn [T Lw V dm Kc att window]        CNN news encoder, inference: HIP vs forward_stock on the same device,
                                             alternated, the spread of the rounds' medians reported (default T = 8 192 and 65 238)
  python tools/kbench.py cnn-train [T ...]   one CNN training step (forward + backward, dropout 0.2), the same way (T = 6 400)
  python tools/kbench.py user-graph [G H C I]   a batch's user graphs: gathered from the [I,U,U] table (digat_gather_tables) vs built
                                             from category indices (digat_user_graph_build), and one build over all I impressions
  python tools/kbench.py train-input [n_behaviours]   the training input, host path vs device path (train_input.py), alternated,
                                             median [min, max] of five rounds: one epoch's negative sampling, the enqueue of 200
                                             steps' inputs, and 60 training steps (B = 64, K = 4; table and derived user graphs)
  python tools/kbench.py ablation-score [passes news_num]   the five ablation encoders over a MIND-small-shaped dev corpus
                                             (65 238 news, N = 10, H = 50, C = 17, d = 400, depth 3; 50 passes of 4 096 rows): the
                                             per-row path (util.gather_batch + graph_encoder.inference) against
                                             util.score_rows(grouped=True), alternated, median [min, max] of five rounds
  python tools/kbench.py topk                segmented top-k (digat_topk_segments) against torch.topk — (a) one segment of 65 238,
                                             k = 10; (b) 256 segments of 65 238, k = 10 and 100 — and against digat_rank_metrics —
                                             (c) 73 152 segments of the dev length distribution, k = 10; alternated in one process,
                                             median [min, max] of five rounds, bytes/s against the one-pass floor rows x 4 B
  python tools/kbench.py recommend [users news_num]   util.recommend: 64 users against the pool of all news at MIND-small shapes
                                             (65 238 news, N = 10, H = 50, C = 17, d = 400, depth 3), users per second;
                                             then util.recommend_report for four diversities beside four recommend(diversity=) calls
  python tools/kbench.py dot-topk [news_num d]   NRMS retrieval: evaluate.dot_topk (fused inner product + top-k, no score matrix)
                                             against torch.matmul + evaluate.topk_segments and torch.matmul + torch.topk, G = 64 and
                                             4 096 users x 65 237 news, d = 400, k = 10 and 100, the three legs in turn, median
                                             [min, max] of five rounds; then nrms.recommend for 4 096 users end to end
  python tools/kbench.py shortlist           long segmented selection (digat_shortlist_segments): 256 segments of 65 238 scores at
                                             m = 128, 256 and 1 024 against torch.topk and, at 128, against digat_topk_segments; the
                                             legs in turn in one process, median [min, max] of five rounds
  python tools/kbench.py dot-shortlist [news_num d]   NRMS retrieval of long lists: evaluate.dot_shortlist (scores a slab of 256 users
                                             at a time, then the selection) against torch.matmul per 1 024 users + torch.topk, G = 64
                                             and 4 096 users x 65 237 news, d = 400, m = 256 and 1 024, 50-entry skip rows, the legs in
                                             turn, median [min, max] of five rounds, time and peak device bytes
  python tools/kbench.py qdot [news_num d]   the quantised first stage: user quantisation + evaluate.qdot_topk / qdot_shortlist at
                                             M = 128, 256 and 1 024 + evaluate.refine_lists to k = 10 and 100, against
                                             evaluate.dot_topk and against torch.matmul per 1 024 users + evaluate.topk_segments, G = 64
                                             and 4 096 users x 65 237 news, d = 400, 50-entry skip rows, the legs in turn, median
                                             [min, max] of five rounds, the parts alone, peak device bytes, the index build; then
                                             nrms.index_report on the planted-signal corpus with fit_retriever's retriever
  python tools/kbench.py dot-rank [news_num d]   retrieval evaluation: evaluate.dot_rank (fused inner product + rank of given targets,
                                             no score matrix) against the same ranks from evaluate.dot_scores or torch.matmul over
                                             chunks of 1 024 users + torch compares and sums with the skip mask, G = 64 and 4 096
                                             users x 65 237 news, d = 400, one and five targets per user, the legs in turn, median
                                             [min, max] of five rounds, time and peak device bytes; then nrms.retrieval_metrics for
                                             4 096 users end to end
  python tools/kbench.py pool-softmax [news_num d]   retrieval training: evaluate.pool_softmax (fused full-pool softmax loss, no score
                                             matrix) against the stock composition — torch.matmul per 1 024 users, masked logsumexp,
                                             gather, autograd backward —, G = 64 and 4 096 users x 65 237 news, d = 400, 50-entry skip
                                             rows, one and five targets per user, forward and forward + backward, the legs in turn,
                                             median [min, max] of five rounds, time and peak device bytes; then nrms.fit_retriever on
                                             the planted-signal corpus: nrms.retrieval_metrics before and after
  python tools/kbench.py list-softmax [d]    listwise distillation: evaluate.list_softmax (fused per-user list softmax, no [G, M, d] gather)
  python tools/kbench.py list-pairwise [d]   pairwise nDCG loss: evaluate.list_pairwise (fused LambdaRank over per-user lists, no [G, M, M] tensor)
                                             against the stock composition — index_select, torch.bmm, log_softmax, KL, autograd —,
                                             G = 64 and 4 096 lists of M = 128 and 1 024 over a compact pool, d = 400, forward and
                                             forward + backward, the legs in turn, median [min, max] of five rounds, time and peak
                                             device bytes; then nrms.distil_retriever on the planted-signal corpus with the trained
                                             DIGAT as the teacher: teacher_agreement@10 and recall@k of the held-out clicks before
                                             and after, with intervals
  python tools/kbench.py diversify [news_num d]   diversified top-k: evaluate.mmr_select (one launch, the Gram in LDS) against gather +
                                             torch.bmm + k rounds of torch element-wise ops and arg-max, G = 64 and 4 096 lists of
                                             M = 128, d = 400, k = 10 and 100, with and without a cap of 2 per category, the legs in
                                             turn, median [min, max] of five rounds; then util.recommend for 64 users at k = 10 with
                                             and without diversity=0.3
  python tools/kbench.py calibrate [rounds demo]   calibrated top-k: evaluate.calibrated_select (one launch, a list in registers) against a
                                             gather of the categories + k rounds of torch element-wise ops with torch.log in float64 and
                                             arg-max, G = 64 and 4 096 lists of M = 128 and 1 024, k = 10 and 100, C = 17, the legs in
                                             turn, median [min, max] of five rounds, time and peak device bytes; then recommend(calibration=)
                                             in {0, 0.3, 0.5, 0.8} on 512 held-out impressions of the planted-signal corpus: kl,
                                             category_max_share, recall@10 and MRR with intervals, paired against calibration 0
  python tools/kbench.py rerank [rounds demo d]    joint re-rank: evaluate.rerank_select (one launch, no Gram: one row of it per step) against
                                             (a) gather + torch.bmm Gram + k rounds of torch ops with float64 logs and (b) rows gathered once + a
                                             batched matrix-vector product per step, both chunked to 1 GiB; G = 64 and 4 096 lists of M = 128
                                             and 1 024, k = 10 and 100, d = 400, C = 17, weights (0.5, 0.3, 0.2) and (0.7, 0.3, 0) (long MMR;
                                             at M = 128 mmr_select too), the legs in turn, median [min, max] of five rounds, time and peak
                                             device bytes; then plain, diversity=0.3, calibration=0.5 and rerank=(0.2, 0.4) on 512 held-out
                                             impressions of the planted-signal corpus: ild, kl, recall@10 and MRR with intervals, paired
                                             against plain
  python tools/kbench.py exposure-cap [rounds demo]   exposure-capped top-k: evaluate.capped_select (prepare, one sort, blocks of rounds, emit)
                                             against the same rounds in stock torch (argsort, sort, cumsum, gather, scatter), G = 64 and
                                             4 096 lists of M = 128 and 1 024 of 65 237 news with a popularity head, k = 10 and 100, caps of
                                             1.2 x and 2 x the mean exposure, the legs in turn, median [min, max] of five rounds, rounds and
                                             peak device bytes; then plain and exposure_cap in {16, 4, 2} on 512 held-out impressions of the
                                             planted-signal corpus: coverage, gini, largest exposure, short lists, recall@10 and MRR with
                                             intervals, paired against plain
  python tools/kbench.py list-pl [d rounds demo]   policy gradient: evaluate.list_pl (fused Plackett-Luce slate likelihood over per-user lists and
                                             its closed-form gradient) against index_select + bmm + gather + logsumexp + flipped logcumsumexp
                                             under autograd, chunked to 1 GiB, (G, M, k, S) in {64, 4 096} x {128, 1 024} x {10, 100} x {1, 8},
                                             forward and forward + backward, time and peak device bytes
  python tools/kbench.py policy [train_users steps k samples log_users replicates logs]   nrms.fit_policy (REINFORCE) beside fit_ranker, the
                                             click softmax and fit_policy(estimator="plrank") on the planted-signal corpus — step times,
                                             the nDCG@k of the steps' own slates, held-out metrics with paired intervals, and the variance
                                             of d_users under both estimators — and (logs = 1) nrms.fit_from_logs on a log the trained
                                             DIGAT makes, with intervals
  python tools/kbench.py plrank [d rounds]   PL-Rank policy gradient: evaluate.list_plrank (score, draw and value in one kernel, the PL-Rank-2
                                             coefficient behind it) against list_softmax forward + pl_sample + list_pl with leave-one-out
                                             weights (what a step was made of) and against the stock torch composition, list-pl's sixteen
                                             shapes, forward and forward + backward, the legs in turn, median [min, max] of five rounds
  python tools/kbench.py pl-sample [rounds demo]   stochastic lists: evaluate.pl_sample (one workgroup per slate: hash, two float64 logs, a
                                             1024-record sort, the probability as a suffix sum) against rand + double log + topk + gather
                                             + flipped logcumsumexp in stock PyTorch, chunked to 1 GiB, (G, M, k, S) in {64, 4 096} x
                                             {128, 1 024} x {10, 100} x {1, 8}, the legs in turn, median [min, max] of five rounds, time
                                             and peak device bytes
  python tools/kbench.py off-policy [users k samples truth_samples replicates]   off-policy evaluation on the planted-signal corpus: the
                                             trained DIGAT logs slates with propensities (util.recommend_slates), colder and hotter
                                             target policies are valued on the log (score_lists, slate_log_prob, off_policy_value: IPS
                                             and SNIPS with intervals, ess / n) beside their true on-policy value
  python tools/kbench.py pl-expect [rounds]  doubly robust control variate: evaluate.pl_expect (pl_log_prob's workgroup with one more suffix
                                             sum beside Z_t) against gathers + the tail's logsumexp + a flipped logcumsumexp and the same
                                             for the weighted sums in stock PyTorch, chunked to 1 GiB, pl-sample's shapes, the legs in turn,
                                             median [min, max] of five rounds, time and peak device bytes
  python tools/kbench.py off-policy-steps [users k shortlist samples truth_samples replicates]   the off-policy demonstration at k = 10 from a
                                             shortlist of 80 with a reward per position: IPS, SNIPS, PDIS and DR (value model: the category
                                             half of the planted match) with intervals (util.off_policy_report) beside the on-policy truth
  python tools/kbench.py list-quality [news_num d]   list quality: evaluate.list_quality (one launch, the Gram in LDS) against the same
                                             figures from gather + torch.bmm, the upper triangle's sum and max, a sort for the
                                             categories, a broadcast compare for the overlap and torch.bincount for the exposure,
                                             G = 64 and 4 096 lists of k = 10 and 100, d = 400, with and without category and base
                                             list, the legs in turn, median [min, max] of five rounds
  python tools/kbench.py bootstrap [units columns replicates]   metric intervals: evaluate.bootstrap_sums (one kernel: hash a draw,
                                             gather the row, add in registers) against torch.randint + gather + sum with the
                                             replicates chunked to about 1 GiB of intermediates, and against the numpy twin at 20
                                             replicates (as measured, not extrapolated); 73 152 units x 4 and 8 columns x 1 000 and
                                             10 000 replicates, and 4 096 units x 8 columns; the legs in turn, median [min, max] of
                                             five rounds, time and peak device bytes
  python tools/kbench.py sag-lists [news categories dim top_M]  the SAG's similar-news lists of a MIND-small-shaped corpus
                                             (65 238 news over 17 categories of skewed sizes, the largest ~30 %, dim 768, top_M 5):
                                             construct_SAG.similar_news_lists_device per category against cos_topk_device + all five
                                             kinds copied to the host + similar_news_lists_host, alternated, median [min, max] of five
                                             rounds (wall clock around a device synchronise); then the walk, and build_similarity
                                             with the embeddings read from .npy files
Timing with torch events on the current stream, median of --iters launches.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from digat_amd import _lib  # noqa: E402


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def bench_xattn(B=1024, n=67, d=400, density=None):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    P, Q, h, X = (torch.randn(B, n, d, device=dev, generator=g) for _ in range(4))
    r = torch.randn(B, d, device=dev, generator=g)
    a = torch.randn(d, device=dev, generator=g) * 0.1
    if density == "mind":
        from digat_amd import synthetic
        batch = synthetic.make_encoder_batch(B, 10, 50, n - 50, d, seed=0)
        A = torch.from_numpy(batch["user_graph"]).to(dev).view(torch.uint8)
        print(f"   MIND-like user graphs: element density {float(batch['user_graph'].mean()):.3f}")
    elif density is None:
        A = torch.ones(B, n, n, dtype=torch.uint8, device=dev)
    else:
        A = (torch.rand(B, n, n, device=dev, generator=g) < density).to(torch.uint8)
        A |= torch.eye(n, dtype=torch.uint8, device=dev)[None]
    out = torch.empty_like(X)
    alpha = torch.empty(B, n, n, device=dev)
    L = _lib.lib()

    def run():
        _lib.check(L.digat_xattn_pairwise_fwd(P.data_ptr(), Q.data_ptr(), h.data_ptr(), X.data_ptr(),
                                              a.data_ptr(), A.data_ptr(), out.data_ptr(), alpha.data_ptr(), B, n, d,
                                              _lib.stream_ptr()), "xattn")
    med, best = timeit(run)
    bytes_b = B * (5.0 * n * d * 4 + d * 4 + n * n) + 4 * d
    lane_ops = 3.0 * B * n * n * d + 2.0 * B * n * n * d / 2
    print(f"xattn B={B} n={n} d={d}: median {med*1e3:.1f} us  best {best*1e3:.1f} us  "
          f"{bytes_b/med/1e6:.0f} GB/s algorithmic  ({bytes_b/1e6:.0f} MB)")


def bench_xattn_entry(B=1024, n=67, d=400, per_node=0):
    """digat_xattn_fwd_mode (K3 + projections + Eq. 8) on MIND-shaped user graphs: the dense pair against the sparse kernel."""
    from digat_amd import synthetic
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    batch = synthetic.make_encoder_batch(B, 10, 50, n - 50, d, seed=0)
    if per_node > 0:       # random graphs with about per_node entries per node (self loops included) instead of MIND-shaped ones
        rnd = torch.rand(B, n, n, generator=torch.Generator().manual_seed(1)) < (per_node - 1) / (n - 1)
        batch["user_graph"] = (rnd | torch.eye(n, dtype=torch.bool)[None]).numpy()
    A = torch.from_numpy(batch["user_graph"]).to(dev).view(torch.uint8)
    X = torch.randn(B, n, d, device=dev, generator=g)
    ctx = torch.randn(B, d, device=dev, generator=g)
    W, F1, F2, F3 = (torch.randn(d, d, device=dev, generator=g) / d ** 0.5 for _ in range(4))
    bW, b3 = torch.randn(d, device=dev, generator=g) * 0.1, torch.randn(d, device=dev, generator=g) * 0.1
    a = torch.randn(d, device=dev, generator=g) * 0.1
    L = _lib.lib()
    nbytes = L.digat_xattn_workspace_bytes(B, n, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outs = {}
    for name, mode in (("dense", 1), ("sparse", 2)):
        out = torch.empty_like(X)

        def run():
            _lib.check(L.digat_xattn_fwd_mode(X.data_ptr(), A.data_ptr(), ctx.data_ptr(), W.data_ptr(), bW.data_ptr(), F1.data_ptr(),
                                              F2.data_ptr(), F3.data_ptr(), b3.data_ptr(), a.data_ptr(), out.data_ptr(), B, n, d, mode,
                                              ws.data_ptr(), nbytes, _lib.stream_ptr()), "xattn_fwd_mode")
        med, best = timeit(run)
        outs[name] = out
        print(f"digat_xattn_fwd_mode {name:6s} B={B} n={n} d={d} (fp32 MFMA projections of all rows included): median {med*1e3:.1f} us  best {best*1e3:.1f} us")
    print(f"   max |dense - sparse| = {float((outs['dense'] - outs['sparse']).abs().max()):.2e}"
          f"   adjacency entries per node {float(batch['user_graph'].sum() / (B * n)):.2f}")


def bench_linear(M=68608, N=400, K=400):
    dev = torch.device("cuda:0")
    x = torch.randn(M, K, device=dev)
    w = torch.randn(N, K, device=dev) / K ** 0.5
    b = torch.randn(N, device=dev)
    y = torch.empty(M, N, device=dev)
    L = _lib.lib()

    def run():
        _lib.check(L.digat_linear_f32(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, M, N, K,
                                      _lib.stream_ptr()), "linear")
    med, best = timeit(run)
    fl = 2.0 * M * N * K
    print(f"linear M={M} N={N} K={K}: median {med*1e3:.1f} us best {best*1e3:.1f} us  {fl/med/1e9:.1f} TFLOP/s")
    if M >= 2048 and N % 80 == 0 and K % 8 == 0:
        y6 = torch.empty(M, N, device=dev)
        ws = torch.empty(L.digat_split_weights_bytes(N, K), dtype=torch.uint8, device=dev)

        def run6():
            _lib.check(L.digat_linear_f32x3(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y6.data_ptr(), N, M, N, K,
                                            ws.data_ptr(), int(os.environ.get("KBENCH_GEMM_FORMAT", "0")), _lib.stream_ptr()), "linear x3")
        m6, b6 = timeit(run6)
        print(f"   bf16x6 (incl. weight split): median {m6*1e3:.1f} us best {b6*1e3:.1f} us  {fl/m6/1e9:.1f} fp32-equivalent TFLOP/s"
              f"  max|diff vs fp32 kernel| {float((y6 - y).abs().max()):.2e}")
    ref = torch.addmm(b, x, w.t())
    t_ref, _ = timeit(lambda: torch.addmm(b, x, w.t()))
    print(f"   (rocBLAS addmm for scale: {t_ref*1e3:.1f} us, max|diff| {float((ref - y).abs().max()):.2e})")


def bench_gemm(M=137216, N=1200, K=400, rounds=3):
    """fp16x3 against fp16-fp8c (DIGAT_GEMM_F16F8C) on the same data, alternated `rounds` times: the projection GEMM alone (split
    images made once, outside the timing), then whole 4 096-row passes of util.score_rows (inference_grouped) on a MIND-small-shaped
    synthetic corpus.  Executed TF/s counts the issued MFMA work (fp16x3: three f16 products over K padded to 32; fp16-fp8c: the
    f16 product over the k-steps below K plus two e4m3 products over K padded to 128) against the fp32-equivalent 2 M N K."""
    import time
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    b = torch.randn(N, device=dev, generator=g)
    L = _lib.lib()
    fmts = {"fp16x3": _lib.GEMM_F16X3, "fp16-fp8c": _lib.GEMM_F16F8C}
    ys, imgs = {}, {}
    for name, f in fmts.items():
        imgs[name] = torch.empty(L.digat_split_weights_bytes_format(N, K, f), dtype=torch.uint8, device=dev)
        _lib.check(L.digat_split_weights(w.data_ptr(), N, K, imgs[name].data_ptr(), f, _lib.stream_ptr()), "split")
        ys[name] = torch.empty(M, N, device=dev)
    # the GEMM alone: digat_linear_f32x3 re-splits per call, so time the split by itself and subtract it
    times = {n: [] for n in fmts}
    for _ in range(rounds):
        for name, f in fmts.items():
            def run():
                _lib.check(L.digat_linear_f32x3(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), ys[name].data_ptr(), N, M, N, K,
                                                imgs[name].data_ptr(), f, _lib.stream_ptr()), "linear")
            def split():
                _lib.check(L.digat_split_weights(w.data_ptr(), N, K, imgs[name].data_ptr(), f, _lib.stream_ptr()), "split")
            t, _ = timeit(run)
            ts, _ = timeit(split)
            times[name].append((t - ts) * 1e3)
    ref = x.double() @ w.double().t() + b.double()
    kp32, kp128 = -(-K // 32) * 32, -(-K // 128) * 128
    ks_f16 = sum(min(4, -(-(K - kt * 128) // 8)) for kt in range(kp128 // 128)) * 32
    issued = {"fp16x3": 3 * 2.0 * M * N * kp32, "fp16-fp8c": 2.0 * M * N * (ks_f16 + 2 * kp128)}
    for name in fmts:
        us = float(np.median(times[name]))
        err = float((ys[name].double() - ref).abs().max() / ref.abs().max())
        print(f"gemm {name:9s} M={M} N={N} K={K}: {us:.1f} us (median of {rounds} alternations: "
              f"{', '.join(f'{t:.1f}' for t in times[name])})  {2.0 * M * N * K / us / 1e6:.1f} fp32-equivalent TF/s  "
              f"{issued[name] / us / 1e6:.1f} executed TF/s  max err / max|y| {err:.2e}")
    # whole scoring passes
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    import types
    spec = synthetic.SynthSpec(news_num=8192, impressions=1200, seed=3)
    corpus = synthetic.make_corpus(spec)
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, 3, seed=4, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=3, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    rows = dc.rows
    npass = rows / 4096.0
    imps = int(spec.impressions)
    enc = model.graph_encoder
    pass_ms = {n: [] for n in fmts}
    for _ in range(rounds):
        for name in fmts:
            enc.projection_mode = name
            util.prepare_news_side(enc, dc, 1024)
            util.score_rows(model, dc, 0, rows, 1024, launch_rows=4096)          # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                util.score_rows(model, dc, 0, rows, 1024, launch_rows=4096)
            torch.cuda.synchronize()
            pass_ms[name].append((time.perf_counter() - t0) * 1e3 / npass)
    for name in fmts:
        ms = float(np.median(pass_ms[name]))
        print(f"pass {name:9s} 4 096-row passes ({npass:.1f} per run, {rows} rows, {imps} impressions): {ms:.3f} ms per pass "
              f"({', '.join(f'{t:.3f}' for t in pass_ms[name])}), {imps / (ms * npass / 1e3):.0f} impressions/s")


def bench_topic(B=1024, H=50, C=17, d=400):
    dev = torch.device("cuda:0")
    U = H + C
    Xu = torch.randn(B, U, d, device=dev)
    kq = torch.randn(B, d, device=dev)
    idx = torch.randint(0, C + 1, (B, H), device=dev, dtype=torch.int64)
    out = torch.empty(B, C + 1, d, device=dev)
    L = _lib.lib()

    def run():
        _lib.check(L.digat_topic_pool_fwd(Xu.data_ptr(), kq.data_ptr(), idx.data_ptr(), out.data_ptr(), B, U, H, C + 1, d,
                                          _lib.stream_ptr()), "topic")
    med, best = timeit(run)
    by = B * (H * d * 4 + d * 4 + H * 8 + (C + 1) * d * 4)
    print(f"topic B={B} H={H} C1={C+1} d={d}: median {med*1e3:.1f} us best {best*1e3:.1f} us "
          f"{by/med/1e6:.0f} GB/s algorithmic ({by/1e6:.0f} MB)")


def bench_msa(T=8192, Lw=32, V=30000, dm=300, h=16, dk=25, att=256):
    import types
    from digat_amd import newsEncoders, synthetic
    dev = torch.device("cuda:0")
    state = synthetic.make_msa_state(V, dm, h, dk, att, seed=1)
    text, mask = synthetic.make_titles(T, Lw, V, seed=2)
    cfg = types.SimpleNamespace(vocabulary_size=V, word_embedding_dim=dm, max_title_length=Lw, dropout_rate=0.2,
                                MSA_head_num=h, MSA_head_dim=dk, attention_dim=att)
    enc = newsEncoders.MSA(cfg)
    enc.load_state_dict({k_: torch.from_numpy(v) for k_, v in state.items()})
    enc = enc.to(dev).eval()
    tt, tm = torch.from_numpy(text).to(dev), torch.from_numpy(mask).to(dev)

    def hip():
        with torch.no_grad():
            return enc(tt, tm)

    def stock():
        with torch.no_grad():
            return enc.forward_stock(tt.unsqueeze(0), tm.unsqueeze(0))
    a = hip()
    b = stock().detach()[0]
    m1, _ = timeit(hip, iters=10)
    m2, _ = timeit(stock, iters=10)
    flops = T * Lw * (2.0 * dm * 3 * h * dk + 2.0 * h * dk * att) + T * h * 4.0 * Lw * Lw * dk
    print(f"MSA news encoder T={T} titles x {Lw} tokens: HIP {m1:.2f} ms ({T/m1/1e3:.2f} M titles/s, {flops/m1/1e9:.1f} TFLOP/s fp32-eq)"
          f"   stock torch {m2:.2f} ms   max|diff| {float((a - b).abs().max()):.2e}")


def bench_msa_train(T=6400, Lw=32, V=30000, dm=300, h=16, dk=25, att=256):
    """One training step of the MSA news encoder (forward + backward, dropout 0.2): digat_msa_fwd_train / digat_msa_bwd /
    digat_embedding_bwd against the stock PyTorch modules.  T = 6400 titles is the reference's step (64 impressions x
    (5 candidates x 10 SAG nodes + 50 history items))."""
    import types
    from digat_amd import newsEncoders, synthetic
    dev = torch.device("cuda:0")
    state = synthetic.make_msa_state(V, dm, h, dk, att, seed=1)
    text, mask = synthetic.make_titles(T, Lw, V, seed=2)
    cfg = types.SimpleNamespace(vocabulary_size=V, word_embedding_dim=dm, max_title_length=Lw, dropout_rate=0.2,
                                MSA_head_num=h, MSA_head_dim=dk, attention_dim=att)
    enc = newsEncoders.MSA(cfg)
    enc.load_state_dict({k_: torch.from_numpy(v) for k_, v in state.items()})
    enc = enc.to(dev).train()
    tt, tm = torch.from_numpy(text).to(dev).unsqueeze(0), torch.from_numpy(mask).to(dev).unsqueeze(0)
    R = torch.randn(1, T, h * dk, device=dev)

    def step(fn):
        def run():
            enc.zero_grad(set_to_none=True)
            (fn(tt, tm) * R).sum().backward()
        return run
    m1, _ = timeit(step(enc), iters=10)
    m2, _ = timeit(step(enc.forward_stock), iters=10)
    M = T * Lw
    flops = 3 * (M * (2.0 * dm * 3 * h * dk + 2.0 * h * dk * att)) + T * h * Lw * Lw * dk * 2.0 * 7
    print(f"MSA training step T={T} titles x {Lw} tokens: HIP {m1:.2f} ms ({flops/m1/1e9:.1f} TFLOP/s fp32-eq)   stock torch {m2:.2f} ms")
    from digat_amd import _lib
    _lib.lib().digat_profile_start(4096)
    step(enc)()
    torch.cuda.synchronize()
    import ctypes as C
    ms = (C.c_double * 7)(); wk = (C.c_double * 7)(); cn = (C.c_int * 7)()
    _lib.lib().digat_profile_stop(ms, wk, cn)
    print("   library kernel ms by kind (proj, linear, xattn, pool, topic, glue, agg):", [round(v, 3) for v in ms], list(cn))


def alternate(fa, fb, rounds=5, iters=5):
    """Medians of ``rounds`` timing rounds of fa and fb, taken in turn (ABAB...): ((median, min, max) of fa's rounds, the same of fb's)."""
    ma, mb = [], []
    for _ in range(rounds):
        ma.append(timeit(fa, iters=iters, warm=1)[0])
        mb.append(timeit(fb, iters=iters, warm=1)[0])
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    return stat(ma), stat(mb)


def _cnn_encoder(T, Lw, V, dm, Kc, att, window):
    import types
    from digat_amd import newsEncoders, synthetic
    dev = torch.device("cuda:0")
    state = synthetic.make_cnn_state(V, dm, Kc, att, "naive", window, seed=1)
    text, mask = synthetic.make_titles(T, Lw, V, seed=2)
    cfg = types.SimpleNamespace(vocabulary_size=V, word_embedding_dim=dm, max_title_length=Lw, dropout_rate=0.2, cnn_method="naive",
                                cnn_kernel_num=Kc, cnn_window_size=window, attention_dim=att)
    enc = newsEncoders.CNN(cfg)
    enc.load_state_dict({k_: torch.from_numpy(v) for k_, v in state.items()})
    return enc.to(dev), torch.from_numpy(text).to(dev).unsqueeze(0), torch.from_numpy(mask).to(dev).unsqueeze(0)


def bench_cnn(T=0, Lw=32, V=30000, dm=300, Kc=400, att=256, window=3):
    """CNN news encoder, inference (digat_cnn_fwd) against forward_stock on the same device in the same process.  T = 65 238 is
    MIND-small's news count (the news-representation cache of a dev run), V x dm = 36 MB: the table sits in the Infinity Cache."""
    for T_ in ([T] if T else [8192, 65238]):
        enc, tt, tm = _cnn_encoder(T_, Lw, V, dm, Kc, att, window)
        enc.eval()

        def hip():
            with torch.no_grad():
                return enc(tt, tm)

        def stock():
            with torch.no_grad():
                return enc.forward_stock(tt, tm)
        diff = float((hip() - stock()).abs().max())
        (m1, lo1, hi1), (m2, lo2, hi2) = alternate(hip, stock)
        flops = 2.0 * T_ * Lw * (window * dm * Kc + Kc * att)
        print(f"CNN news encoder T={T_} titles x {Lw} tokens, window {window}: HIP {m1:.2f} ms [{lo1:.2f}, {hi1:.2f}] ({T_/m1/1e3:.2f} M titles/s, "
              f"{flops/m1/1e9:.1f} TFLOP/s fp32-eq)   stock torch {m2:.2f} ms [{lo2:.2f}, {hi2:.2f}]   max|diff| {diff:.2e}")
        del enc, tt, tm
        torch.cuda.empty_cache()


def bench_cnn_train(T=6400, Lw=32, V=30000, dm=300, Kc=400, att=256, window=3):
    """One training step of the CNN news encoder (forward + backward, both dropouts at 0.2): digat_cnn_fwd_train / digat_cnn_bwd /
    digat_embedding_bwd against the stock PyTorch modules, alternated.  T = 6 400 titles is the reference's step."""
    enc, tt, tm = _cnn_encoder(T, Lw, V, dm, Kc, att, window)
    enc.train()
    R = torch.randn(1, T, Kc, device=tt.device)

    def step(fn):
        def run():
            enc.zero_grad(set_to_none=True)
            (fn(tt, tm) * R).sum().backward()
        return run
    (m1, lo1, hi1), (m2, lo2, hi2) = alternate(step(enc), step(enc.forward_stock))
    flops = 3 * 2.0 * T * Lw * (window * dm * Kc + Kc * att)
    print(f"CNN training step T={T} titles x {Lw} tokens, window {window}: HIP {m1:.2f} ms [{lo1:.2f}, {hi1:.2f}] ({flops/m1/1e9:.1f} TFLOP/s fp32-eq)"
          f"   stock torch {m2:.2f} ms [{lo2:.2f}, {hi2:.2f}]")


def _nrms_model(model, V=30000, dm=300, h=20, dk=20, att=200, Lw=32, H=50, A=10, dropout=0.2):
    from digat_amd import nrms, synthetic
    cfg = nrms.make_config(model=model, vocabulary_size=V, word_embedding_dim=dm, head_num=h, head_dim=dk, attention_dim=att,
                           max_title_length=Lw, max_history_num=H, augmented_news_num=A, dropout_rate=dropout)
    m = nrms.Model(cfg)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in synthetic.make_nrms_state(V, dm, h, dk, att, sa=(model == "NRMS-SA"), seed=1).items()})
    return m.to(torch.device("cuda:0"))


def bench_nrms_news(T=65238, Lw=32, V=30000):
    """NRMS news encoder, inference (digat_mhsa_fwd: key-masked attention) against forward_stock, alternated in one process.
    T = 65 238 is MIND-small's news count: the plain news cache of a dev run."""
    from digat_amd import synthetic
    m = _nrms_model("NRMS", V=V, Lw=Lw).eval()
    enc = m.news_encoder
    text, mask = synthetic.make_titles(T, Lw, V, seed=2)
    tt, tm = torch.from_numpy(text).cuda().unsqueeze(0), torch.from_numpy(mask).cuda().unsqueeze(0)

    def hip():
        with torch.no_grad():
            return enc(tt, tm)

    def stock():
        with torch.no_grad():
            return enc.forward_stock(tt, tm)
    diff = float((hip() - stock()).abs().max())
    (m1, lo1, hi1), (m2, lo2, hi2) = alternate(hip, stock)
    print(f"NRMS news encoder T={T} titles x {Lw} tokens: HIP {m1:.2f} ms [{lo1:.2f}, {hi1:.2f}] ({T/m1/1e3:.2f} M titles/s)"
          f"   stock torch {m2:.2f} ms [{lo2:.2f}, {hi2:.2f}]   max|diff| {diff:.2e}")


def bench_nrms_user(B=4096, H=50, N=65238):
    """NRMS user encoder, inference: B users x H history items looked up in the cached news representations by id (digat_mhsa_fwd with
    the cache as its table) against index_select + encode_stock, alternated."""
    m = _nrms_model("NRMS", H=H).eval()
    ue = m.user_encoder
    g = torch.Generator().manual_seed(3)
    cache = torch.randn(N, m.news_embedding_dim, generator=g).cuda()
    ids = torch.randint(0, N, (B, H), generator=g).cuda()
    length = torch.randint(0, H + 1, (B, 1), generator=g)
    mask = (torch.arange(H)[None, :] < length).cuda()

    def hip():
        with torch.no_grad():
            return ue.encode_cached(cache, ids, mask)

    def stock():
        with torch.no_grad():
            return ue.encode_stock(cache.index_select(0, ids.flatten()).view(B, H, -1), mask)
    diff = float((hip() - stock()).abs().max())
    (m1, lo1, hi1), (m2, lo2, hi2) = alternate(hip, stock)
    print(f"NRMS user encoder B={B} users x {H} history items: HIP {m1:.2f} ms [{lo1:.2f}, {hi1:.2f}] ({B/m1/1e3:.2f} M users/s)"
          f"   stock torch {m2:.2f} ms [{lo2:.2f}, {hi2:.2f}]   max|diff| {diff:.2e}")


def bench_nrms_train(B=64, K=5, A=10, H=50, Lw=32, V=30000, sa=1):
    """One training step of the whole model (forward + backward, dropout 0.2): B impressions x (K candidates x (1 + A) titles + H history
    titles) through the HIP pairs against forward_stock, alternated."""
    from digat_amd import synthetic
    m = _nrms_model("NRMS-SA" if sa else "NRMS", V=V, Lw=Lw, H=H, A=A).train()
    dev = torch.device("cuda:0")

    def titles(n, seed):
        t, k = synthetic.make_titles(n, Lw, V, seed=seed)
        return torch.from_numpy(t).to(dev), torch.from_numpy(k).to(dev)
    ut, um = (x.view(B, H, Lw) for x in titles(B * H, 4))
    nt, nm = (x.view(B, K, Lw) for x in titles(B * K, 5))
    at, am = (x.view(B, K, A, Lw) for x in titles(B * K * A, 6))
    hm = (torch.arange(H)[None, :] < torch.randint(0, H + 1, (B, 1), generator=torch.Generator().manual_seed(7))).to(dev)
    label = torch.zeros(B, dtype=torch.long, device=dev)

    def step(fn):
        def run():
            m.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(fn(ut, um, hm, nt, nm, at, am), label).backward()
        return run
    (m1, lo1, hi1), (m2, lo2, hi2) = alternate(step(m), step(m.forward_stock))
    print(f"{m.model_name} training step {B} x ({K} x {1 + A if sa else 1} + {H}) titles x {Lw} tokens: HIP {m1:.2f} ms [{lo1:.2f}, {hi1:.2f}]"
          f"   stock torch {m2:.2f} ms [{lo2:.2f}, {hi2:.2f}]")


def bench_sag(n=30000, m=30000, dim=768, top_M=5, news_num=65238, hop=2, cpu_rows=32):
    """SAG construction: cosine top-k of one category of n news against an m-news corpus, and the walk over
    news_num similarity lists; the reference's per-news loop (oracle restatement) timed on cpu_rows rows beside it."""
    import time
    from digat_amd import construct_SAG, synthetic
    from oracle import sag_oracle
    dev = torch.device("cuda:0")
    title, content = synthetic.make_semantic_embeddings(max(n, m), dim, seed=3, clusters=200)
    t, c = torch.from_numpy(title).to(dev), torch.from_numpy(content).to(dev)
    ms, _ = timeit(lambda: construct_SAG.cos_topk_device(t[:n], c[:n], t[:m], c[:m], top_M), iters=3, warm=1)
    flops = 4 * 2.0 * n * m * dim
    t0 = time.perf_counter()
    sag_oracle.generate_cos_similarities(*(torch.from_numpy(x) for x in (title[:cpu_rows], content[:cpu_rows], title[:m], content[:m])), top_M)
    cpu_ms_row = (time.perf_counter() - t0) * 1e3 / cpu_rows
    print(f"SAG cosine top-{top_M + 1}: n={n} x m={m} x dim={dim}: HIP {ms:.1f} ms ({n / ms * 1e3:.0f} news/s, {flops / ms / 1e9:.1f} TFLOP/s fp32-eq)"
          f"   CPU per-news loop {cpu_ms_row:.1f} ms/news ({1e3 / cpu_ms_row:.0f} news/s, {torch.get_num_threads()} threads, {cpu_rows} rows)")
    rng = np.random.default_rng(4)
    ids, cos, length = synthetic.make_similarity_lists(rng, news_num, top_M, isolated_frac=0.02)
    nn = synthetic.news_graph_size(top_M, hop)
    dv = [torch.from_numpy(a).to(dev) for a in (ids, cos, length)]
    ms2, _ = timeit(lambda: construct_SAG.news_graph_device(*dv, top_M=top_M, hop=hop, news_node_num=nn), iters=5, warm=1)
    sub = min(news_num, 4000)
    sub_ids = np.minimum(ids[:sub], sub - 1)
    t0 = time.perf_counter()
    sag_oracle.generate_news_graph(sub_ids, cos[:sub], length[:sub], top_M, hop, nn)
    cpu2 = (time.perf_counter() - t0) * 1e3 / sub
    print(f"SAG walk: {news_num} news, top_M={top_M}, hop={hop}, {nn} nodes: HIP {ms2:.2f} ms ({news_num / ms2 / 1e3:.2f} M news/s)"
          f"   CPU walk {cpu2 * news_num:.0f} ms ({1 / cpu2:.1f} k news/s, 1 thread, {sub} rows)")


def bench_sag_lists(news_num=65238, categories=17, dim=768, top_M=5, rounds=5):
    """Embeddings -> similar-news lists for a whole corpus, two ways in one process, alternated, median [min, max] of ``rounds``
    rounds of wall clock (device synchronised): (a) one ``similar_news_lists_device`` call per category (CSR validation and upload
    included), (b) the route without the fused entry: ``cos_topk_device`` per category, its [5, n, k] tables copied to the host,
    ``similar_news_lists_host``.  Embeddings are on the device for both.  Then the news-graph walk over (a)'s lists, and
    ``build_similarity`` end to end (news bookkeeping + .npy files read from a temporary directory + upload + (a))."""
    import shutil
    import tempfile
    import time
    from digat_amd import construct_SAG, synthetic
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    share = 0.7 ** np.arange(categories)
    sizes = np.maximum((share / share.sum() * news_num).astype(np.int64), 8)
    sizes[0] += news_num - sizes.sum()
    news, serial = [], 0
    for c, size in enumerate(sizes):                                   # ~2 % of the news repeat a title; a quarter are test news
        for i in range(int(size)):
            serial += 1
            group = i if rng.random() > 0.02 or i == 0 else int(rng.integers(0, i))
            news.append(("N%d" % serial, "c%d" % c, "s", "title %d of %d" % (group, c), "abstract %d" % serial, int(rng.integers(0, 4)) % 3))
    news_ID = {"<PAD>": 0, **{n[0]: i + 1 for i, n in enumerate(news)}}
    dictionaries = {"news_ID": news_ID, "category": {"c%d" % c: c for c in range(categories)}}
    rows, _ = construct_SAG.category_rows(news)
    root = tempfile.mkdtemp(prefix="kbench_sag_")
    try:
        work, embeddings = [], {}
        for c in range(categories):
            name = "c%d" % c
            full, corpus, gs, gm, cs, cm = construct_SAG.category_tables(rows[name], news_ID, "small")
            title, content = synthetic.make_semantic_embeddings(len(full[2]), dim, seed=c)
            at = {t: i for i, t in enumerate(full[2])}
            pick = np.array([at[t] for t in corpus[2]])
            tables = (title, content, title[pick], content[pick])
            for (mode, sub), pair in zip(construct_SAG.EMBEDDING_DIRS.items(), (tables[:2], tables[2:])):
                os.makedirs(os.path.join(root, sub), exist_ok=True)
                for kind, x in zip(("title", "content"), pair):
                    np.save(os.path.join(root, sub, "%s_semantic_embeddings-%s.npy" % (kind, name)), x)
            embeddings[name] = tuple(torch.from_numpy(x).to(dev) for x in tables)
            work.append((embeddings[name], gs, gm, cs, cm))
        N = len(news_ID)
        print(f"sag-lists: {N - 1} news, {categories} categories of {int(sizes.max())} .. {int(sizes.min())} news, dim {dim}, top_M {top_M}; "
              f"{sum(len(w[1]) - 1 for w in work)} query groups, {sum(len(w[3]) - 1 for w in work)} corpus groups")
        out = tuple(torch.zeros(shape, dtype=dt, device=dev) for shape, dt in (((N, top_M), torch.int32), ((N, top_M), torch.float32), ((N,), torch.int32)))

        def fused():
            for emb, gs, gm, cs, cm in work:
                construct_SAG.similar_news_lists_device(*emb, top_M, gs, gm, cs, cm, N, out=out)

        host_out = [None]

        def unfused():
            res = (np.zeros((N, top_M), dtype=np.int32), np.zeros((N, top_M), dtype=np.float32), np.zeros(N, dtype=np.int32))
            for emb, gs, gm, cs, cm in work:
                values, indices = construct_SAG.cos_topk_device(*emb, top_M=top_M)
                values, indices = values.cpu().numpy(), indices.cpu().numpy()
                construct_SAG.similar_news_lists_host(values[4], indices[4], values.shape[2], gs, gm, cs, cm, top_M, N, out=res)
            host_out[0] = res

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        fused()
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(wall(fused))
            tb.append(wall(unfused))
        same = all(np.array_equal(o.cpu().numpy(), h) for o, h in zip(out, host_out[0]))
        stat = lambda v: "%.1f ms [%.1f, %.1f]" % (sorted(v)[len(v) // 2], min(v), max(v))
        print(f"  similar_news_lists_device per category : {stat(ta)}")
        print(f"  cos_topk_device + 5 kinds to host + host walk : {stat(tb)}   ({sorted(tb)[len(tb) // 2] / sorted(ta)[len(ta) // 2]:.1f}x; same lists: {same})")
        nn = synthetic.news_graph_size(top_M, 2)
        tw = [wall(lambda: construct_SAG.news_graph_device(*out, top_M=top_M, hop=2, news_node_num=nn)) for _ in range(rounds)]
        print(f"  news_graph_device (2 hops, {nn} nodes) over those lists : {stat(tw)}")
        td = [wall(lambda: construct_SAG.build_similarity(news, dictionaries, root, top_M, "small")) for _ in range(3)]
        print(f"  build_similarity end to end (news_meta, .npy files read, upload, lists) : {stat(td)}  (3 runs)")
    finally:
        shutil.rmtree(root, ignore_errors=True)


def bench_user_graph(G=1024, H=50, C=17, I=73152, rounds=5):
    """A scoring batch's user graphs and category masks, three ways in one process, alternated, median [min, max] of ``rounds``
    rounds: (a) the table path's two gathers (digat_gather_tables) of G consecutive impressions, (b) digat_user_graph_build with
    ``rows`` for the same impressions, (c) one build over all I impressions (MIND-small dev: 73 152).  Every call of (a) and (b)
    takes the next block of G impressions, so the table rows (a) reads come from HBM as in a scoring run, not from a warm cache.
    A launch is a few microseconds, less than its enqueue from Python: each timing replays a captured hipGraph of many launches
    (no host work between them) between two events and divides by their number."""
    from digat_amd import util
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    U, C1 = H + C, C + 1
    w = 1.0 / np.arange(1, C + 1) ** 1.2
    cats = rng.choice(C, size=(I, H), p=w / w.sum())
    hist_len = np.clip(np.round(rng.lognormal(3.0, 0.8, size=I)), 0, H).astype(np.int64)       # synthetic.make_corpus's histories
    ci = torch.from_numpy(np.where(np.arange(H)[None, :] < hist_len[:, None], cats, C).astype(np.int64)).to(dev)
    table, mask_table, entries = util.user_graphs_from_indices(ci, C, want_entries=True)
    per_node = float(entries.sum(dtype=torch.float64)) / (I * U)
    all_rows = torch.arange(I, dtype=torch.int64, device=dev)
    blocks = max(1, I // G)
    out_a = (torch.empty((G, U, U), dtype=torch.bool, device=dev), torch.empty((G, C1), dtype=torch.bool, device=dev))
    out_b = (torch.empty((G, U, U), dtype=torch.bool, device=dev), torch.empty((G, C1), dtype=torch.bool, device=dev))
    L, turn = _lib.lib(), [0, 0]

    def gather():
        rows = all_rows[(turn[0] % blocks) * G:].data_ptr()
        turn[0] += 1
        jobs = [(table.data_ptr(), out_a[0].data_ptr(), U * U, G, rows, 0, 1), (mask_table.data_ptr(), out_a[1].data_ptr(), C1, G, rows, 0, 1)]
        arr = (_lib.GatherJob * 2)(*[_lib.GatherJob(*j) for j in jobs])
        _lib.check(L.digat_gather_tables(arr, 2, _lib.stream_ptr()), "digat_gather_tables")

    def build():
        rows = all_rows[(turn[1] % blocks) * G:].data_ptr()
        turn[1] += 1
        _lib.check(L.digat_user_graph_build(ci.data_ptr(), rows, G, H, C, out_b[0].data_ptr(), out_b[1].data_ptr(), None, _lib.stream_ptr()),
                   "digat_user_graph_build")

    def build_all():
        _lib.check(L.digat_user_graph_build(ci.data_ptr(), None, I, H, C, table.data_ptr(), mask_table.data_ptr(), None, _lib.stream_ptr()),
                   "digat_user_graph_build")

    gather(); build()
    torch.cuda.synchronize()
    same = torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1])

    def captured(fn, reps):
        """``reps`` launches of fn as one hipGraph: a replay runs them back to back with no host enqueue between them."""
        turn[0] = turn[1] = 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(reps):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        return graph, reps

    def replay_us(item):
        graph, reps = item
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); graph.replay(); b.record(); b.synchronize()
        return a.elapsed_time(b) / reps * 1e3          # us per launch

    ga, gb, gc = captured(gather, 4 * blocks), captured(build, 4 * blocks), captured(build_all, 4)
    ta, tb, tc = [], [], []
    for _ in range(rounds):
        ta.append(replay_us(ga)); tb.append(replay_us(gb)); tc.append(replay_us(gc))
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = stat(ta), stat(tb), stat(tc)
    wb, wc = G * (U * U + C1), I * (U * U + C1)
    print(f"user graphs, H={H} C={C} U={U}, {per_node:.2f} entries per node, gathered == built: {same}")
    print(f"  (a) table gathers, G={G}: {ma:.1f} us [{la:.1f}, {ha:.1f}]  ({2 * wb / ma / 1e6:.2f} TB/s read + written)")
    print(f"  (b) build with rows, G={G}: {mb:.1f} us [{lb:.1f}, {hb:.1f}]  ({wb / mb / 1e6:.2f} TB/s written)")
    print(f"  (c) build over I={I}: {mc:.1f} us [{lc:.1f}, {hc:.1f}]  ({wc / mc / 1e6:.2f} TB/s written, {wc / 1e6:.0f} MB)")
    print(f"  device memory of the table path: {I * (U * U + C1) / 1e6:.0f} MB; derived: 0 (the indices, {I * H * 8 / 1e6:.0f} MB, are needed either way)")


def bench_train_input(n_behaviours=20000, rounds=5):
    """The training input through the host path (trainer.SyntheticTrainSet + Trainer.gather) and the device path
    (train_input.DeviceTrainSet), in one process, alternated, median [min, max] of ``rounds`` rounds:
    (a) one epoch's negative sampling over ``n_behaviours`` synthetic behaviours with pools of 4-58 candidates, K = 4: the host
        loop against one launch (wall time to completion, and the kernel alone between two events);
    (b) the inputs of 200 consecutive steps, B = 64, K = 4, N = 10, H = 50, C = 17: host time until the last step is enqueued,
        one synchronisation after it (the time including the drain is printed next to it);
    (c) 60 training steps (d = 400, three layers) with either input, wall time per step including the drain at the end.
    (b) and (c) run with the user graphs as a table and derived from the category indices."""
    import time
    import types
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    from digat_amd.train_input import DeviceTrainSet, negative_samples_host
    from digat_amd.trainer import SyntheticTrainSet, Trainer
    dev = torch.device("cuda:0")
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    fmt = lambda v, unit: "%.3f %s [%.3f, %.3f]" % (*stat(v)[:1], unit, *stat(v)[1:])

    # (a) sampling
    rng = np.random.default_rng(11)
    m = rng.integers(4, 59, size=n_behaviours)
    rows = int(m.sum()) + n_behaviours
    lab = np.zeros(rows, dtype=np.int8)
    starts = np.r_[0, np.cumsum(m + 1)[:-1]]
    lab[starts] = 1
    fake = types.SimpleNamespace(row_impression=np.repeat(np.arange(n_behaviours, dtype=np.int64), m + 1),
                                 row_candidate=rng.integers(1, 65000, size=rows).astype(np.int32), row_label=lab,
                                 news_node_ID=np.zeros((65000, 1), dtype=np.int64), history=np.zeros((n_behaviours, 1), dtype=np.int32))
    host_set, dev_set = SyntheticTrainSet(fake, 4, seed=0), DeviceTrainSet(fake, 4, seed=0, device=dev)
    dev_set.negative_sampling(0)
    torch.cuda.synchronize()
    same = np.array_equal(dev_set.samples_host(), negative_samples_host(dev_set.click.cpu().numpy(), dev_set.pool_offsets.cpu().numpy(),
                                                                        dev_set.pool.cpu().numpy(), 4, 0, 0))
    th, td, tk = [], [], []
    for r in range(rounds):
        t0 = time.perf_counter(); host_set.negative_sampling(); th.append((time.perf_counter() - t0) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(); dev_set.negative_sampling(); b.record()
        torch.cuda.synchronize()
        td.append((time.perf_counter() - t0) * 1e3); tk.append(a.elapsed_time(b))
    print(f"(a) negative sampling, {len(host_set)} behaviours, pools 4-58, K=4 (kernel == numpy restatement: {same})")
    print(f"    host loop   {fmt(th, 'ms')}  ({stat(th)[0] / len(host_set) * 1e3:.2f} us per behaviour)")
    print(f"    device call {fmt(td, 'ms')} to completion; the launch between two events {fmt(tk, 'ms')}")

    # (b), (c)
    spec = synthetic.SynthSpec(news_num=8192, impressions=2048, seed=3)
    corpus = synthetic.make_corpus(spec)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=3, dropout_rate=0.2,
                                epoch=1, batch_size=64, lr=1e-4, weight_decay=0.0, gradient_clip_norm=1.0)
    torch.manual_seed(0)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding), trainable=True))
    model.initialize()
    model = model.to(dev).train()
    for user_graphs in ("table", "derived"):
        dc = util.DeviceCorpus.from_numpy(corpus, dev, user_graphs=user_graphs)
        dev_set = DeviceTrainSet(corpus, 4, seed=0, device=dev)
        dev_set.negative_sampling(0)
        host_set = SyntheticTrainSet(corpus, 4, seed=0)
        host_set.samples[:] = dev_set.samples_host()
        trainers = {"host": Trainer(model, cfg, dc, host_set), "device": Trainer(model, cfg, dc, dev_set)}
        batches = {k: [b for b in t.batches(1) if (b[1] if k == "device" else len(b)) == 64] for k, t in trainers.items()}
        print(f"user graphs: {user_graphs}; {len(host_set)} behaviours, {len(batches['host'])} full batches of 64, N={spec.news_graph_size} "
              f"H={spec.max_history_num} C={spec.category_num} d={spec.embedding_dim}")
        enq, tot = {k: [] for k in trainers}, {k: [] for k in trainers}
        for r in range(rounds + 1):                                  # round 0 warms both paths
            for k, t in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(200):
                    out = t.gather(batches[k][s % len(batches[k])])
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r:
                    enq[k].append((t1 - t0) * 1e6 / 200); tot[k].append((t2 - t0) * 1e6 / 200)
        for k in trainers:
            print(f"(b) step inputs, {k:6s}: enqueue {fmt(enq[k], 'us')} per step; with the drain {fmt(tot[k], 'us')}")
        step = {k: [] for k in trainers}
        for r in range(rounds + 1):
            for k, t in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(60):
                    t.train_step(batches[k][s % len(batches[k])], read_loss=False)
                torch.cuda.synchronize()
                if r:
                    step[k].append((time.perf_counter() - t0) * 1e3 / 60)
        for k in trainers:
            print(f"(c) training step, {k:6s} input: {fmt(step[k], 'ms')} per step (60 steps, one drain)")


def bench_ablation_score(passes=50, news_num=65238, rounds=5):
    """Scoring throughput of the ablation encoders, two legs per encoder in one process, alternated (``alternate``):
    (a) the per-row path, written with the gathers of ``util.gather_batch`` and ``graph_encoder.inference`` alone — every row
        carries its own copy of the impression's user tensors and every layer runs per row;
    (b) ``util.score_rows(grouped=True)``: the pipeline, per-news context tables and per-impression user layers.
    One timed run is all ``passes`` passes of 4 096 rows.  The per-news tables (``prepare_news_side``) are built before, untimed."""
    import types
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    rows_per_pass, depth = 4096, 3
    impressions = int(passes * rows_per_pass / 37.0 * 1.03) + 8
    spec = synthetic.SynthSpec(news_num=news_num, sag_neighbors=3, sag_hops=2, impressions=impressions, seed=61)
    corpus = synthetic.make_corpus(spec)
    assert corpus.rows >= passes * rows_per_pass, (corpus.rows, passes * rows_per_pass)
    end = passes * rows_per_pass
    n_imp = int(corpus.row_impression[end - 1]) + 1
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    batches = util.launch_batches(0, end, 1024)
    print(f"ablation-score: {news_num} news, N = {spec.news_graph_size}, H = {spec.max_history_num}, C = {spec.category_num}, "
          f"d = {spec.embedding_dim}, depth {depth}; {end} rows of {n_imp} impressions in {len(batches)} passes", flush=True)
    choices = (("wo_SA", "wo_SA"), ("Seq_SA", "Seq_SA"), ("wo_interaction", "wo_interaction"),
               ("News_graph_wo_inter", "news_graph_wo_inter"), ("User_graph_wo_inter", "user_graph_wo_inter"))
    for name, choice in choices:
        cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder=choice, news_graph_size=spec.news_graph_size,
                                    max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth,
                                    dropout_rate=0.2)
        state = synthetic.make_ablation_state_dict(name, spec.embedding_dim, spec.category_num, depth, seed=62, bias_std=0.05)
        model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
        model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        model = model.to(dev).eval()
        enc = model.graph_encoder
        util.prepare_news_side(enc, dc, 1024)
        out = torch.empty(end, dtype=torch.float32, device=dev)

        def per_row():
            with torch.no_grad():
                for s, e in batches:
                    ue, Au, cm, ci, Xn, An, Mn, c0 = util.gather_batch(dc, s, e)
                    n, u = enc.inference(Xn, An, Mn, ue, Au, cm, ci, c0)
                    _lib.binding().row_logits(n, u, out[s:e])

        def grouped():
            out.copy_(util.score_rows(model, dc, 0, end, 1024, grouped=True))
        per_row()
        a = out.clone()
        grouped()
        rms = float(a.double().pow(2).mean().sqrt())
        diff = float((out - a).abs().max())
        (ma, lo_a, hi_a), (mb, lo_b, hi_b) = alternate(per_row, grouped, rounds=rounds, iters=1)
        per = lambda ms: ms / len(batches)
        print(f"  {name:20s} per-row {per(ma):7.3f} ms / 4096 rows [{per(lo_a):.3f}, {per(hi_a):.3f}]  {n_imp / ma * 1e3:9.0f} impressions/s | "
              f"grouped {per(mb):7.3f} ms [{per(lo_b):.3f}, {per(hi_b):.3f}]  {n_imp / mb * 1e3:9.0f} impressions/s | "
              f"x{ma / mb:.2f}  max|d| {diff:.2e} (rms {rms:.2e})", flush=True)
        del model, enc
        dc.news_ctx_layers = dc.c_n0 = None
        torch.cuda.empty_cache()


def bench_topk(rounds=5):
    """``digat_topk_segments`` (the C entry, buffers allocated once) against what the tree had before for the same question, in one
    process, alternated (``alternate``): ``torch.topk`` where the segments are equally long — its tie order is unspecified, so it is
    a yardstick for speed only — and ``digat_rank_metrics`` (ranks of every element, one wave per segment) on the ragged dev
    shape.  GB/s = rows x 4 B / time: the floor is one pass over the scores."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)

    def ours(scores, start, k):
        R, S = int(scores.shape[0]), int(start.shape[0]) - 1
        need = int(L.digat_topk_segments_workspace_bytes(R, S, k))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        out_s = torch.empty((S, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((S, k), dtype=torch.int64, device=dev)
        out_c = torch.empty((S,), dtype=torch.int32, device=dev)

        def run():
            _lib.check(L.digat_topk_segments(scores.data_ptr(), start.data_ptr(), R, S, None, None, 0, k, out_s.data_ptr(), out_i.data_ptr(),
                                             out_c.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), "digat_topk_segments")
        return run, (out_s, out_i, out_c)

    def line(tag, rows, a, b, other):
        (ma, lo_a, hi_a), (mb, lo_b, hi_b) = a, b
        gbs = lambda ms: rows * 4 / ms / 1e6
        print(f"  {tag:42s} digat_topk_segments {ma * 1e3:9.1f} us [{lo_a * 1e3:.1f}, {hi_a * 1e3:.1f}]  {gbs(ma):7.1f} GB/s | "
              f"{other} {mb * 1e3:9.1f} us [{lo_b * 1e3:.1f}, {hi_b * 1e3:.1f}]  {gbs(mb):7.1f} GB/s | x{mb / ma:.2f}", flush=True)

    P = 65238
    for S, ks in ((1, (10,)), (256, (10, 100))):
        scores = torch.randn(S * P, generator=g).to(dev)
        start = (torch.arange(S + 1, dtype=torch.int64) * P).to(dev)
        for k in ks:
            run, outs = ours(scores, start, k)
            run()
            want = torch.topk(scores.view(S, P), k, dim=1)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], want.values), "scores differ from torch.topk's"       # distinct values: no tie to order
            a, b = alternate(run, lambda: torch.topk(scores.view(S, P), k, dim=1), rounds=rounds, iters=10)
            line(f"{S} segment(s) of {P}, k = {k}", S * P, a, b, "torch.topk")
    rng = np.random.default_rng(0)
    lengths = np.clip(rng.poisson(37.0, size=73152), 2, 300)
    start_np = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    R = int(start_np[-1])
    scores = torch.randn(R, generator=g).to(dev)
    start = torch.from_numpy(start_np).to(dev)
    run, outs = ours(scores, start, 10)
    ranks = torch.empty(R, dtype=torch.int32, device=dev)

    def rank_all():
        _lib.check(L.digat_rank_metrics(scores.data_ptr(), None, start.data_ptr(), len(lengths), ranks.data_ptr(), None, None, _lib.stream_ptr()),
                   "digat_rank_metrics")
    run()
    rank_all()
    torch.cuda.synchronize()
    pos, cnt, rk = outs[1].cpu().numpy(), outs[2].cpu().numpy(), ranks.cpu().numpy()
    for s in range(0, len(lengths), 997):
        assert np.array_equal(rk[start_np[s] + pos[s, :cnt[s]]], np.arange(1, cnt[s] + 1)), s
    a, b = alternate(run, rank_all, rounds=rounds, iters=10)
    line(f"{len(lengths)} ragged segments ({R} rows), k = 10", R, a, b, "digat_rank_metrics")


def _recommend_setup(users, news_num, depth=3):
    """A MIND-small-shaped synthetic corpus on the device and a DIGAT model with random weights: ``(spec, model, dc)``."""
    import types
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    spec = synthetic.SynthSpec(news_num=news_num, sag_neighbors=3, sag_hops=2, impressions=max(users, 256), seed=61)
    corpus = synthetic.make_corpus(spec)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, depth, seed=62, bias_std=0.05)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return spec, model.to(dev).eval(), util.DeviceCorpus.from_numpy(corpus, dev)


def bench_recommend(users=64, news_num=65238, rounds=5):
    """``util.recommend`` for ``users`` impressions of a MIND-small-shaped corpus against the pool of all non-PAD news, k = 10, the
    history excluded: users per second, median [min, max] of ``rounds`` runs; and the selection's share (``evaluate.topk_segments``
    on scores of the same shape with the same skip rows).  The per-news tables are built before, untimed."""
    from digat_amd import evaluate, util
    dev = torch.device("cuda:0")
    depth = 3
    spec, model, dc = _recommend_setup(users, news_num, depth)
    pool = torch.arange(1, news_num, dtype=torch.int64, device=dev)
    who = np.arange(users)
    rows = users * (news_num - 1)
    print(f"recommend: {users} users x {news_num - 1} news = {rows} pairs, N = {spec.news_graph_size}, H = {spec.max_history_num}, "
          f"C = {spec.category_num}, d = {spec.embedding_dim}, depth {depth}, k = 10", flush=True)
    util.recommend(model, dc, who, pool, 10)                         # builds the per-news tables, warms every path
    torch.cuda.synchronize()
    import time
    secs = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        util.recommend(model, dc, who, pool, 10)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    secs.sort()
    med = secs[len(secs) // 2]
    print(f"  util.recommend {med:.3f} s [{secs[0]:.3f}, {secs[-1]:.3f}]: {users / med:.1f} users/s, "
          f"{med / (rows / 4096) * 1e3:.3f} ms per 4096 pairs", flush=True)
    scores = torch.randn(rows, device=dev)
    _, cand, seg = util.recommend_rows(0, users, pool, None)
    skip = dc.history[:users].contiguous()
    med_ms, best_ms = timeit(lambda: evaluate.topk_segments(scores, seg, 10, ids=cand, skip=skip), iters=10)
    print(f"  of which selection (topk_segments, ids + {skip.shape[1]}-entry skip rows): median {med_ms:.3f} ms, best {best_ms:.3f} ms "
          f"({rows * 12 / med_ms / 1e6:.1f} GB/s of scores + ids)", flush=True)
    del scores
    # the diversity sweep: one scoring pass for four diversities, beside four separate recommend(diversity=) calls
    fs = (0.0, 0.1, 0.3, 0.5)
    report = lambda: util.recommend_report(model, dc, who, pool, 10, fs)
    separate = lambda: [util.recommend(model, dc, who, pool, 10, diversity=f) for f in fs]
    report(), separate()
    torch.cuda.synchronize()
    secs = {"report": [], "separate": []}
    for _ in range(rounds):
        for name, fn in (("report", report), ("separate", separate)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
    (ra, rlo, rhi), (sa, slo, shi) = ((sorted(v)[len(v) // 2], min(v), max(v)) for v in (secs["report"], secs["separate"]))
    print(f"  util.recommend_report, {len(fs)} diversities (lists and their quality): {ra:.3f} s [{rlo:.3f}, {rhi:.3f}] | {len(fs)} x "
          f"util.recommend(diversity=) (lists alone): {sa:.3f} s [{slo:.3f}, {shi:.3f}] (x{sa / ra:.2f})", flush=True)


def bench_dot_topk(news_num=65238, d=400, rounds=5):
    """``evaluate.dot_topk`` (the fused inner-product + top-k kernel: no score matrix) against the two ways to the same lists that
    write the [G, P] matrix first — (a) ``torch.matmul`` + ``evaluate.topk_segments``, built only from what the tree had before,
    and (b) ``torch.matmul`` + ``torch.topk`` (tie order unspecified: a yardstick for speed only) — in one process, the three legs
    taken in turn, median [min, max] of ``rounds`` rounds; G in {64, 4 096} users against all but the PAD row of a MIND-small-sized
    table, k in {10, 100}.  Then ``nrms.recommend`` for 4 096 users end to end (news caches, user vectors, selection)."""
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    news = torch.randn(news_num, d, generator=g).to(dev)
    P = news_num - 1
    table = news[1:]                                                # the pool "every news but row 0" as a table of its own
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    for G in (64, 4096):
        users = torch.randn(G, d, generator=g).to(dev)
        seg = (torch.arange(G + 1, dtype=torch.int64) * P).to(dev)
        for k in (10, 100):
            fused = lambda: evaluate.dot_topk(users, table, k)
            via_segments = lambda: evaluate.topk_segments(torch.matmul(users, table.t()).view(-1), seg, k)
            via_torch = lambda: torch.topk(torch.matmul(users, table.t()), k, dim=1)
            got, want = fused(), via_torch()
            torch.cuda.synchronize()
            same = float((got[1] == want.indices).float().mean())    # the products round differently: near-ties may swap
            times = ([], [], [])
            for _ in range(rounds):
                for leg, fn in zip(times, (fused, via_segments, via_torch)):
                    leg.append(timeit(fn, iters=5, warm=1)[0])
            (a, alo, ahi), (b, blo, bhi), (c, clo, chi) = (stat(t) for t in times)
            product = timeit(lambda: evaluate.dot_scores(users, table), iters=5, warm=1)[0] if k == 10 else None
            ws = int(L.digat_dot_topk_workspace_bytes(G, P, k))
            print(f"  G = {G:5d}, P = {P}, d = {d}, k = {k:3d}: dot_topk {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({2.0 * G * P * d / a / 1e9:6.1f} TFLOP/s, "
                  f"workspace {ws / 2**20:.1f} MiB) | matmul + topk_segments {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}) | "
                  f"matmul + torch.topk {c:8.3f} ms [{clo:.3f}, {chi:.3f}] (x{c / a:.2f}) | score matrix {4.0 * G * P / 2**20:.1f} MiB | "
                  f"ids equal to torch.topk's: {same:.4f}" + (f" | dot_scores alone {product:.3f} ms" if product else ""), flush=True)
            del got, want
        del users, seg
        torch.cuda.empty_cache()
    G, H, Lw, V = 4096, 50, 32, 30000
    m = _nrms_model("NRMS", V=V, Lw=Lw, H=H).eval()
    text, mask = synthetic.make_titles(news_num, Lw, V, seed=2)
    length = torch.randint(0, H + 1, (G, 1), generator=g)
    hist_mask = torch.arange(H)[None, :] < length
    hist = torch.randint(1, news_num, (G, H), generator=g) * hist_mask
    corpus = types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                   augmented_title_text=None, augmented_title_mask=None, history_ids=hist.to(dev), history_mask=hist_mask.to(dev))
    who = np.arange(G)
    nrms.recommend(m, corpus, who, k=10)
    torch.cuda.synchronize()
    secs = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        nrms.recommend(m, corpus, who, k=10)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    med, lo, hi = stat(secs)
    vec = nrms.user_vectors(m, corpus, who)
    _, aug = nrms.news_caches(m, corpus.title_text, corpus.title_mask, None, None, 4096)
    pool = torch.arange(1, news_num, dtype=torch.int64, device=dev)
    skip = corpus.history_ids
    sel, _ = timeit(lambda: evaluate.dot_topk(vec, aug, 10, pool=pool, skip=skip), iters=5, warm=1)
    print(f"  nrms.recommend, {G} users x {P} news, k = 10, history excluded: {med:.3f} s [{lo:.3f}, {hi:.3f}] ({G / med:.0f} users/s), "
          f"of which dot_topk with the pool and {H}-entry skip rows {sel:.3f} ms", flush=True)


def bench_shortlist(rounds=5):
    """``digat_shortlist_segments`` (the C entry, buffers allocated once) on 256 segments of 65 238 scores at m in {128, 256, 1024},
    against ``torch.topk`` (tie order unspecified: a yardstick for speed only) and, at 128, against ``digat_topk_segments``; the legs
    taken in turn in one process, median [min, max] of ``rounds`` rounds.  GB/s = rows x 4 B / time: the floor is one pass."""
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    S, P = 256, 65238
    R = S * P
    scores = torch.randn(R, generator=g).to(dev)
    start = (torch.arange(S + 1, dtype=torch.int64) * P).to(dev)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def entry(name, m):
        need = int(getattr(L, name + "_workspace_bytes")(R, S, m))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        outs = (torch.empty((S, m), dtype=torch.float32, device=dev), torch.empty((S, m), dtype=torch.int64, device=dev),
                torch.empty((S,), dtype=torch.int32, device=dev))

        def run():
            _lib.check(getattr(L, name)(scores.data_ptr(), start.data_ptr(), R, S, None, None, 0, m, outs[0].data_ptr(), outs[1].data_ptr(),
                                        outs[2].data_ptr(), ws.data_ptr(), need, _lib.stream_ptr()), name)
        return run, outs, need
    print(f"shortlist: {S} segments of {P} scores; us per call, median [min, max] of {rounds} rounds", flush=True)
    for m in (128, 256, 1024):
        run, outs, need = entry("digat_shortlist_segments", m)
        stock = lambda: torch.topk(scores.view(S, P), m, dim=1)
        legs = [("digat_shortlist_segments", run), ("torch.topk", stock)]
        run()
        want = stock()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], want.values), "scores differ from torch.topk's"         # equal scores may swap their indices there
        assert torch.equal(scores.view(S, P).gather(1, outs[1]), outs[0]) and bool((outs[2] == m).all())
        if m <= 128:
            old, old_outs, _ = entry("digat_topk_segments", m)
            old()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, old_outs)), "lists differ from digat_topk_segments'"
            legs.append(("digat_topk_segments", old))
        times = [[] for _ in legs]
        for _ in range(rounds):
            for leg, (_, fn) in zip(times, legs):
                leg.append(timeit(fn, iters=10, warm=1)[0])
        base = stat(times[0])[0]
        print(f"  m = {m:4d} (workspace {need / 2**20:.1f} MiB): " + " | ".join(
            f"{name} {a * 1e3:9.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}] {R * 4 / a / 1e6:7.1f} GB/s" + ("" if n == 0 else f" (x{a / base:.2f})")
            for n, ((name, _), (a, lo, hi)) in enumerate(zip(legs, map(stat, times)))), flush=True)


def bench_dot_shortlist(news_num=65238, d=400, rounds=5):
    """``evaluate.dot_shortlist`` (scores stored a slab of 256 users at a time, then the long selection) against ``torch.matmul`` per
    1 024 users + the skip positions set to -inf + ``torch.topk`` (tie order unspecified and another rounding of the products: a
    yardstick for speed and memory only), G in {64, 4 096} users x all but the PAD row of a MIND-small-sized table, m in {256, 1024},
    50-entry skip rows; the two legs in turn in one process, median [min, max] of ``rounds`` rounds, and the peak device bytes of a
    first call (workspace included)."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    table = torch.randn(news_num, d, generator=g).to(dev)[1:].contiguous()
    P = news_num - 1

    def peak(fn):
        _lib._workspaces.clear()                                      # a first call: the workspace is part of the peak
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"dot-shortlist: P = {P} news, d = {d}, 50-entry skip rows; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (4096, 64):
        users = torch.randn(G, d, generator=g).to(dev)
        skip_pos = torch.randint(1, P, (G, 50), generator=g).to(dev)
        for m in (256, 1024):
            ours = lambda: evaluate.dot_shortlist(users, table, m, skip=skip_pos)                # no pool: the id is the position

            def stock():
                vals, idx = [], []
                for g0 in range(0, G, 1024):
                    sc = torch.matmul(users[g0:g0 + 1024], table.t())
                    sc.scatter_(1, skip_pos[g0:g0 + 1024], float("-inf"))
                    top = torch.topk(sc, m, dim=1)
                    vals.append(top.values)
                    idx.append(top.indices)
                return torch.cat(vals), torch.cat(idx)
            (got, pa), (want, pb) = peak(ours), peak(stock)
            same = float((got[1] == want[1]).float().mean())          # the products round differently: near-ties may swap
            (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=3)
            product = timeit(lambda: evaluate.dot_scores(users, table), iters=3, warm=1)[0]
            ws = int(L.digat_dot_shortlist_workspace_bytes(G, P, m, min(G, evaluate.SHORTLIST_SLAB_USERS)))
            print(f"  G = {G:5d}, m = {m:4d}: dot_shortlist {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] (workspace {ws / 2**20:.1f} MiB, peak {pa / 2**20:.1f} "
                  f"MiB) | matmul + torch.topk {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak {pb / 2**20:.1f} MiB) | score matrix "
                  f"{4.0 * G * P / 2**20:.1f} MiB | ids equal to torch.topk's: {same:.4f} | dot_scores alone {product:.3f} ms", flush=True)
            del got, want
        del users, skip_pos
        torch.cuda.empty_cache()


def bench_qdot(news_num=65238, d=400, rounds=5, demo=1):
    """The quantised first stage against the two fp32 ones: user quantisation + ``evaluate.qdot_topk`` (M = 128) / ``qdot_shortlist``
    (M = 256, 1 024) + ``evaluate.refine_lists`` to k, against ``evaluate.dot_topk`` (k = 10, 100) and against ``torch.matmul`` per
    1 024 users + the skip positions at -inf + ``evaluate.topk_segments``; G in {4 096, 64} users x all but the PAD row of a
    MIND-small-sized table, d = 400, 50-entry skip rows.  The legs run in turn in one process: median [min, max] of ``rounds`` rounds,
    the parts of the quantised leg timed alone, the peak device bytes of a first call of every leg, the index build.  Then (``demo``)
    ``nrms.index_report`` on the planted-signal corpus with the retriever ``fit_retriever``'s demonstration trains."""
    import types
    from digat_amd import evaluate, nrms, synthetic
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    table = torch.randn(news_num, d, generator=g).to(dev)[1:].contiguous()
    P = news_num - 1
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    fmt = lambda s: f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"

    def peak(fn):
        _lib._workspaces.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    build = timeit(lambda: evaluate.quantize_rows(table), iters=5, warm=2)[0]
    qn, sn = evaluate.quantize_rows(table)
    print(f"qdot: P = {P} news, d = {d}, 50-entry skip rows; ms per call, median [min, max] of {rounds} rounds; index build "
          f"(quantize_rows of the table): {build:.3f} ms, codes {qn.numel() / 2**20:.1f} MiB beside {4.0 * table.numel() / 2**20:.1f} MiB", flush=True)
    for G in (4096, 64):
        users = torch.randn(G, d, generator=g).to(dev)
        skip_pos = torch.randint(1, P, (G, 50), generator=g).to(dev)
        seg = torch.arange(0, 1025, device=dev) * P
        for k in (10, 100):
            exact = lambda: evaluate.dot_topk(users, table, k, skip=skip_pos)

            def stock():
                out = []
                for g0 in range(0, G, 1024):
                    sc = torch.matmul(users[g0:g0 + 1024], table.t())
                    sc.scatter_(1, skip_pos[g0:g0 + 1024], float("-inf"))
                    out.append(evaluate.topk_segments(sc.view(-1), seg[:sc.shape[0] + 1], k))
                return out
            want, pe = peak(exact)
            _, ps = peak(stock)
            for M in (128, 256, 1024):
                if M < k:
                    continue

                def first(M=M):
                    qu, su = evaluate.quantize_rows(users)
                    if M <= 128:
                        return evaluate.qdot_topk(qu, su, qn, sn, M, skip=skip_pos)
                    return evaluate.qdot_shortlist(qu, su, qn, sn, M, skip=skip_pos)

                def ours(M=M):
                    _, ids, cnt = first(M)
                    return evaluate.refine_lists(users, table, ids, cnt, k)
                got, pq = peak(ours)
                inside = float(((got[1].unsqueeze(2) == want[1].unsqueeze(1)).any(dim=1) | (want[1] < 0)).all(dim=1).float().mean())
                legs = [[], [], []]
                for _ in range(rounds):
                    for leg, fn in zip(legs, (ours, exact, stock)):
                        leg.append(timeit(fn, iters=3, warm=1)[0])
                t_first = timeit(first, iters=3, warm=1)[0]
                _, ids, cnt = first()
                t_refine = timeit(lambda: evaluate.refine_lists(users, table, ids, cnt, k), iters=3, warm=1)[0]
                qu, su = evaluate.quantize_rows(users)
                t_scores = timeit(lambda: evaluate.qdot_scores(qu, su, qn, sn), iters=3, warm=1)[0] if G <= 1024 else float("nan")
                a, b, c = (stat(v) for v in legs)
                print(f"  G = {G:5d}, k = {k:3d}, M = {M:4d}: quantised + refine {fmt(a)} (first stage {t_first:.3f}, refine_lists {t_refine:.3f}, "
                      f"qdot_scores alone {t_scores:.3f}; peak {pq / 2**20:.1f} MiB) | dot_topk {fmt(b)} (x{b[0] / a[0]:.2f}, peak {pe / 2**20:.1f} MiB) | "
                      f"matmul + topk_segments {fmt(c)} (x{c[0] / a[0]:.2f}, peak {ps / 2**20:.1f} MiB) | users whose dot_topk list is "
                      f"returned whole: {inside:.4f}", flush=True)
                del got, ids, cnt
            del want
        del users, skip_pos
        torch.cuda.empty_cache()
    if not demo:
        return
    corpus = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    N, H, Lw, V = corpus.spec.news_num, corpus.spec.max_history_num, 16, 4000
    text, mask = synthetic.make_titles(N, Lw, V, seed=2)

    def part(lo, hi):
        c = synthetic.slice_impressions(corpus, lo, hi)
        hist = torch.from_numpy(c.history.astype(np.int64)).to(dev)
        return types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                     augmented_title_text=None, augmented_title_mask=None, history_ids=hist, history_mask=hist != 0,
                                     row_candidate=c.row_candidate.astype(np.int64), row_impression=c.row_impression, row_label=c.row_label)
    held, train = part(0, synthetic.PLANTED_DEV_IMPRESSIONS), part(synthetic.PLANTED_DEV_IMPRESSIONS, corpus.spec.impressions)
    m = _nrms_model("NRMS", V=V, dm=64, h=8, dk=8, att=32, Lw=Lw, H=H, dropout=0.2)
    nrms.fit_retriever(m, train, 400, batch_users=256, lr=1e-3, seed=0)
    users = np.arange(int(held.history_ids.shape[0]))
    print(f"  index_report: planted-signal corpus, {N - 1} news, NRMS at d = 64 after fit_retriever's 400 steps, {len(users)} held-out "
          f"impressions, k = 10; 95 % intervals over users", flush=True)
    for r in nrms.index_report(m, held, users, k=10, ms=(32, 64, 128, 256)):
        iv = r["intervals"]
        cell = lambda name: f"{r[name]:.4f} [{iv[name]['lo']:.4f}, {iv[name]['hi']:.4f}]"
        print(f"    M = {r['m']:4d}: containment {cell('containment')}, agreement@10 {cell('agreement')}", flush=True)


def matrix_ranks(users, table, pos, skip_pos, product, chunk=1024):
    """The ranks of ``evaluate.dot_rank`` built from what the tree had before it: per chunk of users the [chunk, P] score matrix
    (``product(users, table)``), then torch compares and sums against every target's own score with the skip mask.  ``pos`` [G, t]
    target positions, ``skip_pos`` [G, L] skipped positions.  Plain float compares: NaNs and signed zeros are not the
    contract's (there are none in the benchmark's data)."""
    G, P = users.shape[0], table.shape[0]
    where = torch.arange(P, device=users.device)[None, :]
    out = torch.empty(pos.shape, dtype=torch.int32, device=users.device)
    for g0 in range(0, G, chunk):
        S = product(users[g0:g0 + chunk], table)
        sp = skip_pos[g0:g0 + chunk]
        elem = torch.ones(S.shape, dtype=torch.bool, device=S.device)
        elem.scatter_(1, sp, False)
        for j in range(pos.shape[1]):
            q = pos[g0:g0 + chunk, j:j + 1]
            own = S.gather(1, q)
            before = ((S > own) | ((S == own) & (where < q))) & elem
            out[g0:g0 + chunk, j] = torch.where(elem.gather(1, q)[:, 0], before.sum(dim=1), torch.full_like(q[:, 0], -1)).to(torch.int32)
    return out


def bench_dot_rank(news_num=65238, d=400, rounds=5):
    """``evaluate.dot_rank`` (the fused inner-product + rank-of-target kernel: no score matrix) against the same ranks built from
    what the tree had before it — the [1 024, P] score matrix per chunk of users from ``evaluate.dot_scores`` (same bits: the ranks
    must be equal) or ``torch.matmul`` (near-ties may differ), then torch compares and sums with the skip mask (``matrix_ranks``) —
    in one process, the three legs taken in turn, median [min, max] of ``rounds`` rounds, and each leg's peak of device bytes
    beyond its inputs; G in {64, 4 096} users against all but the PAD row of a MIND-small-sized table, one and five targets per
    user, 50-entry skip rows.  Then ``nrms.retrieval_metrics`` for 4 096 users end to end."""
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    news = torch.randn(news_num, d, generator=g).to(dev)
    P = news_num - 1
    table = news[1:].contiguous()
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"dot-rank: P = {P} news, d = {d}, 50-entry skip rows; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        users = torch.randn(G, d, generator=g).to(dev)
        skip_pos = torch.randint(1, P, (G, 50), generator=g).to(dev)
        for per in (1, 5):
            pos = torch.randint(0, P, (G, per), generator=g).to(dev)
            start = np.arange(G + 1, dtype=np.int64) * per
            flat = pos.reshape(-1).contiguous()
            fused = lambda: evaluate.dot_rank(users, table, flat, start, skip=skip_pos)[0]      # no pool: the id is the position
            via_scores = lambda: matrix_ranks(users, table, pos, skip_pos, evaluate.dot_scores)
            via_matmul = lambda: matrix_ranks(users, table, pos, skip_pos, lambda u, t: torch.matmul(u, t.t()))
            (got, pa), (want, pb), (near, pc) = peak(fused), peak(via_scores), peak(via_matmul)
            exact = bool(torch.equal(got.view(G, per), want))
            close = float((got.view(G, per) == near).float().mean())
            times = ([], [], [])
            for _ in range(rounds):
                for leg, fn in zip(times, (fused, via_scores, via_matmul)):
                    leg.append(timeit(fn, iters=3, warm=1)[0])
            (a, alo, ahi), (b, blo, bhi), (c, clo, chi) = (stat(t) for t in times)
            ws = int(L.digat_dot_rank_workspace_bytes(G, P, G * per))
            print(f"  G = {G:5d}, {per} target(s) per user: dot_rank {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({2.0 * G * P * d / a / 1e9:6.1f} TFLOP/s, "
                  f"workspace {ws} B, peak {pa / 2**20:.2f} MiB) | dot_scores + torch {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
                  f"{pb / 2**20:.1f} MiB) | matmul + torch {c:8.3f} ms [{clo:.3f}, {chi:.3f}] (x{c / a:.2f}, peak {pc / 2**20:.1f} MiB) | "
                  f"ranks equal to the dot_scores leg's: {exact}, share equal to the matmul leg's: {close:.4f}", flush=True)
            del got, want, near
        del users, skip_pos
        torch.cuda.empty_cache()
    G, H, Lw, V = 4096, 50, 32, 30000
    m = _nrms_model("NRMS", V=V, Lw=Lw, H=H).eval()
    text, mask = synthetic.make_titles(news_num, Lw, V, seed=2)
    length = torch.randint(0, H + 1, (G, 1), generator=g)
    hist_mask = torch.arange(H)[None, :] < length
    hist = torch.randint(1, news_num, (G, H), generator=g) * hist_mask
    corpus = types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                   augmented_title_text=None, augmented_title_mask=None, history_ids=hist.to(dev), history_mask=hist_mask.to(dev))
    who = np.arange(G)
    targets = (torch.randint(1, news_num, (G,), generator=g).numpy(), np.arange(G + 1, dtype=np.int64))
    res = nrms.retrieval_metrics(m, corpus, who, targets=targets)
    torch.cuda.synchronize()
    secs = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        nrms.retrieval_metrics(m, corpus, who, targets=targets)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    med, lo, hi = stat(secs)
    vec = nrms.user_vectors(m, corpus, who)
    _, aug = nrms.news_caches(m, corpus.title_text, corpus.title_mask, None, None, 4096)
    pool = torch.arange(1, news_num, dtype=torch.int64, device=dev)
    tpos = torch.from_numpy(targets[0] - 1).to(dev)
    sel, _ = timeit(lambda: evaluate.dot_rank(vec, aug, tpos, targets[1], pool=pool, skip=corpus.history_ids), iters=5, warm=1)
    print(f"  nrms.retrieval_metrics, {G} users x {P} news, one target each, history excluded: {med:.3f} s [{lo:.3f}, {hi:.3f}] "
          f"({G / med:.0f} users/s), of which dot_rank with the pool and {H}-entry skip rows {sel:.3f} ms; recall@128 {res['recall@128']:.4f}, "
          f"median rank {res['median_rank']:.0f}, not ranked {res['not_ranked']}", flush=True)


def stock_pool_softmax(users, table, pos, skip_pos, scale=1.0, chunk=1024):
    """The loss of ``evaluate.pool_softmax`` from stock PyTorch: per chunk of users the [chunk, P] scores (``torch.matmul``), the
    skip positions masked out, ``logsumexp``, the targets gathered.  ``pos`` [G, t] target positions, ``skip_pos`` [G, L].  A target
    inside its user's skip row is not treated (there is none in the benchmark's data).  Returns the summed loss."""
    total = users.new_zeros(())
    for g0 in range(0, users.shape[0], chunk):
        x = scale * torch.matmul(users[g0:g0 + chunk], table.t())
        masked = x.scatter(1, skip_pos[g0:g0 + chunk], float("-inf"))
        total = total + (torch.logsumexp(masked, dim=1, keepdim=True) - x.gather(1, pos[g0:g0 + chunk])).sum()
    return total


def bench_pool_softmax(news_num=65238, d=400, rounds=5):
    """``evaluate.pool_softmax`` (the fused full-pool softmax loss and its gradients: no score matrix) against ``stock_pool_softmax``
    under autograd, in one process, the legs taken in turn, median [min, max] of ``rounds`` rounds of three calls, and each leg's
    peak of device bytes beyond its inputs; forward alone (``no_grad``) and forward + backward.  Then ``nrms.fit_retriever`` on the
    planted-signal corpus (``synthetic.PLANTED_SPEC`` with random titles): ``nrms.retrieval_metrics`` of the held-out impressions
    before and after."""
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(0)
    P = news_num - 1
    table = (torch.randn(P, d, generator=g) / d ** 0.5).to(dev)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        out = float(out)
        return out, torch.cuda.max_memory_allocated() - base
    print(f"pool-softmax: P = {P} news, d = {d}, 50-entry skip rows; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        users = (3.0 * torch.randn(G, d, generator=g)).to(dev)
        skip_pos = torch.randint(1, P, (G, 50), generator=g).to(dev)
        for per in (1, 5):
            pos = torch.randint(0, P, (G, per), generator=g).to(dev)
            pos = torch.where((pos[:, :, None] == skip_pos[:, None, :]).any(dim=2), torch.zeros_like(pos), pos)   # position 0 is never skipped
            start = np.arange(G + 1, dtype=np.int64) * per
            flat = pos.reshape(-1).contiguous()

            def fused_fwd():
                with torch.no_grad():
                    return evaluate.pool_softmax(users, table, flat, start, skip=skip_pos)[0].sum()

            def stock_fwd():
                with torch.no_grad():
                    return stock_pool_softmax(users, table, pos, skip_pos)

            def both(fn):
                def run():
                    u, t = users.detach().requires_grad_(True), table.detach().requires_grad_(True)
                    loss = fn(u, t)
                    loss.backward()
                    return loss.detach() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])
                return run
            fused_both = both(lambda u, t: evaluate.pool_softmax(u, t, flat, start, skip=skip_pos)[0].sum())
            stock_both = both(lambda u, t: stock_pool_softmax(u, t, pos, skip_pos))
            legs = (fused_fwd, stock_fwd, fused_both, stock_both)
            peaks = [peak(fn) for fn in legs]
            times = [[] for _ in legs]
            for _ in range(rounds):
                for leg, fn in zip(times, legs):
                    leg.append(timeit(fn, iters=3, warm=1)[0])
            (a, alo, ahi), (b, blo, bhi), (c, clo, chi), (e, elo, ehi) = (stat(t) for t in times)
            ws = int(L.digat_pool_softmax_workspace_bytes(G, P, G * per, d))
            print(f"  G = {G:5d}, {per} target(s) per user: forward: pool_softmax {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] (peak {peaks[0][1] / 2**20:.2f} "
                  f"MiB) | stock {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak {peaks[1][1] / 2**20:.1f} MiB) || forward + backward: "
                  f"pool_softmax {c:8.3f} ms [{clo:.3f}, {chi:.3f}] ({6.0 * G * P * d / c / 1e9:5.1f} TFLOP/s, workspace {ws / 2**20:.1f} MiB, peak "
                  f"{peaks[2][1] / 2**20:.1f} MiB) | stock {e:8.3f} ms [{elo:.3f}, {ehi:.3f}] (x{e / c:.2f}, peak {peaks[3][1] / 2**20:.1f} MiB) | "
                  f"summed loss {peaks[0][0]:.3f} vs stock {peaks[1][0]:.3f}", flush=True)
        del users, skip_pos
        torch.cuda.empty_cache()
    # the first stage trained for retrieval on the planted-signal corpus
    corpus = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    N, H, Lw, V = corpus.spec.news_num, corpus.spec.max_history_num, 16, 4000
    text, mask = synthetic.make_titles(N, Lw, V, seed=2)

    def part(lo, hi):
        c = synthetic.slice_impressions(corpus, lo, hi)
        hist = torch.from_numpy(c.history.astype(np.int64)).to(dev)
        return types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                     augmented_title_text=None, augmented_title_mask=None, history_ids=hist, history_mask=hist != 0,
                                     row_candidate=c.row_candidate.astype(np.int64), row_impression=c.row_impression, row_label=c.row_label)
    held, train = part(0, synthetic.PLANTED_DEV_IMPRESSIONS), part(synthetic.PLANTED_DEV_IMPRESSIONS, corpus.spec.impressions)
    m = _nrms_model("NRMS", V=V, dm=64, h=8, dk=8, att=32, Lw=Lw, H=H, dropout=0.2)
    report = lambda r, l: (f"recall@10 {r['recall@10']:.4f}, recall@100 {r['recall@100']:.4f}, median rank {r['median_rank']:.0f}, "
                           f"targets {r['targets']}, not ranked {r['not_ranked']}, retrieval loss {l['nll']:.4f}")
    print(f"  planted-signal corpus, {N - 1} news, held-out impressions [0, {synthetic.PLANTED_DEV_IMPRESSIONS}): before: "
          + report(nrms.retrieval_metrics(m, held), nrms.retrieval_loss(m, held)), flush=True)
    steps = 400
    t0 = time.perf_counter()
    losses = nrms.fit_retriever(m, train, steps, batch_users=256, lr=1e-3, seed=0)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print(f"  nrms.fit_retriever: {steps} steps of 256 users against the full pool, lr 1e-3: {secs:.1f} s ({1e3 * secs / steps:.1f} ms per step), "
          f"loss {np.mean(losses[:10]):.4f} (first ten steps) -> {np.mean(losses[-10:]):.4f} (last ten); after: "
          + report(nrms.retrieval_metrics(m, held), nrms.retrieval_loss(m, held)), flush=True)


def stock_list_softmax(users, rows, ids, count, teacher, scale=1.0, temperature=1.0):
    """The summed loss of ``evaluate.list_softmax`` from stock PyTorch: ``index_select`` into [G, M, d], ``torch.bmm``, ``log_softmax``
    over the slots below ``count``, ``F.kl_div`` against ``softmax(teacher / temperature)``.  Every id is a row and every teacher value
    finite in the benchmark's data."""
    G, M = ids.shape
    x = scale * torch.bmm(rows.index_select(0, ids.reshape(-1)).view(G, M, -1), users.unsqueeze(2)).squeeze(2)
    out = torch.arange(M, device=ids.device)[None, :] >= count[:, None]
    logp = torch.log_softmax(x.masked_fill(out, float("-inf")), dim=1)
    logq = torch.log_softmax((teacher / temperature).masked_fill(out, float("-inf")), dim=1)
    return torch.nn.functional.kl_div(logp.masked_fill(out, 0.0), logq.masked_fill(out, 0.0), reduction="sum", log_target=True)


def bench_list_softmax(d=400, rounds=5, demo=1):
    """``evaluate.list_softmax`` (the fused per-user list softmax and its gradients: no [G, M, d] gather, no float atomics) against
    ``stock_list_softmax`` under autograd, in one process, the legs taken in turn, median [min, max] of ``rounds`` rounds of three
    calls, and each leg's peak of device bytes beyond its inputs; forward alone (``no_grad``) and forward + backward.  The pool is
    compact: the distinct ids of the batch's lists, drawn from min(65 237, G M / 4) rows.  Then (``demo``) the demonstration run:
    ``nrms.distil_retriever`` on the planted-signal corpus, the trained DIGAT (tests/golden/trained_planted_state.npz) teaching an
    NRMS at d = 64 on its own shortlists of 256."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        out = float(out)
        return out, torch.cuda.max_memory_allocated() - base
    print(f"list-softmax: d = {d}, compact pool, temperature 2; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            P = max(M, min(65237, G * M // 4))
            rows = (torch.randn(P, d, generator=g) / d ** 0.5).to(dev)
            users = (3.0 * torch.randn(G, d, generator=g)).to(dev)
            ids = torch.stack([torch.randperm(P, generator=g)[:M] for _ in range(G)]).to(dev)       # no id twice in a list, many times across lists
            count = torch.randint(M // 2, M + 1, (G,), generator=g).to(torch.int32).to(dev)
            teacher = (3.0 * torch.randn(G, M, generator=g)).to(dev)

            def fused_fwd():
                with torch.no_grad():
                    return evaluate.list_softmax(users, rows, ids, count, teacher, temperature=2.0)[0].sum()

            def stock_fwd():
                with torch.no_grad():
                    return stock_list_softmax(users, rows, ids, count, teacher, temperature=2.0)

            def both(fn):
                def run():
                    u, t = users.detach().requires_grad_(True), rows.detach().requires_grad_(True)
                    loss = fn(u, t)
                    loss.backward()
                    return loss.detach() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])
                return run
            fused_both = both(lambda u, t: evaluate.list_softmax(u, t, ids, count, teacher, temperature=2.0)[0].sum())
            stock_both = both(lambda u, t: stock_list_softmax(u, t, ids, count, teacher, temperature=2.0))
            legs = (fused_fwd, stock_fwd, fused_both, stock_both)
            peaks = [peak(fn) for fn in legs]
            times = [[] for _ in legs]
            for _ in range(rounds):
                for leg, fn in zip(times, legs):
                    leg.append(timeit(fn, iters=3, warm=1)[0])
            (a, alo, ahi), (b, blo, bhi), (c, clo, chi), (e, elo, ehi) = (stat(t) for t in times)
            print(f"  G = {G:5d}, M = {M:4d}, P = {P:5d}: forward: list_softmax {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] (peak {peaks[0][1] / 2**20:.2f} "
                  f"MiB) | stock {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak {peaks[1][1] / 2**20:.1f} MiB) || forward + backward: "
                  f"list_softmax {c:8.3f} ms [{clo:.3f}, {chi:.3f}] (gather {8.0 * G * M * d / c / 1e6:6.1f} GB/s, peak {peaks[2][1] / 2**20:.1f} "
                  f"MiB) | stock {e:8.3f} ms [{elo:.3f}, {ehi:.3f}] (x{e / c:.2f}, peak {peaks[3][1] / 2**20:.1f} MiB) | "
                  f"summed loss {peaks[0][0]:.3f} vs stock {peaks[1][0]:.3f}", flush=True)
            del rows, users, ids, count, teacher
            torch.cuda.empty_cache()
    if demo:
        demo_distil()


def demo_distil(train_users=2048, held_users=1024, m=256, steps=300, temperature=2.0, replicates=2000):
    """The demonstration run of listwise distillation: on the planted-signal corpus the trained DIGAT
    (tests/golden/trained_planted_state.npz) teaches an NRMS at d = 64 with random titles.  The lists are the student's own
    ``nrms.shortlist`` (m = 256) of ``train_users`` training impressions, scored once by ``util.score_lists``.  Reported, before and
    after ``nrms.distil_retriever``, on ``held_users`` held-out impressions: ``nrms.teacher_agreement`` @10 of the student's shortlist
    with the teacher's top 10 over the whole catalogue (``util.recommend``), and ``nrms.retrieval_metrics``' recall@k of the held-out
    clicks, each with ``evaluate.metric_intervals`` / ``rank_metrics_intervals``."""
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {k: v for k, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    corpus = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    spec = corpus.spec
    N, H, Lw, V = spec.news_num, spec.max_history_num, 16, 4000
    text, mask = synthetic.make_titles(N, Lw, V, seed=2)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size, max_history_num=H,
                                category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    digat = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    digat.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    digat = digat.to(dev).eval()

    def part(lo, hi):
        c = synthetic.slice_impressions(corpus, lo, hi)
        hist = torch.from_numpy(c.history.astype(np.int64)).to(dev)
        ns = types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                   augmented_title_text=None, augmented_title_mask=None, history_ids=hist, history_mask=hist != 0,
                                   row_candidate=c.row_candidate.astype(np.int64), row_impression=c.row_impression, row_label=c.row_label)
        return ns, util.DeviceCorpus.from_numpy(c, dev)
    (held, dc_held), (train, dc_train) = part(0, synthetic.PLANTED_DEV_IMPRESSIONS), part(synthetic.PLANTED_DEV_IMPRESSIONS, spec.impressions)
    student = _nrms_model("NRMS", V=V, dm=64, h=8, dk=8, att=32, Lw=Lw, H=H, dropout=0.2)
    hu = np.arange(held_users, dtype=np.int64)
    pool = np.arange(1, N, dtype=np.int64)
    t_ids, _, t_count = util.recommend(digat, dc_held, hu, pool, 10)

    def report(tag):
        s_ids, _, s_count = nrms.shortlist(student, held, hu, m=m)
        agree = nrms.teacher_agreement(s_ids, s_count, t_ids, t_count, ks=(10,))
        iv = evaluate.metric_intervals(agree["per_user"], names=agree["names"], replicates=replicates)
        r = nrms.retrieval_metrics(student, held, users=hu, ks=(10, 100, m), intervals=replicates)
        fmt = lambda f: f"{f['value']:.4f} [{f['lo']:.4f}, {f['hi']:.4f}]" if isinstance(f, dict) and "lo" in f else str(f)
        print(f"  {tag}: teacher_agreement@10 of the shortlist of {m}: {fmt(iv['agreement@10'])}; held-out clicks: "
              + ", ".join(f"recall@{k} {fmt(r['intervals'][f'recall@{k}'])}" for k in (10, 100, m))
              + f", median rank {r['median_rank']:.0f} ({r['targets']} targets)", flush=True)
        return agree["agreement@10"]
    print(f"distillation demo: planted-signal corpus, {N - 1} news; teacher: the trained DIGAT; student: NRMS at d = 64, random titles; "
          f"{held_users} held-out users, 95 % intervals from {replicates} replicates over users", flush=True)
    report("before")
    tu = np.arange(train_users, dtype=np.int64)
    t0 = time.perf_counter()
    ids, _, count = nrms.shortlist(student, train, tu, m=m)
    teacher = util.score_lists(digat, dc_train, tu, ids, count)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    losses = nrms.distil_retriever(student, train, (tu, ids, teacher, count), steps, batch_users=64, lr=1e-3, seed=0, temperature=temperature)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"  lists: nrms.shortlist + util.score_lists for {train_users} users x {m}: {t1 - t0:.1f} s; nrms.distil_retriever: {steps} steps of "
          f"64 lists, lr 1e-3, temperature {temperature}: {t2 - t1:.1f} s ({1e3 * (t2 - t1) / steps:.1f} ms per step), mean KL "
          f"{np.mean(losses[:10]):.4f} (first ten steps) -> {np.mean(losses[-10:]):.4f} (last ten)", flush=True)
    report("after")


def stock_list_pairwise(users, rows, ids, count, gain, disc, backward=False, budget=1 << 30):
    """The summed loss of ``evaluate.list_pairwise`` from stock PyTorch under autograd, the lists in chunks whose [g, M, M] float32
    intermediates hold ``budget`` bytes each: ``index_select`` + ``torch.bmm``, ranks from a stable ``argsort``, the [g, M, M]
    differences of scores, gains and discounts, ``softplus``.  ``backward``: every chunk's loss is differentiated as soon as it
    stands, so that one chunk's graph lives at a time.  Every id is a row and every gain finite and >= 0 in the benchmark's data."""
    G, M = ids.shape
    step = max(1, budget // (4 * M * M))
    slot = torch.arange(M, device=ids.device)
    total = torch.zeros((), device=ids.device)
    for lo in range(0, G, step):
        sl = slice(lo, lo + step)
        g = ids[sl].shape[0]
        x = torch.bmm(rows.index_select(0, ids[sl].reshape(-1)).view(g, M, -1), users[sl].unsqueeze(2)).squeeze(2)
        with torch.no_grad():
            out = slot[None, :] >= count[sl][:, None]
            order = torch.argsort(x.masked_fill(out, float("-inf")), dim=1, descending=True, stable=True)
            r = torch.empty_like(order).scatter_(1, order, slot[None, :].expand(g, M))
            gn = gain[sl].masked_fill(out, 0.0)
            Dr = disc[r].masked_fill(out, 0.0)
            idcg = (torch.sort(gn, dim=1, descending=True).values * disc[None, :]).sum(dim=1).clamp(min=1e-30)
            W = torch.relu(gn[:, :, None] - gn[:, None, :]) * (Dr[:, :, None] - Dr[:, None, :]).abs() / idcg[:, None, None]
            W = W.masked_fill(out[:, :, None] | out[:, None, :], 0.0)
        loss = (W * torch.nn.functional.softplus(-(x[:, :, None] - x[:, None, :]))).sum()
        if backward:
            loss.backward()
        total = total + loss.detach()
    return total


def bench_list_pairwise(d=400, rounds=5, demo=1):
    """``evaluate.list_pairwise`` (the fused pairwise nDCG loss and its gradients: no [G, M, M] tensor, no [G, M, d] gather, fp64 pair
    arithmetic, no float atomics) against ``stock_list_pairwise`` (float32, chunked to 1 GiB intermediates) under autograd, in one
    process, the legs taken in turn, median [min, max] of ``rounds`` rounds of three calls, and each leg's peak of device bytes beyond
    its inputs; forward alone (``no_grad``) and forward + backward; click gains (one to three ones a list) and all-distinct gains
    (every pair live).  The pool is compact, as in ``bench_list_softmax``.  Then (``demo``) ``demo_rank``."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        out = float(out)
        return out, torch.cuda.max_memory_allocated() - base
    print(f"list-pairwise: d = {d}, compact pool, full discount; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            P = max(M, min(65237, G * M // 4))
            rows = (torch.randn(P, d, generator=g) / d ** 0.5).to(dev)
            users = (3.0 * torch.randn(G, d, generator=g)).to(dev)
            ids = torch.stack([torch.randperm(P, generator=g)[:M] for _ in range(G)]).to(dev)
            count = torch.randint(M // 2, M + 1, (G,), generator=g).to(torch.int32).to(dev)
            D = evaluate.ndcg_discount(M)
            disc = torch.from_numpy(D).float().to(dev)
            clicks = torch.zeros(G, M)
            for row in clicks:
                row[torch.randperm(M // 2, generator=g)[:int(torch.randint(1, 4, (1,), generator=g))]] = 1.0
            distinct = torch.stack([torch.randperm(M, generator=g).float() for _ in range(G)]) * 0.25
            for tag, gain in (("click gains", clicks.to(dev)), ("distinct gains", distinct.to(dev))):
                def fused_fwd():
                    with torch.no_grad():
                        return evaluate.list_pairwise(users, rows, ids, count, gain, discount=D)[0].sum()

                def stock_fwd():
                    with torch.no_grad():
                        return stock_list_pairwise(users, rows, ids, count, gain, disc)

                def fused_both():
                    u, t = users.detach().requires_grad_(True), rows.detach().requires_grad_(True)
                    loss = evaluate.list_pairwise(u, t, ids, count, gain, discount=D)[0].sum()
                    loss.backward()
                    return loss.detach() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])

                def stock_both():
                    u, t = users.detach().requires_grad_(True), rows.detach().requires_grad_(True)
                    loss = stock_list_pairwise(u, t, ids, count, gain, disc, backward=True)
                    return loss + 0.0 * (u.grad[0, 0] + t.grad[0, 0])
                legs = (fused_fwd, stock_fwd, fused_both, stock_both)
                peaks = [peak(fn) for fn in legs]
                times = [[] for _ in legs]
                for _ in range(rounds):
                    for leg, fn in zip(times, legs):
                        leg.append(timeit(fn, iters=3, warm=1)[0])
                (a, alo, ahi), (b, blo, bhi), (c, clo, chi), (e, elo, ehi) = (stat(t) for t in times)
                print(f"  G = {G:5d}, M = {M:4d}, P = {P:5d}, {tag}: forward: list_pairwise {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] (peak "
                      f"{peaks[0][1] / 2**20:.2f} MiB) | stock {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak {peaks[1][1] / 2**20:.1f} MiB) || "
                      f"forward + backward: list_pairwise {c:8.3f} ms [{clo:.3f}, {chi:.3f}] (peak {peaks[2][1] / 2**20:.1f} MiB) | stock {e:8.3f} ms "
                      f"[{elo:.3f}, {ehi:.3f}] (x{e / c:.2f}, peak {peaks[3][1] / 2**20:.1f} MiB) | summed loss {peaks[0][0]:.3f} vs stock "
                      f"{peaks[1][0]:.3f}", flush=True)
            del rows, users, ids, count, clicks, distinct
            torch.cuda.empty_cache()
    if demo:
        demo_rank()


def demo_rank(train_users=2048, steps=300, k=10, replicates=2000):
    """The demonstration run of the pairwise nDCG loss: on the planted-signal corpus two copies of one NRMS at d = 64 (random titles)
    are trained on the whole impressions of ``train_users`` training users with the same seeded draws, steps and learning rate — one
    by ``nrms.fit_ranker`` on ``impression_gain_lists`` (click gains, nDCG@``k`` weights), one by ``nrms.distil_retriever`` on
    ``impression_lists`` (the listwise click softmax).  Both score the held-out impressions with ``nrms.compute_scores``;
    ``evaluate.compare_metrics`` gives the paired intervals of the per-impression AUC, MRR, nDCG@5 and nDCG@10.  The mean nDCG@``k``
    of the training lists themselves, before and after, says whether the steps fit what they were given."""
    import copy
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic
    dev = torch.device("cuda:0")
    corpus = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    spec = corpus.spec
    N, H, Lw, V = spec.news_num, spec.max_history_num, 16, 4000
    text, mask = synthetic.make_titles(N, Lw, V, seed=2)

    def part(lo, hi):
        c = synthetic.slice_impressions(corpus, lo, hi)
        hist = torch.from_numpy(c.history.astype(np.int64)).to(dev)
        return types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                     augmented_title_text=None, augmented_title_mask=None, history_ids=hist, history_mask=hist != 0,
                                     row_candidate=c.row_candidate.astype(np.int64), row_impression=c.row_impression, row_label=c.row_label)
    held, train = part(0, synthetic.PLANTED_DEV_IMPRESSIONS), part(synthetic.PLANTED_DEV_IMPRESSIONS, spec.impressions)
    ranker = _nrms_model("NRMS", V=V, dm=64, h=8, dk=8, att=32, Lw=Lw, H=H, dropout=0.2)
    softmax = copy.deepcopy(ranker)
    tu = np.arange(train_users, dtype=np.int64)
    gains, clicks = nrms.impression_gain_lists(train, tu), nrms.impression_lists(train, tu)
    labels = np.asarray(held.row_label)

    def rows_of(model):
        scores, _, metrics = nrms.compute_scores(model, held)
        return evaluate.impression_metrics(scores, held.row_impression, labels), metrics
    print(f"ranking demo: planted-signal corpus, {N - 1} news; NRMS at d = 64, random titles; {len(gains[0])} training impressions of up to "
          f"{gains[1].shape[1]} candidates; held-out: {int(held.history_ids.shape[0])} impressions", flush=True)
    def train_ndcg(model):
        """The mean nDCG@k of the TRAINING lists under the model's scores, in eval mode: ``list_pairwise``'s own second output."""
        model.eval()
        idx, ids, gain, count = nrms._check_lists(*gains[:3], gains[3], int(train.history_ids.shape[0]))
        total = 0.0
        with torch.no_grad():
            for lo in range(0, len(idx), 256):
                sl = slice(lo, lo + 256)
                user, table, pos, cnt, _ = nrms._list_front(model, train, idx[sl], ids[sl], count[sl])
                total += float(evaluate.list_pairwise(user, table, pos, cnt, torch.from_numpy(gain[sl]).to(dev),
                                                      discount=evaluate.ndcg_discount(ids.shape[1], k))[1].sum())
        return total / len(idx)
    print("  before: AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % rows_of(ranker)[1] + f"; training lists: nDCG@{k} {train_ndcg(ranker):.4f}", flush=True)
    t0 = time.perf_counter()
    l_rank = nrms.fit_ranker(ranker, train, gains, steps, batch_users=64, lr=1e-3, seed=0, k=k)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    l_soft = nrms.distil_retriever(softmax, train, clicks, steps, batch_users=64, lr=1e-3, seed=0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"  fit_ranker (k = {k}): {steps} steps of 64 lists, lr 1e-3: {1e3 * (t1 - t0) / steps:.1f} ms per step, loss {np.mean(l_rank[:10]):.4f} "
          f"(first ten steps) -> {np.mean(l_rank[-10:]):.4f} (last ten); distil_retriever on impression_lists: {1e3 * (t2 - t1) / steps:.1f} ms "
          f"per step, loss {np.mean(l_soft[:10]):.4f} -> {np.mean(l_soft[-10:]):.4f}", flush=True)
    (ra, ma), (rb, mb) = rows_of(ranker), rows_of(softmax)
    print("  after fit_ranker:        AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % ma + f"; training lists: nDCG@{k} {train_ndcg(ranker):.4f}", flush=True)
    print("  after the click softmax: AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % mb + f"; training lists: nDCG@{k} {train_ndcg(softmax):.4f}", flush=True)
    cmp_ = evaluate.compare_metrics(ra, rb, names=("AUC", "MRR", "nDCG@5", "nDCG@10"), replicates=replicates)
    for name in ("MRR", "nDCG@10"):
        f = cmp_[name]
        print(f"  {name}: fit_ranker - click softmax = {f['diff']:+.4f} [{f['lo']:+.4f}, {f['hi']:+.4f}], p = {f['p']:.4f}, wins {f['wins']:.3f} "
              f"({replicates} paired replicates over impressions)", flush=True)


def torch_mmr(ids, scores, count, vectors, k, lam, category=None, q=0):
    """Greedy maximal-marginal relevance built only from stock PyTorch: gather, ``torch.bmm``, then k rounds of element-wise ops and
    arg-max over all lists at once.  Every id is taken to lie in the table; NaN scores and the order among tied values are not the
    contract's (a yardstick for speed)."""
    G, M = ids.shape
    dev = ids.device
    rows = vectors[ids]
    sim = torch.bmm(rows, rows.transpose(1, 2))
    elem = torch.arange(M, device=dev)[None, :] < count[:, None]
    pen = torch.zeros((G, M), device=dev)
    chosen = torch.zeros((G, M), dtype=torch.bool, device=dev)
    same = torch.zeros((G, M), dtype=torch.int32, device=dev)
    cat = category[ids] if q else None
    out_i = torch.full((G, k), -1, dtype=torch.int64, device=dev)
    out_s = torch.full((G, k), float("-inf"), device=dev)
    cnt = torch.zeros(G, dtype=torch.int32, device=dev)
    ar = torch.arange(G, device=dev)
    neg = torch.full((), float("-inf"), device=dev)
    for t in range(k):
        ok = elem & ~chosen
        if q:
            ok &= same < q
        value = torch.where(ok, lam * scores - (1.0 - lam) * pen, neg)
        j = value.argmax(dim=1)
        live = ok[ar, j]
        out_i[:, t] = torch.where(live, ids[ar, j], out_i[:, t])
        out_s[:, t] = torch.where(live, scores[ar, j], out_s[:, t])
        chosen[ar, j] |= live
        pen = torch.maximum(pen, sim[ar, j])
        if q:
            same += ((cat == cat[ar, j][:, None]) & live[:, None]).to(torch.int32)
        cnt += live.to(torch.int32)
    return out_s, out_i, cnt


def bench_diversify(news_num=65238, d=400, rounds=5):
    """``evaluate.mmr_select`` against ``torch_mmr`` (what the tree had: gather + ``torch.bmm`` + k rounds of tiny launches), the two
    legs in turn in one process, median [min, max] of ``rounds`` rounds: G in {64, 4 096} lists of M = 128 ids of a table of
    ``news_num`` unit rows, k in {10, 100}, without and with a cap of 2 per category (17 categories).  Then ``util.recommend`` for
    64 users at k = 10 without and with ``diversity=0.3``, and ``mmr_select`` on lists of that shape, for the stage's share."""
    import time
    from digat_amd import evaluate, util
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    M = 128
    table = util.unit_rows(torch.randn(news_num, d, generator=g).to(dev))
    table[1::2] = table[0:news_num - 1:2][:table[1::2].shape[0]]   # every other row a copy of its neighbour: the penalty bites
    category = torch.randint(0, 17, (news_num,), generator=g, dtype=torch.int32).to(dev)
    print(f"diversify: lists of M = {M} ids of {news_num} unit rows, d = {d}; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        ids = torch.randint(0, news_num, (G, M), generator=g).to(dev)
        scores = torch.randn(G, M, generator=g).to(dev)
        count = torch.full((G,), M, dtype=torch.int32, device=dev)
        for k in (10, 100):
            for q in (0, 2):
                cat = category if q else None
                ours = lambda: evaluate.mmr_select(ids, scores, count, table, k, 0.7, category=cat, max_per_category=q)
                stock = lambda: torch_mmr(ids, scores, count, table, k, 0.7, category, q)
                got, want = ours(), stock()
                torch.cuda.synchronize()
                same = float((got[1] == want[1]).float().mean())     # bmm rounds otherwise than the fmaf chain: near-ties may swap
                (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=5)
                print(f"  G = {G:5d}, k = {k:3d}, cap {q}: mmr_select {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({2.0 * G * M * M * d / a / 1e9:6.2f} TFLOP/s "
                      f"of Gram) | gather + bmm + {k} torch rounds {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}) | ids equal: {same:.4f}",
                      flush=True)
        del ids, scores, count
    del table
    torch.cuda.empty_cache()
    users = 64
    spec, model, dc = _recommend_setup(users, news_num)
    pool = torch.arange(1, news_num, dtype=torch.int64, device=dev)
    who = np.arange(users)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    legs = {"plain k = 10": dict(), "plain k' = 40": dict(k=40), "diversity=0.3": dict(diversity=0.3),
            "diversity=0.3, 2 per category": dict(diversity=0.3, max_per_category=2)}
    for kw in legs.values():
        util.recommend(model, dc, who, pool, kw.pop("k", 10), **kw)  # the per-news tables, every path warm
    legs["plain k' = 40"]["k"] = 40
    torch.cuda.synchronize()
    secs = {name: [] for name in legs}
    for _ in range(rounds):
        for name, kw in legs.items():
            kw = dict(kw)
            t0 = time.perf_counter()
            util.recommend(model, dc, who, pool, kw.pop("k", 10), **kw)
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
    for name, v in secs.items():
        med, lo, hi = stat(v)
        print(f"  util.recommend, {users} users x {news_num - 1} news, {name}: {med:.3f} s [{lo:.3f}, {hi:.3f}]", flush=True)
    i, s, c = util.recommend(model, dc, who, pool, 40)
    unit = util.unit_rows(dc.news_embedding)
    sel, _ = timeit(lambda: evaluate.mmr_select(i, s, c, unit, 10, 0.7), iters=10)
    norm, _ = timeit(lambda: util.unit_rows(dc.news_embedding), iters=10)
    print(f"  of which mmr_select on the {users} lists of 40: {sel:.3f} ms, unit_rows of the {news_num} x {spec.embedding_dim} table: {norm:.3f} ms",
          flush=True)


def torch_calibrate(ids, scores, count, category, target, k, lam, alpha=0.01):
    """The calibrated re-rank built only from stock PyTorch — what the tree offered before ``digat_calibrated_select``: a gather of
    the categories, then k rounds of element-wise operations with ``torch.log`` in float64, a gather of the gains and arg-max over
    all lists at once.  Every id is taken to lie in the table and every category in [0, C); NaN scores and the order among tied
    values are not the contract's (a yardstick for speed)."""
    G, M = ids.shape
    dev = ids.device
    cat = category[ids].to(torch.int64)
    p = target.to(torch.float64)
    live = p > 0
    one = torch.ones((), dtype=torch.float64, device=dev)
    elem = torch.arange(M, device=dev)[None, :] < count[:, None]
    chosen = torch.zeros((G, M), dtype=torch.bool, device=dev)
    n = torch.zeros_like(p)
    out_i = torch.full((G, k), -1, dtype=torch.int64, device=dev)
    out_s = torch.full((G, k), float("-inf"), device=dev)
    cnt = torch.zeros(G, dtype=torch.int32, device=dev)
    ar = torch.arange(G, device=dev)
    neg = torch.full((), float("-inf"), device=dev)
    rel = lam * scores
    for t in range(k):
        q0 = torch.where(live, (1.0 - alpha) * n / (t + 1.0) + alpha * p, one)
        q1 = torch.where(live, (1.0 - alpha) * (n + 1.0) / (t + 1.0) + alpha * p, one)
        gain = ((1.0 - lam) * (p * (torch.log(q1) - torch.log(q0))).to(torch.float32))
        ok = elem & ~chosen
        value = torch.where(ok, rel + gain.gather(1, cat), neg)
        j = value.argmax(dim=1)
        hit = ok[ar, j]
        out_i[:, t] = torch.where(hit, ids[ar, j], out_i[:, t])
        out_s[:, t] = torch.where(hit, scores[ar, j], out_s[:, t])
        chosen[ar, j] |= hit
        n[ar, cat[ar, j]] += hit.to(torch.float64)
        cnt += hit.to(torch.int32)
    q = torch.where(live, (1.0 - alpha) * n / torch.clamp(cnt, min=1).to(torch.float64)[:, None] + alpha * p, one)
    kl = torch.where(live, p * (torch.log(torch.where(live, p, one)) - torch.log(q)), torch.zeros_like(p)).sum(dim=1).to(torch.float32)
    return out_s, out_i, cnt, kl


def bench_calibrate(rounds=5, demo=1):
    """``evaluate.calibrated_select`` against ``torch_calibrate``, the two legs in turn in one process, median [min, max] of
    ``rounds`` rounds and each leg's peak of device bytes beyond its inputs: G in {64, 4 096} lists of M in {128, 1 024} ids,
    k in {10, 100}, C = 17 categories, targets from a Dirichlet draw, lam = 0.5.  Then (``demo``) the effect on the planted-signal
    corpus (``demo_calibrate``)."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    news_num, C = 65238, 17
    category = torch.randint(0, C, (news_num,), generator=g, dtype=torch.int32).to(dev)
    conc = torch.distributions.Dirichlet(torch.full((C,), 0.7))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"calibrate: lists of ids of {news_num} news in C = {C} categories, lam = 0.5, alpha = 0.01; ms per call, median [min, max] of "
          f"{rounds} rounds", flush=True)
    for G in (64, 4096):
        torch.manual_seed(G)
        target = conc.sample((G,)).to(torch.float32).to(dev)
        for M in (128, 1024):
            ids = torch.randint(0, news_num, (G, M), generator=g).to(dev)
            scores = torch.randn(G, M, generator=g).sort(dim=1, descending=True).values.to(dev)      # a shortlist comes sorted
            count = torch.full((G,), M, dtype=torch.int32, device=dev)
            for k in (10, 100):
                ours = lambda: evaluate.calibrated_select(ids, scores, count, category, target, k, 0.5)
                stock = lambda: torch_calibrate(ids, scores, count, category, target, k, 0.5)
                (got, pa), (want, pb) = peak(ours), peak(stock)
                same = float((got[1] == want[1]).float().mean())         # torch.log is another logarithm: near-ties may swap
                dkl = float((got[3] - want[3]).abs().max())
                (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=5)
                print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}: calibrated_select {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({1e3 * a / k:.2f} us per step, "
                      f"peak {pa / 2**20:.2f} MiB) | gather + {k} torch rounds {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
                      f"{pb / 2**20:.1f} MiB) | ids equal: {same:.4f}, max |kl - kl| {dkl:.2e}", flush=True)
            del ids, scores, count
        del target
    torch.cuda.empty_cache()
    if demo:
        demo_calibrate()


def demo_calibrate(users=512, k=10, calibrations=(0.0, 0.3, 0.5, 0.8), replicates=2000):
    """What ``recommend(calibration=)`` does on the planted-signal corpus: the trained DIGAT (tests/golden/trained_planted_state.npz),
    ``users`` held-out impressions against the pool of all news, k = 10, one ``util.recommend`` per value of ``calibrations``.
    Reported per value, as means over the users with 95 % intervals (``evaluate.metric_intervals``, users resampled) and, against
    calibration 0, the paired difference (``evaluate.compare_metrics``): ``kl`` (``util.calibration_kl`` of the list against the
    history's category mix), ``category_max_share`` (``evaluate.list_quality``), recall@k of the impression's clicked candidates
    (summed hits over summed clicks) and MRR."""
    import types
    from digat_amd import evaluate, synthetic, util
    from digat_amd.main import clicked_targets
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    corpus = synthetic.slice_impressions(full, 0, users)
    spec = full.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    C = int(dc.news_category.max()) + 1
    target = evaluate.category_share(dc.history, dc.news_category, C)
    tg_ids, tg_start = clicked_targets(dc, corpus.row_label)
    names = ("kl", "category_max_share", f"recall@{k}", "mrr")

    def columns(f):
        ids, scores, count = util.recommend(model, dc, who, pool, k, calibration=f)
        kl = util.calibration_kl(ids, count, dc.news_category, target).cpu().numpy().astype(np.float64)
        q = evaluate.list_quality(ids, count, category=dc.news_category)
        el = q["elements"].cpu().numpy().astype(np.float64)
        share = q["category_max"].cpu().numpy().astype(np.float64) / np.maximum(el, 1.0)
        col = evaluate.rank_metric_columns(evaluate.list_ranks(ids, count, tg_ids, tg_start), tg_start, ks=(k,))
        ones = np.ones(users)
        spread = float(scores[:, 0].mean() - scores[:, k - 1].mean())
        return (np.stack([kl, share, col[f"hits@{k}"], col["rr"]], axis=1), np.stack([ones, ones, col["targets"], col["has"]], axis=1), spread)
    base = None
    print(f"calibration demo: planted-signal corpus, {spec.news_num - 1} news in {C} categories, the trained DIGAT, {users} held-out "
          f"impressions, k = {k}, shortlist min(1024, 8 k) = {min(1024, 8 * k)}; means with 95 % intervals from {replicates} replicates over "
          f"users; 'vs 0': paired difference to calibration 0", flush=True)
    for f in calibrations:
        values, den, spread = columns(f)
        iv = evaluate.metric_intervals(values, names=names, replicates=replicates, denominators=den)
        line = f"  calibration {f:.1f}: " + "  ".join(f"{name} {iv[name]['value']:.4f} [{iv[name]['lo']:.4f}, {iv[name]['hi']:.4f}]" for name in names)
        if base is None:
            base = (values, den)
            line += f"  (score of slot 1 minus slot {k}, mean: {spread:.3f})"
        else:
            cmp = evaluate.compare_metrics(values, base[0], names=names, replicates=replicates, denominators_a=den, denominators_b=base[1])
            line += " | vs 0: " + "  ".join(f"{name} {cmp[name]['diff']:+.4f} [{cmp[name]['lo']:+.4f}, {cmp[name]['hi']:+.4f}] p {cmp[name]['p']:.3f}"
                                            for name in names)
        print(line, flush=True)


def torch_topk_keys(x):
    """``evaluate.topk_keys`` in stock PyTorch, int64."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    nan = (b & 0x7fffffff) > 0x7f800000
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where(b >= 0x80000000, 0xffffffff - b, b | 0x80000000)
    return torch.where(nan, torch.ones_like(key), key)


def torch_capped(ids, scores, count, k, caps, P, max_rounds=1024):
    """Exposure-capped top-k built only from stock PyTorch — the rounds of ``evaluate.capped_select_host`` as they stand there: one
    stable argsort per list, one stable sort of the item words, then per round a cumsum over the lists, a gather into item order, a
    segmented cumsum, a scatter of the new rejections and one read of how many there were.  The same contract, bit for bit."""
    G, M = ids.shape
    dev = ids.device
    ks = torch_topk_keys(scores)
    elem = (torch.arange(M, device=dev)[None, :] < count.to(torch.int64).clamp(0, M)[:, None]) & (ids >= 0) & (ids < P) & (ks > 0x007fffff)
    order = torch.argsort(-torch.where(elem, ks, -torch.ones_like(ks)), dim=1, stable=True)
    words = torch.where(elem, (torch.where(elem, ids, torch.zeros_like(ids)) << 32) | (0xffffffff - ks),
                        torch.full_like(ids, 0x7fffffffffffffff)).view(-1)
    words, perm = torch.sort(words, stable=True)
    sid = words >> 32
    at = torch.arange(G * M, device=dev)
    start = torch.cummax(torch.where(torch.cat([sid[:1] == sid[:1], sid[1:] != sid[:-1]]), at, torch.zeros_like(at)), dim=0).values
    cap_of = caps.to(torch.int64)[sid.clamp(max=max(P - 1, 0))] if P else torch.zeros_like(sid)
    rejected = ~elem.view(-1)
    rounds = 0
    while True:
        if rounds == max_rounds:
            raise RuntimeError("torch_capped: no fixed point")
        rounds += 1
        alive = ~rejected.view(G, M).gather(1, order)
        ahead = alive.cumsum(dim=1)
        wanted = alive & (ahead <= k)
        demand = torch.zeros((G, M), dtype=torch.bool, device=dev).scatter_(1, order, wanted)
        d = demand.view(-1)[perm].to(torch.int64)
        before = d.cumsum(dim=0) - d
        before = before - before[start]
        gone = rejected[perm]
        new = (before >= cap_of) & ~gone
        if int(new.sum()) == 0:
            break
        rejected = rejected.scatter(0, perm, gone | new)
    out_i = torch.full((G * k,), -1, dtype=torch.int64, device=dev)
    out_s = torch.full((G * k,), float("-inf"), device=dev)
    out_p = torch.full((G * k,), -1, dtype=torch.int32, device=dev)
    to = (torch.arange(G, device=dev)[:, None] * k + ahead - 1)[wanted]
    out_i[to] = ids.gather(1, order)[wanted]
    out_s[to] = scores.gather(1, order)[wanted]
    out_p[to] = order[wanted].to(torch.int32)
    return out_i.view(G, k), out_s.view(G, k), wanted.sum(dim=1).to(torch.int32), out_p.view(G, k), rounds


def popular_lists(G, M, P, generator, dev, slab=256):
    """``(ids [G,M] int64, scores [G,M] float32)`` on ``dev``: per list M distinct news of P drawn with a strong popularity head
    (Gumbel top-M over ``-1.2 log(rank)``), scored by that popularity plus unit noise, on a grid of 1/64 — exact ties are met —, each
    list sorted by score as a shortlist comes."""
    weight = -1.2 * torch.log(torch.arange(1, P + 1, dtype=torch.float32, device=dev))
    ids, scores = [], []
    for g0 in range(0, G, slab):
        n = min(slab, G - g0)
        u = torch.rand((n, P), generator=generator).to(dev).clamp_(1e-9, 1 - 1e-9)
        pick = (weight[None, :] - torch.log(-torch.log(u))).topk(M, dim=1).indices
        s = torch.round((0.7 * weight[pick] + torch.randn((n, M), generator=generator).to(dev)) * 64) / 64
        s, o = s.sort(dim=1, descending=True, stable=True)
        ids.append(pick.gather(1, o))
        scores.append(s)
    return torch.cat(ids), torch.cat(scores)


def bench_exposure_cap(rounds=5, demo=1):
    """``evaluate.capped_select`` against ``torch_capped`` — the same rounds in stock PyTorch —, the two legs in turn in one process,
    median [min, max] of ``rounds`` rounds, each leg's peak of device bytes beyond its inputs and the rounds the call took: G in
    {64, 4 096} lists of M in {128, 1 024} of 65 237 news with a popularity head (``popular_lists``), k in {10, 100}, a cap of 1.2 x
    and 2 x the mean exposure G k / P (rounded up, at least 1).  Both legs read their counters back every block / round: the times
    are whole calls.  Then (``demo``) the effect on the planted-signal corpus (``demo_exposure_cap``)."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    P = 65237

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"exposure-cap: lists of distinct ids of {P} news with a popularity head; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            ids, scores = popular_lists(G, M, P, g, dev)
            count = torch.full((G,), M, dtype=torch.int32, device=dev)
            for k in (10, 100):
                for factor in (1.2, 2.0):
                    cap = max(1, int(np.ceil(factor * G * k / P)))
                    caps = torch.full((P,), cap, dtype=torch.int32, device=dev)
                    ours = lambda: evaluate.capped_select(ids, scores, count, k, caps, P)
                    stock = lambda: torch_capped(ids, scores, count, k, caps, P)
                    (got, pa), (want, pb) = peak(ours), peak(stock)
                    same = all(torch.equal(x, y) for x, y in zip(got[:4], want[:4])) and got[4] == want[4]
                    short = float((got[2] < k).float().mean())
                    top = int(torch.bincount(got[0][got[0] >= 0].view(-1), minlength=P).max())
                    (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=3)
                    print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, cap = {cap:3d} ({factor} x mean): capped_select {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] "
                          f"({got[4]} rounds, peak {pa / 2**20:.1f} MiB) | stock rounds {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
                          f"{pb / 2**20:.1f} MiB) | identical: {same} | largest exposure {top}, short lists {short:.3f}", flush=True)
            del ids, scores, count
    torch.cuda.empty_cache()
    if demo:
        demo_exposure_cap()


def demo_exposure_cap(users=512, k=10, caps=(16, 4, 2), shortlist=128, replicates=2000):
    """What ``recommend(exposure_cap=)`` does on the planted-signal corpus, in ``recommend_report``'s setting: the trained DIGAT
    (tests/golden/trained_planted_state.npz), ``users`` held-out impressions against the pool of all news in ONE call, k = 10, the
    plain call and one call per value of ``caps`` from a shortlist of ``shortlist``.  Per call: ``coverage`` and ``gini`` of the
    exposure over the pool (``evaluate.quality_summary``; figures of the whole batch: no interval), the largest exposure, the share
    of lists shorter than k, and recall@k of the impression's clicked candidates (summed hits over summed clicks) and MRR as means
    with 95 % intervals (``evaluate.metric_intervals``, users resampled) and, against the plain call, the paired difference
    (``evaluate.compare_metrics``)."""
    import types
    from digat_amd import evaluate, synthetic, util
    from digat_amd.main import clicked_targets
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    corpus = synthetic.slice_impressions(full, 0, users)
    spec = full.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    tg_ids, tg_start = clicked_targets(dc, corpus.row_label)
    names = (f"recall@{k}", "mrr")

    def columns(cap):
        kw = {} if cap is None else dict(exposure_cap=cap, shortlist=shortlist)
        ids, scores, count = util.recommend(model, dc, who, pool, k, **kw)
        exposure = torch.zeros((spec.news_num,), dtype=torch.int32, device=dev)
        q = evaluate.quality_summary(evaluate.list_quality(ids, count, exposure=exposure), exposure, pool)
        col = evaluate.rank_metric_columns(evaluate.list_ranks(ids, count, tg_ids, tg_start), tg_start, ks=(k,))
        batch = (q["coverage"], q["gini"], int(exposure.max()), float((count < k).float().mean()))
        return np.stack([col[f"hits@{k}"], col["rr"]], axis=1), np.stack([col["targets"], col["has"]], axis=1), batch
    print(f"exposure-cap demo: planted-signal corpus, {spec.news_num - 1} news, the trained DIGAT, {users} held-out impressions in one call, "
          f"k = {k} (mean exposure {users * k / (spec.news_num - 1):.2f}), shortlist {shortlist}; recall and MRR: means with 95 % intervals "
          f"from {replicates} replicates over users; 'vs plain': paired difference", flush=True)
    base = None
    for cap in (None,) + tuple(caps):
        values, den, (coverage, gini, top, short) = columns(cap)
        iv = evaluate.metric_intervals(values, names=names, replicates=replicates, denominators=den)
        line = (f"  {'plain' if cap is None else 'cap %3d' % cap}: coverage {coverage:.4f}  gini {gini:.4f}  largest exposure {top}  short lists "
                f"{short:.4f}  " + "  ".join(f"{name} {iv[name]['value']:.4f} [{iv[name]['lo']:.4f}, {iv[name]['hi']:.4f}]" for name in names))
        if base is None:
            base = (values, den)
        else:
            cmp = evaluate.compare_metrics(values, base[0], names=names, replicates=replicates, denominators_a=den, denominators_b=base[1])
            line += " | vs plain: " + "  ".join(f"{name} {cmp[name]['diff']:+.4f} [{cmp[name]['lo']:+.4f}, {cmp[name]['hi']:+.4f}] p {cmp[name]['p']:.3f}"
                                                for name in names)
        print(line, flush=True)


def torch_rerank(ids, scores, count, vectors, category, target, k, w, alpha=0.01, lazy=False, budget=1 << 30):
    """The joint re-rank built only from stock PyTorch, over chunks of lists that keep a leg's largest tensors within ``budget``
    bytes.  ``lazy`` False: gather + ``torch.bmm`` Gram [g, M, M], then k rounds of element-wise operations with ``torch.log`` in
    float64 and arg-max over the chunk's lists at once.  ``lazy`` True: the rows are gathered once per chunk and every step takes
    one batched matrix-vector product with the picked rows — no Gram.  Every id is taken to lie in the table and every category in
    [0, C); NaN scores and the order among tied values are not the contract's (a yardstick for speed)."""
    G, M = ids.shape
    d = int(vectors.shape[1])
    dev = ids.device
    wr, wd, wc = (float(x) for x in w)
    per_list = 4 * M * d + (0 if lazy else 4 * M * M) + 64 * M
    step = max(1, min(G, budget // per_list))
    outs = []
    one = torch.ones((), dtype=torch.float64, device=dev)
    neg = torch.full((), float("-inf"), device=dev)
    for g0 in range(0, G, step):
        I, S, cn = ids[g0:g0 + step], scores[g0:g0 + step], count[g0:g0 + step]
        g = int(I.shape[0])
        rows = vectors[I]
        sim = None if lazy or wd == 0 else torch.bmm(rows, rows.transpose(1, 2))
        elem = torch.arange(M, device=dev)[None, :] < cn[:, None]
        pen = torch.zeros((g, M), device=dev)
        chosen = torch.zeros((g, M), dtype=torch.bool, device=dev)
        ar = torch.arange(g, device=dev)
        out_i = torch.full((g, k), -1, dtype=torch.int64, device=dev)
        out_s = torch.full((g, k), float("-inf"), device=dev)
        cnt = torch.zeros(g, dtype=torch.int32, device=dev)
        rel = wr * S
        if wc != 0:
            cat = category[I].to(torch.int64)
            p = target[g0:g0 + step].to(torch.float64)
            live = p > 0
            n = torch.zeros_like(p)
        for t in range(k):
            ok = elem & ~chosen
            value = rel - wd * pen if wd != 0 else rel
            if wc != 0:
                q0 = torch.where(live, (1.0 - alpha) * n / (t + 1.0) + alpha * p, one)
                q1 = torch.where(live, (1.0 - alpha) * (n + 1.0) / (t + 1.0) + alpha * p, one)
                gain = wc * (p * (torch.log(q1) - torch.log(q0))).to(torch.float32)
                value = value + gain.gather(1, cat)
            j = torch.where(ok, value, neg).argmax(dim=1)
            hit = ok[ar, j]
            out_i[:, t] = torch.where(hit, I[ar, j], out_i[:, t])
            out_s[:, t] = torch.where(hit, S[ar, j], out_s[:, t])
            chosen[ar, j] |= hit
            if wd != 0 and t + 1 < k:
                row = torch.bmm(rows, rows[ar, j][:, :, None])[:, :, 0] if lazy else sim[ar, j]
                pen = torch.maximum(pen, row)
            if wc != 0:
                n[ar, cat[ar, j]] += hit.to(torch.float64)
            cnt += hit.to(torch.int32)
        outs.append((out_s, out_i, cnt))
    return tuple(torch.cat([o[x] for o in outs]) for x in range(3))


def bench_rerank(rounds=5, demo=1, d=400):
    """``evaluate.rerank_select`` against ``torch_rerank`` with a Gram (a) and lazy (b), the legs in turn in one process, median
    [min, max] of ``rounds`` rounds and each leg's peak of device bytes beyond its inputs: G in {64, 4 096} lists of M in {128,
    1 024} ids of unit rows, d = 400, k in {10, 100}, C = 17, weights (0.5, 0.3, 0.2) and — long MMR — (0.7, 0.3, 0); at M = 128
    without a calibration weight also ``evaluate.mmr_select``.  Then (``demo``) the effect on the planted-signal corpus
    (``demo_rerank``)."""
    from digat_amd import evaluate, util
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    news_num, C = 65238, 17
    table = util.unit_rows(torch.randn(news_num, d, generator=g).to(dev))
    table[1::2] = table[0:news_num - 1:2][:table[1::2].shape[0]]   # every other row a copy of its neighbour: the penalty bites
    category = torch.randint(0, C, (news_num,), generator=g, dtype=torch.int32).to(dev)
    conc = torch.distributions.Dirichlet(torch.full((C,), 0.7))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    print(f"rerank: lists of ids of {news_num} unit rows, d = {d}, C = {C} categories, alpha = 0.01; ms per call, median [min, max] of "
          f"{rounds} rounds; (a) gather + bmm Gram + k torch rounds, (b) rows gathered once + one batched matrix-vector product per step, "
          f"both chunked to 1 GiB", flush=True)
    for G in (64, 4096):
        torch.manual_seed(G)
        target = conc.sample((G,)).to(torch.float32).to(dev)
        for M in (128, 1024):
            ids = torch.randint(0, news_num, (G, M), generator=g).to(dev)
            scores = torch.randn(G, M, generator=g).sort(dim=1, descending=True).values.to(dev)      # a shortlist comes sorted
            count = torch.full((G,), M, dtype=torch.int32, device=dev)
            for k in (10, 100):
                for w in ((0.5, 0.3, 0.2), (0.7, 0.3, 0.0)):
                    w32 = tuple(np.float32(x) for x in w)
                    cal = w[2] != 0
                    legs = {"rerank_select": lambda: evaluate.rerank_select(ids, scores, count, table, k, *w32, category=category if cal else None,
                                                                            target=target if cal else None),
                            "(a)": lambda: torch_rerank(ids, scores, count, table, category, target, k, w32),
                            "(b)": lambda: torch_rerank(ids, scores, count, table, category, target, k, w32, lazy=True)}
                    if M == 128 and not cal:
                        legs["mmr_select"] = lambda: evaluate.mmr_select(ids, scores, count, table, k, w32[0])
                    outs = {name: peak(fn) for name, fn in legs.items()}
                    got = outs["rerank_select"][0]
                    same = {name: float((got[1] == o[0][1]).float().mean()) for name, o in outs.items() if name != "rerank_select"}
                    iters = 5 if G * M * k <= 64 * 1024 * 100 else 2
                    ms = {name: [] for name in legs}
                    for _ in range(rounds):
                        for name, fn in legs.items():
                            ms[name].append(timeit(fn, iters=iters, warm=1)[0])
                    a = stat(ms["rerank_select"])[0]
                    line = f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, w = {w}: "
                    line += " | ".join(f"{name} {stat(v)[0]:9.3f} ms [{stat(v)[1]:.3f}, {stat(v)[2]:.3f}]"
                                       + (f" (x{stat(v)[0] / a:.2f})" if name != "rerank_select" else f" ({1e3 * a / k:.1f} us per step)")
                                       + f" peak {outs[name][1] / 2**20:.1f} MiB" for name, v in ms.items())
                    line += " | ids equal: " + ", ".join(f"{name} {v:.4f}" for name, v in same.items())
                    print(line, flush=True)
            del ids, scores, count
        del target
    del table
    torch.cuda.empty_cache()
    if demo:
        demo_rerank()


def demo_rerank(users=512, k=10, shortlist=80, replicates=2000):
    """What ``recommend(rerank=)`` does on the planted-signal corpus beside the re-rankers of one kind: the trained DIGAT
    (tests/golden/trained_planted_state.npz), ``users`` held-out impressions against the pool of all news, k = 10, shortlist 80:
    plain, ``diversity=0.3``, ``calibration=0.5`` and ``rerank=(0.2, 0.4)``.  Reported per setting, as means over the users with
    95 % intervals (``evaluate.metric_intervals``) and, against plain, the paired difference (``evaluate.compare_metrics``): ``ild``
    (``evaluate.list_quality`` over unit rows), ``kl`` (``util.calibration_kl`` against the history's category mix), recall@k of the
    impression's clicked candidates (summed hits over summed clicks) and MRR."""
    import types
    from digat_amd import evaluate, synthetic, util
    from digat_amd.main import clicked_targets
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    corpus = synthetic.slice_impressions(full, 0, users)
    spec = full.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    C = int(dc.news_category.max()) + 1
    target = evaluate.category_share(dc.history, dc.news_category, C)
    unit = util.unit_rows(dc.news_embedding)
    tg_ids, tg_start = clicked_targets(dc, corpus.row_label)
    names = ("ild", "kl", f"recall@{k}", "mrr")
    settings = (("plain", dict()), ("diversity=0.3", dict(diversity=0.3, shortlist=shortlist)),
                ("calibration=0.5", dict(calibration=0.5, shortlist=shortlist)), ("rerank=(0.2, 0.4)", dict(rerank=(0.2, 0.4), shortlist=shortlist)))

    def columns(kw):
        ids, scores, count = util.recommend(model, dc, who, pool, k, **kw)
        kl = util.calibration_kl(ids, count, dc.news_category, target).cpu().numpy().astype(np.float64)
        q = evaluate.list_quality(ids, count, vectors=unit)
        el = q["elements"].cpu().numpy().astype(np.float64)
        two = (el > 1).astype(np.float64)                                 # quality_summary's ild: the mean over lists with a pair
        ild = two * (1.0 - q["sim_sum"].cpu().numpy() / np.maximum(el * (el - 1.0) / 2.0, 1.0))
        col = evaluate.rank_metric_columns(evaluate.list_ranks(ids, count, tg_ids, tg_start), tg_start, ks=(k,))
        ones = np.ones(users)
        return (np.stack([ild, kl, col[f"hits@{k}"], col["rr"]], axis=1), np.stack([two, ones, col["targets"], col["has"]], axis=1),
                evaluate.quality_summary(q))
    base = None
    print(f"rerank demo: planted-signal corpus, {spec.news_num - 1} news in {C} categories, the trained DIGAT, {users} held-out impressions, "
          f"k = {k}, shortlist {shortlist}; means with 95 % intervals from {replicates} replicates over users; 'vs plain': paired difference",
          flush=True)
    for name, kw in settings:
        values, den, summary = columns(kw)
        iv = evaluate.metric_intervals(values, names=names, replicates=replicates, denominators=den)
        line = f"  {name}: " + "  ".join(f"{m} {iv[m]['value']:.4f} [{iv[m]['lo']:.4f}, {iv[m]['hi']:.4f}]" for m in names)
        line += f"  (quality_summary ild {summary['ild']:.4f})"
        if base is None:
            base = (values, den)
        else:
            cmp = evaluate.compare_metrics(values, base[0], names=names, replicates=replicates, denominators_a=den, denominators_b=base[1])
            line += " | vs plain: " + "  ".join(f"{m} {cmp[m]['diff']:+.4f} [{cmp[m]['lo']:+.4f}, {cmp[m]['hi']:+.4f}] p {cmp[m]['p']:.3f}"
                                                for m in names)
        print(line, flush=True)


def stock_pl_sample(scores, count, k, temperature, samples, budget=1 << 30):
    """Plackett-Luce slates with their log-probabilities built only from stock PyTorch — what the tree offered before
    ``digat_pl_sample``: ``torch.rand`` -> two float64 logarithms -> add -> ``torch.topk`` -> gather -> the unpicked tail's
    ``logsumexp`` and a flipped ``logcumsumexp`` over the picks -> sum, over as many lists at a time as keep the [g, S, M] float64
    intermediates (noise, keys, the masked copy, topk's workspace) inside ``budget`` bytes.  Its draws are ``torch.rand``'s: not
    reproducible bit for bit across batch shapes, and not the contract's (a yardstick for speed and memory).  Every list is taken
    to hold at least k live entries."""
    G, M = scores.shape
    dev = scores.device
    a = scores.to(torch.float64) / temperature
    a = torch.where(torch.arange(M, device=dev)[None, :] < count[:, None], a, torch.full((), float("-inf"), dtype=torch.float64, device=dev))
    picks = torch.empty((G, samples, k), dtype=torch.int64, device=dev)
    logp = torch.empty((G, samples), dtype=torch.float64, device=dev)
    rows = max(1, budget // (samples * M * 8 * 4))
    for g0 in range(0, G, rows):
        ag = a[g0:g0 + rows, None, :].expand(-1, samples, -1)
        key = ag - torch.log(-torch.log(torch.rand(ag.shape, dtype=torch.float64, device=dev)))
        idx = key.topk(k, dim=2).indices
        mine = ag.gather(2, idx)
        tail = ag.scatter(2, idx, float("-inf")).logsumexp(dim=2, keepdim=True)
        lse = torch.cat([mine, tail], dim=2).flip(2).logcumsumexp(dim=2).flip(2)[:, :, :k]
        picks[g0:g0 + rows] = idx
        logp[g0:g0 + rows] = (mine - lse).sum(dim=2)
    return picks, logp


def bench_pl_sample(rounds=5, demo=0):
    """``evaluate.pl_sample`` against ``stock_pl_sample``, the two legs in turn in one process, median [min, max] of ``rounds``
    rounds and each leg's peak of device bytes beyond its inputs: (G, M, k, S) in {64, 4 096} x {128, 1 024} x {10, 100} x {1, 8},
    scores N(0, 1) sorted as a shortlist comes, T = 1.  The two legs draw different slates (another generator), so the check beside
    the times is statistical: the mean ``logp`` of either leg's slates."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"pl-sample: Plackett-Luce slates of k from lists of M scores, S samples per list, T = 1; ms per call, median [min, max] of "
          f"{rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            scores = torch.randn(G, M, generator=g).sort(dim=1, descending=True).values.to(dev)
            count = torch.full((G,), M, dtype=torch.int32, device=dev)
            for k in (10, 100):
                for S in (1, 8):
                    ours = lambda: evaluate.pl_sample(scores, count, k, 1.0, seed=1, samples=S)
                    stock = lambda: stock_pl_sample(scores, count, k, 1.0, S)
                    (got, pa), (want, pb) = peak(ours), peak(stock)
                    ma, mb = float(got[2].mean()), float(want[1].mean())
                    (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=5)
                    print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, S = {S}: pl_sample {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({1e3 * a / (G * S):.2f} us "
                          f"per slate, peak {pa / 2**20:.2f} MiB) | stock composition {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
                          f"{pb / 2**20:.1f} MiB) | mean logp {ma:.3f} vs {mb:.3f}", flush=True)
            del scores, count
    torch.cuda.empty_cache()
    if demo:
        demo_off_policy()


def demo_off_policy(users=2000, k=3, samples=4, truth_samples=64, replicates=2000):
    """Off-policy evaluation end to end on the planted-signal corpus.  The LOGGING policy: the trained DIGAT
    (tests/golden/trained_planted_state.npz), ``util.recommend_slates`` over ``users`` held-out impressions against the pool of all
    news — a shortlist of 8 k, ``samples`` slates of k per user at temperature T_log (the mean spread — standard deviation — of a
    user's shortlist scores, so that the policy is neither uniform nor the arg-max).  The TARGET policies: the same scores at other
    temperatures (T_log / 2, colder: nearer the plain list; 2 T_log, hotter).  Reward of a slate: its mean planted match
    (``synthetic.planted_reward``: 1 for a news of a preferred sub-topic, 1/2 for its category).  Per target: ``util.score_lists``
    on the logged shortlists, ``util.slate_log_prob`` of the logged slates, ``evaluate.off_policy_value`` (users kept together);
    beside it the target's TRUE value: ``truth_samples`` slates per user drawn from the target itself on the same shortlists."""
    import types
    from digat_amd import evaluate, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    pref, news_sub = synthetic.planted_match(full)
    corpus = synthetic.slice_impressions(full, 0, users)
    spec = full.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    reward = lambda slates: synthetic.planted_reward(pref[:users], news_sub, slates.cpu().numpy(), spec.subtopics_per_category)
    short = util.recommend(model, dc, who, pool, 8 * k)
    t_log = float(short[1].to(torch.float64).std(dim=1).mean())
    log = util.recommend_slates(model, dc, who, pool, k, t_log, samples=samples, seed=1)
    r_log = reward(log["slates"]).reshape(-1)
    plain = float(reward(short[0][:, None, :k]).mean())
    units = np.arange(0, users * samples + 1, samples)
    print(f"off-policy demo: planted-signal corpus, the trained DIGAT logs {samples} slates of k = {k} for each of {users} held-out "
          f"impressions from a shortlist of {8 * k} at T_log = {t_log:.4f}; reward = mean planted match of the slate; logged mean reward "
          f"{r_log.mean():.4f} (the plain top-{k}: {plain:.4f}); intervals: 95 %, {replicates} replicates over users", flush=True)
    for name, t_target in (("colder", t_log / 2), ("hotter", 2 * t_log)):
        scores = util.score_lists(model, dc, who, log["ids"], log["count"])
        lt, _, covered = util.slate_log_prob(log["ids"], scores, log["count"], log["slates"], t_target)
        out = evaluate.off_policy_value(r_log, lt.cpu().numpy().reshape(-1), log["logp"].cpu().numpy().reshape(-1), units=units,
                                        replicates=replicates)
        own = util.sample_lists(log["ids"], scores, log["count"], k, t_target, seed=2, samples=truth_samples, streams=torch.as_tensor(who))
        truth = float(reward(own[0]).mean())
        sn, ip = out["snips"], out["ips"]
        print(f"  target {name} (T = {t_target:.4f}): SNIPS {sn['value']:.4f} [{sn['lo']:.4f}, {sn['hi']:.4f}]  IPS {ip['value']:.4f} "
              f"[{ip['lo']:.4f}, {ip['hi']:.4f}]  truth (on-policy, {truth_samples} slates per user) {truth:.4f}  the SNIPS interval holds it: "
              f"{sn['lo'] <= truth <= sn['hi']}  ess / n {out['ess'] / out['n']:.3f}  max weight {out['max_weight']:.1f}  covered "
              f"{float(covered.float().mean()):.3f}", flush=True)


def stock_pl_expect(scores, count, picks, values, temperature, budget=1 << 30):
    """``evaluate.pl_expect``'s ``logp``, ``step_logp`` and ``step_mean`` built only from stock PyTorch in float64 — what the tree
    offered before ``digat_pl_expect``: a gather of the picks, the unpicked tail's ``logsumexp`` and a flipped ``logcumsumexp`` for
    ``log Z_t``; the same for the weighted sums in the linear domain — ``exp(a - a_max) v``, its gather, the tail's sum and a flipped
    ``cumsum`` — and one division; over as many lists at a time as keep the [g, S, M] float64 intermediates (the expanded scores
    and values, the masked copies, the weights and products) inside ``budget`` bytes.  Every slate is taken to be k live, distinct
    positions."""
    G, M = scores.shape
    S, k = int(picks.shape[1]), int(picks.shape[2])
    dev = scores.device
    a = scores.to(torch.float64) / temperature
    a = torch.where(torch.arange(M, device=dev)[None, :] < count[:, None], a, torch.full((), float("-inf"), dtype=torch.float64, device=dev))
    v = torch.where(torch.isfinite(values), values, torch.zeros_like(values)).to(torch.float64)
    logp = torch.empty((G, S), dtype=torch.float64, device=dev)
    step = torch.empty((G, S, k), dtype=torch.float64, device=dev)
    mean = torch.empty((G, S, k), dtype=torch.float64, device=dev)
    rows = max(1, budget // (S * M * 8 * 6))
    for g0 in range(0, G, rows):
        ag = a[g0:g0 + rows, None, :].expand(-1, S, -1)
        idx = picks[g0:g0 + rows].to(torch.int64)
        mine = ag.gather(2, idx)
        tail = ag.scatter(2, idx, float("-inf")).logsumexp(dim=2, keepdim=True)
        lse = torch.cat([mine, tail], dim=2).flip(2).logcumsumexp(dim=2).flip(2)[:, :, :k]
        top = a[g0:g0 + rows].amax(dim=1)[:, None, None]
        wv = torch.exp(ag - top) * v[g0:g0 + rows, None, :]
        num = torch.cat([wv.gather(2, idx), wv.scatter(2, idx, 0.0).sum(dim=2, keepdim=True)], dim=2).flip(2).cumsum(dim=2).flip(2)[:, :, :k]
        step[g0:g0 + rows] = mine - lse
        logp[g0:g0 + rows] = step[g0:g0 + rows].sum(dim=2)
        mean[g0:g0 + rows] = num / torch.exp(lse - top)
    return logp, step, mean


def bench_pl_expect(rounds=5):
    """``evaluate.pl_expect`` against ``stock_pl_expect``, the two legs in turn in one process, median [min, max] of ``rounds``
    rounds and each leg's peak of device bytes beyond its inputs: ``pl-sample``'s shapes, (G, M, k, S) in {64, 4 096} x {128, 1 024}
    x {10, 100} x {1, 8}, scores N(0, 1) sorted as a shortlist comes, values N(0, 1), T = 1, the slates ``pl_sample``'s own.  Beside
    the times: the largest difference of the two legs' ``step_mean``."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"pl-expect: logp, step_logp and the per-step expectation of a value for S logged slates of k per list of M, T = 1; ms per call, "
          f"median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            scores = torch.randn(G, M, generator=g).sort(dim=1, descending=True).values.to(dev)
            values = torch.randn(G, M, generator=g).to(dev)
            count = torch.full((G,), M, dtype=torch.int32, device=dev)
            for k in (10, 100):
                for S in (1, 8):
                    picks = evaluate.pl_sample(scores, count, k, 1.0, seed=1, samples=S)[0]
                    ours = lambda: evaluate.pl_expect(scores, count, picks, values, 1.0)
                    stock = lambda: stock_pl_expect(scores, count, picks, values, 1.0)
                    (got, pa), (want, pb) = peak(ours), peak(stock)
                    diff = float((got[2] - want[2]).abs().max())
                    (a, alo, ahi), (b, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=5)
                    print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, S = {S}: pl_expect {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] ({1e6 * a / (G * S):.1f} ns "
                          f"per slate, peak {pa / 2**20:.2f} MiB) | stock composition {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
                          f"{pb / 2**20:.1f} MiB) | max |step_mean difference| {diff:.2e}", flush=True)
                    del picks
            del scores, values, count
    torch.cuda.empty_cache()


def demo_off_policy_steps(users=2000, k=10, shortlist=80, samples=4, truth_samples=64, replicates=2000):
    """``demo_off_policy`` at a size the slate-level weight cannot carry — k = 10 from a shortlist of 80 — with a reward per POSITION
    (the planted match of the item at t: 1 for a preferred sub-topic, 1/2 for its category) and all four estimators side by side
    (``util.off_policy_report``): IPS and SNIPS on the slate's summed reward, PDIS, and DR with a deliberately imperfect value
    model — the category half alone: 1/2 for a news of a preferred sub-topic's category, sub-topic or not.  Beside them the target's
    TRUE value: the summed reward of ``truth_samples`` slates per user drawn from the target itself on the same shortlists."""
    import types
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    pref, news_sub = synthetic.planted_match(full)
    corpus = synthetic.slice_impressions(full, 0, users)
    spec = full.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    model = model.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    spc = spec.subtopics_per_category

    def item_reward(slates):                                            # [G, S, k] news ids -> the planted match of every item
        sl = slates.cpu().numpy()
        return synthetic.planted_reward(pref[:users], news_sub, sl.reshape(users, -1, 1), spc).reshape(sl.shape)
    short = util.recommend(model, dc, who, pool, shortlist)
    t_log = float(short[1].to(torch.float64).std(dim=1).mean())
    log = util.recommend_slates(model, dc, who, pool, k, t_log, samples=samples, seed=1, shortlist=shortlist)
    r_log = item_reward(log["slates"])
    ids = log["ids"].cpu().numpy()
    p = pref[:users][:, None, :]
    same_cat = ((news_sub[np.maximum(ids, 0)][..., None] // spc == p // spc) & (p >= 0)).any(axis=-1)
    values = torch.from_numpy(np.where(ids >= 0, 0.5 * same_cat, 0.0).astype(np.float32)).to(dev)
    units = np.arange(0, users * samples + 1, samples)
    print(f"off-policy-steps demo: planted-signal corpus, the trained DIGAT logs {samples} slates of k = {k} for each of {users} held-out "
          f"impressions from a shortlist of {shortlist} at T_log = {t_log:.4f}; reward = the summed planted match of the slate's items, "
          f"logged mean {r_log.sum(axis=2).mean():.4f}; value model: the category half alone; intervals: 95 %, {replicates} replicates over users",
          flush=True)
    scores = util.score_lists(model, dc, who, log["ids"], log["count"])
    for name, t_target in (("colder", t_log / 2), ("hotter", 2 * t_log)):
        rep = util.off_policy_report(log, scores, r_log, values=values, temperature=t_target, units=units, replicates=replicates)
        own = util.sample_lists(log["ids"], scores, log["count"], k, t_target, seed=2, samples=truth_samples, streams=torch.as_tensor(who))
        truth = float(item_reward(own[0]).sum(axis=2).mean())
        print(f"  target {name} (T = {t_target:.4f}): truth (on-policy, {truth_samples} slates per user) {truth:.4f}; slate weight: ess / n "
              f"{rep['ess'] / rep['n']:.4f}, max {rep['max_weight']:.1f}; per position ess / n {rep['step_ess'][0] / rep['n']:.3f} (t = 0) .. "
              f"{rep['step_ess'][-1] / rep['n']:.4f} (t = {k - 1}), max {rep['step_max_weight'].max():.1f}; dropped {rep['dropped']}", flush=True)
        for est in ("ips", "snips", "pdis", "dr"):
            f = rep[est]
            print(f"    {est.upper():5s} {f['value']:.4f} [{f['lo']:.4f}, {f['hi']:.4f}]  width {f['hi'] - f['lo']:.4f}  se {f['se']:.4f}  holds the truth: "
                  f"{f['lo'] <= truth <= f['hi']}", flush=True)


def stock_list_pl(users, rows, ids, count, picks, inv_t, backward=False, budget=1 << 30):
    """The summed ``logp`` of ``evaluate.list_pl`` from stock PyTorch under autograd in float32 — ``index_select`` + ``torch.bmm``, then
    ``evaluate._pl_stock``: a gather of the picks, ``logsumexp`` of the unpicked tail, a flipped ``logcumsumexp`` — the lists in chunks
    whose [g, M, d] gather and [g, S, M] intermediates (the expanded scores, the mask, the masked copy) hold ``budget`` bytes.
    ``backward``: every chunk is differentiated as soon as it stands.  Every id is a row in the benchmark's data."""
    from digat_amd import evaluate
    G, M = ids.shape
    S, d = int(picks.shape[1]), int(users.shape[1])
    step = max(1, budget // (4 * (M * d + 4 * S * M)))
    slot = torch.arange(M, device=ids.device)
    total = torch.zeros((), dtype=torch.float32, device=ids.device)
    for lo in range(0, G, step):
        sl = slice(lo, lo + step)
        g = ids[sl].shape[0]
        x = torch.bmm(rows.index_select(0, ids[sl].reshape(-1)).view(g, M, -1), users[sl].unsqueeze(2)).squeeze(2)
        logp = evaluate._pl_stock(x, slot[None, :] < count[sl][:, None], picks[sl], inv_t)[0].sum()
        if backward:
            logp.backward()
        total = total + logp.detach()
    return total


def bench_list_pl(d=400, rounds=5, demo=0):
    """``evaluate.list_pl`` (the fused Plackett-Luce slate likelihood and its gradients: no [G, M, d] gather, no [G, S, M] tensor, no
    float atomics) against ``stock_list_pl`` (float32, chunked to 1 GiB) under autograd, in one process, the legs taken in turn,
    median [min, max] of ``rounds`` rounds of three calls, and each leg's peak of device bytes beyond its inputs; forward alone
    (``no_grad``) and forward + backward; (G, M, k, S) in {64, 4 096} x {128, 1 024} x {10, 100} x {1, 8}, a compact pool.  Then
    (``demo``) ``demo_policy``."""
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        out = float(out)
        return out, torch.cuda.max_memory_allocated() - base
    print(f"list-pl: d = {d}, compact pool, scale = 1, T = 1; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            P = max(M, min(65237, G * M // 4))
            rows = (torch.randn(P, d, generator=g) / d ** 0.5).to(dev)
            users = (3.0 * torch.randn(G, d, generator=g)).to(dev)
            ids = torch.stack([torch.randperm(P, generator=g)[:M] for _ in range(G)]).to(dev)
            count = torch.randint(M * 3 // 4, M + 1, (G,), generator=g).to(torch.int32).to(dev)
            for k in (10, 100):
                for S in (1, 8):
                    noise = torch.rand(G, S, M, generator=g).to(dev)
                    noise = noise.masked_fill(torch.arange(M, device=dev)[None, None, :] >= count[:, None, None], 2.0)
                    order = noise.argsort(dim=2)[:, :, :k]
                    picks = torch.where(order < count[:, None, None], order, torch.full_like(order, -1)).to(torch.int32).contiguous()
                    del noise, order

                    def fused_fwd():
                        with torch.no_grad():
                            return evaluate.list_pl(users, rows, ids, count, picks)[0].sum()

                    def stock_fwd():
                        with torch.no_grad():
                            return stock_list_pl(users, rows, ids, count, picks, 1.0)

                    def fused_both():
                        u, t = users.detach().requires_grad_(True), rows.detach().requires_grad_(True)
                        logp = evaluate.list_pl(u, t, ids, count, picks)[0].sum()
                        logp.backward()
                        return logp.detach() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])

                    def stock_both():
                        u, t = users.detach().requires_grad_(True), rows.detach().requires_grad_(True)
                        logp = stock_list_pl(u, t, ids, count, picks, 1.0, backward=True)
                        return logp + 0.0 * (u.grad[0, 0] + t.grad[0, 0])
                    legs = (fused_fwd, stock_fwd, fused_both, stock_both)
                    peaks = [peak(fn) for fn in legs]
                    times = [[] for _ in legs]
                    for _ in range(rounds):
                        for leg, fn in zip(times, legs):
                            leg.append(timeit(fn, iters=3, warm=1)[0])
                    (a, alo, ahi), (b, blo, bhi), (c, clo, chi), (e, elo, ehi) = (stat(t) for t in times)
                    print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, S = {S}: forward: list_pl {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] (peak "
                          f"{peaks[0][1] / 2**20:.2f} MiB) | stock {b:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak {peaks[1][1] / 2**20:.1f} MiB) "
                          f"|| forward + backward: list_pl {c:8.3f} ms [{clo:.3f}, {chi:.3f}] (peak {peaks[2][1] / 2**20:.1f} MiB) | stock {e:8.3f} ms "
                          f"[{elo:.3f}, {ehi:.3f}] (x{e / c:.2f}, peak {peaks[3][1] / 2**20:.1f} MiB) | summed logp {peaks[0][0]:.1f} vs stock "
                          f"{peaks[1][0]:.1f}", flush=True)
                    del picks
            del rows, users, ids, count
            torch.cuda.empty_cache()
    if demo:
        demo_policy()


def _ideal_weight(gain, k):
    """``1 / IDCG@k`` per list (0 where that is 0), float64 numpy [G], from a gain tensor [G, M]."""
    from digat_amd import evaluate
    g = gain.detach().cpu().numpy().astype(np.float64)
    g = np.where(np.isfinite(g) & (g > 0), g, 0.0)
    top = -np.sort(-g, axis=1)[:, :k]
    idcg = (top * evaluate.ndcg_discount(k)[:top.shape[1]]).sum(axis=1)
    return np.where(idcg > 0, 1.0 / np.where(idcg > 0, idcg, 1.0), 0.0)


def _loo(r):
    """Leave-one-out weights of rewards [G, S]: the reward minus the mean of the list's other samples (the reward itself at S = 1)."""
    S = int(r.shape[1])
    return r if S == 1 else r - (r.sum(dim=1, keepdim=True) - r) / (S - 1)


def stock_reinforce(users, rows, ids, count, gain, lw, k, S, backward=False, budget=1 << 30):
    """A sampled-slate policy-gradient step from stock PyTorch in float32: ``index_select`` + ``torch.bmm`` scores, Gumbel keys from
    ``torch.rand`` and ``topk`` for the slates, a gather of the gains for the nDCG@k of every slate, leave-one-out weights, and
    ``evaluate._pl_stock`` for the likelihood under autograd — the lists in chunks of ``budget`` bytes of intermediates, as
    ``stock_list_pl``.  Returns the summed reward."""
    from digat_amd import evaluate
    G, M = ids.shape
    d = int(users.shape[1])
    step = max(1, budget // (4 * (M * d + 6 * S * M)))
    slot = torch.arange(M, device=ids.device)
    disc = torch.from_numpy(evaluate.ndcg_discount(k)).to(ids.device).float()
    total = torch.zeros((), dtype=torch.float32, device=ids.device)
    for lo in range(0, G, step):
        sl = slice(lo, lo + step)
        g = ids[sl].shape[0]
        x = torch.bmm(rows.index_select(0, ids[sl].reshape(-1)).view(g, M, -1), users[sl].unsqueeze(2)).squeeze(2)
        live = slot[None, :] < count[sl][:, None]
        with torch.no_grad():
            key = x.detach()[:, None, :] - torch.log(-torch.log(torch.rand((g, S, M), device=x.device).clamp_(1e-20, 1.0 - 1e-7)))
            top = key.masked_fill(~live[:, None, :], float("-inf")).topk(min(k, M), dim=2)
            picks = torch.where(torch.isfinite(top.values), top.indices, torch.full_like(top.indices, -1))
            got = torch.where(picks >= 0, gain[sl].gather(1, picks.clamp(min=0).view(g, -1)).view(picks.shape), torch.zeros((), device=x.device))
            r = (got * disc[:picks.shape[2]]).sum(dim=2) * lw[sl][:, None]
            w = _loo(r)
        if backward:
            (-(w * evaluate._pl_stock(x, live, picks, 1.0)[0]).sum() / (g * S)).backward()
        total = total + r.sum()
    return total


def bench_plrank(d=400, rounds=5):
    """``evaluate.list_plrank`` (one pass: score, draw, value; the PL-Rank coefficient kernel behind it) against (1) what the tree had
    for a sampled-slate policy-gradient step — ``list_softmax``'s forward for the scores, ``pl_sample``, the slates' nDCG@k by a gather
    of the positions (no ``slate_positions``), leave-one-out weights, ``list_pl`` forward and backward — and (2) ``stock_reinforce``
    (float32, chunked to 1 GiB), in one process, the legs taken in turn, median [min, max] of ``rounds`` rounds of three calls; forward
    alone (``no_grad``) and forward + backward; ``list-pl``'s sixteen shapes, click-like gains (three positive per list)."""
    from digat_amd import evaluate, nrms
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))
    print(f"plrank: d = {d}, compact pool, scale = 1, T = 1, nDCG@k; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for M in (128, 1024):
            P = max(M, min(65237, G * M // 4))
            rows = (torch.randn(P, d, generator=g) / d ** 0.5).to(dev)
            users = (3.0 * torch.randn(G, d, generator=g)).to(dev)
            ids = torch.stack([torch.randperm(P, generator=g)[:M] for _ in range(G)]).to(dev)
            count = torch.randint(M * 3 // 4, M + 1, (G,), generator=g).to(torch.int32).to(dev)
            gain = torch.zeros(G, M)
            gain.scatter_(1, torch.stack([torch.randperm(M * 3 // 4, generator=g)[:3] for _ in range(G)]), 1.0)
            gain = gain.to(dev)
            zero = torch.zeros((G, M), device=dev)
            for k in (10, 100):
                lw = _ideal_weight(gain, k)
                lw_t = torch.from_numpy(lw).to(dev)
                for S in (1, 8):
                    def fused(backward):
                        u, t = users.detach().requires_grad_(backward), rows.detach().requires_grad_(backward)
                        value = evaluate.list_plrank(u, t, ids, count, gain, k, S, None, lw, seed=1)[0]
                        if not backward:
                            return value.sum()
                        (-value.sum() / G).backward()
                        return value.detach().sum() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])

                    def parent(backward):
                        with torch.no_grad():
                            scores = evaluate.list_softmax(users, rows, ids, count, zero)[2]
                            picks = evaluate.pl_sample(scores, count, k, 1.0, 1, S)[0]
                            w = _loo(nrms.slate_ndcg(gain, picks, k))
                        u, t = users.detach().requires_grad_(backward), rows.detach().requires_grad_(backward)
                        logp = evaluate.list_pl(u, t, ids, count, picks)[0]
                        if not backward:
                            return logp.sum()
                        (-(w * logp).sum() / (G * S)).backward()
                        return logp.detach().sum() + 0.0 * (u.grad[0, 0] + t.grad[0, 0])

                    def stock(backward):
                        u, t = users.detach().requires_grad_(backward), rows.detach().requires_grad_(backward)
                        if not backward:
                            with torch.no_grad():
                                return stock_reinforce(u, t, ids, count, gain, lw_t.float(), k, S)
                        r = stock_reinforce(u, t, ids, count, gain, lw_t.float(), k, S, backward=True)
                        return r + 0.0 * (u.grad[0, 0] + t.grad[0, 0])
                    legs = [lambda f=f, b=b: f(b) for b in (False, True) for f in (fused, parent, stock)]
                    times = [[] for _ in legs]
                    for _ in range(rounds):
                        for leg, fn in zip(times, legs):
                            leg.append(timeit(fn, iters=3, warm=1)[0])
                    st = [stat(t) for t in times]
                    cell = lambda i: f"{st[i][0]:8.3f} ms [{st[i][1]:.3f}, {st[i][2]:.3f}]"
                    print(f"  G = {G:5d}, M = {M:4d}, k = {k:3d}, S = {S}: forward: list_plrank {cell(0)} | softmax + sample + list_pl {cell(1)} "
                          f"(x{st[1][0] / st[0][0]:.2f}) | stock {cell(2)} (x{st[2][0] / st[0][0]:.2f}) || forward + backward: list_plrank {cell(3)} | "
                          f"softmax + sample + list_pl {cell(4)} (x{st[4][0] / st[3][0]:.2f}) | stock {cell(5)} (x{st[5][0] / st[3][0]:.2f})", flush=True)
            del rows, users, ids, count, gain, zero
            torch.cuda.empty_cache()


def gradient_variance(model, train, lists, k=10, samples=4, draws=64, batch=64):
    """The variance of one step's ``d_users`` under both estimators of the gradient of minus the mean expected nDCG@k of a batch: the
    model in eval mode, the first ``batch`` lists, ``draws`` values of ``first_sample`` (``samples`` apart), the encoders run once.
    PL-Rank: ``list_plrank``'s backward.  REINFORCE: ``pl_sample`` on the same scores, ``slate_ndcg``, leave-one-out weights, ``list_pl``'s
    backward, divided by the valid lists times ``samples`` so that both estimate the same gradient (``policy_step`` divides by the number
    of slates with a non-zero weight instead: another scale, not another direction).  Returns per estimator ``(total variance summed over the coordinates, squared norm of the mean)`` and the
    distance between the two means."""
    from digat_amd import evaluate, nrms
    users, ids, gain, count = nrms._check_lists(*lists[:3], lists[3], int(train.history_ids.shape[0]))
    b = np.arange(min(batch, len(users)))
    model.eval()
    with torch.no_grad():
        user, table, pos, cnt, _ = nrms._list_front(model, train, users[b], ids[b], count[b])
    dev = user.device
    gn = torch.from_numpy(gain[b]).to(dev)
    lw = _ideal_weight(gn, k)
    valid = max(int((lw > 0).sum()), 1)
    streams = torch.from_numpy(users[b]).to(dev)
    got ={"plrank": [], "reinforce": []}
    for f in range(draws):
        u = user.detach().requires_grad_(True)
        value, _, _, scores = evaluate.list_plrank(u, table, pos, cnt, gn, k, samples, None, lw, seed=0, first_sample=f * samples, streams=streams)
        (-value.sum() / valid).backward()
        got["plrank"].append(u.grad.double().cpu().numpy().copy())
        picks = evaluate.pl_sample(scores, cnt, k, 1.0, 0, samples, f * samples, streams)[0]
        w = _loo(nrms.slate_ndcg(gn, picks, k))
        u = user.detach().requires_grad_(True)
        logp = evaluate.list_pl(u, table, pos, cnt, picks)[0]
        (-(w * logp).sum() / (valid * samples)).backward()
        got["reinforce"].append(u.grad.double().cpu().numpy().copy())
    out = {}
    for name, v in got.items():
        v = np.stack(v)
        out[name] = (float(v.var(axis=0, ddof=1).sum()), float((v.mean(axis=0) ** 2).sum()))
    out["distance"] = float(np.sqrt(((np.stack(got["plrank"]).mean(axis=0) - np.stack(got["reinforce"]).mean(axis=0)) ** 2).sum()))
    return out


def demo_policy(train_users=2048, steps=300, k=10, samples=4, log_users=2000, replicates=2000, logs=1):
    """The demonstration runs of the policy-gradient surface on the planted-signal corpus, in ``demo_rank``'s setting (NRMS at d = 64,
    random titles, ``train_users`` training impressions, ``steps`` steps of 64 lists, lr 1e-3, the same seeded draws).  (1) Three copies
    of one model: ``nrms.fit_policy`` (REINFORCE on the expected nDCG@``k`` of ``samples`` sampled slates), ``nrms.fit_ranker`` and the
    listwise click softmax; held-out AUC / MRR / nDCG with ``evaluate.compare_metrics``; then a fourth copy under
    ``fit_policy(estimator="plrank")`` — its step time beside REINFORCE's from the same run (both warmed by three untimed steps on
    further copies), the nDCG@``k`` of the steps' own slates, its held-out metrics paired against the REINFORCE leg — and
    ``gradient_variance`` of both estimators on the untrained model.  ``logs`` = 0 stops here.  (2) ``nrms.fit_from_logs``: the trained DIGAT
    logs slates for ``log_users`` held-out impressions (``demo_off_policy``'s log and reward); a fresh NRMS is trained on the log; it
    is judged by the mean reward of its OWN slates on the logged shortlists before and after, and by ``evaluate.off_policy_value`` of
    its likelihoods on the log.  Beside it: what the graph-free first scoring pass of a ``fit_from_logs`` step costs."""
    import copy
    import time
    import types
    from digat_amd import evaluate, nrms, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    dev = torch.device("cuda:0")
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    spec = full.spec
    N, H, Lw, V = spec.news_num, spec.max_history_num, 16, 4000
    text, mask = synthetic.make_titles(N, Lw, V, seed=2)

    def part(lo, hi):
        c = synthetic.slice_impressions(full, lo, hi)
        hist = torch.from_numpy(c.history.astype(np.int64)).to(dev)
        return types.SimpleNamespace(title_text=torch.from_numpy(text).to(dev), title_mask=torch.from_numpy(mask).to(dev),
                                     augmented_title_text=None, augmented_title_mask=None, history_ids=hist, history_mask=hist != 0,
                                     row_candidate=c.row_candidate.astype(np.int64), row_impression=c.row_impression, row_label=c.row_label)
    held, train = part(0, synthetic.PLANTED_DEV_IMPRESSIONS), part(synthetic.PLANTED_DEV_IMPRESSIONS, spec.impressions)
    base = _nrms_model("NRMS", V=V, dm=64, h=8, dk=8, att=32, Lw=Lw, H=H, dropout=0.2)
    policy, ranker, softmax, student, plrank, fixed, *warm = (copy.deepcopy(base) for _ in range(8))      # before base runs: its caches do not copy
    tu = np.arange(train_users, dtype=np.int64)
    gains, clicks = nrms.impression_gain_lists(train, tu), nrms.impression_lists(train, tu)
    labels = np.asarray(held.row_label)

    def rows_of(model):
        scores, _, metrics = nrms.compute_scores(model, held)
        return evaluate.impression_metrics(scores, held.row_impression, labels), metrics
    print(f"policy demo (1): planted-signal corpus, NRMS at d = 64, random titles; {len(gains[0])} training impressions of up to "
          f"{gains[1].shape[1]} candidates; held-out: {int(held.history_ids.shape[0])} impressions", flush=True)
    print("  before: AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % rows_of(base)[1], flush=True)
    for est, copy_ in zip(("reinforce", "plrank"), warm):              # three steps of either on a copy: the timed legs start warm
        nrms.fit_policy(copy_, train, gains, 3, k=k, samples=samples, batch_users=64, lr=1e-3, seed=0, estimator=est)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    l_pol, r_pol = nrms.fit_policy(policy, train, gains, steps, k=k, samples=samples, batch_users=64, lr=1e-3, seed=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    l_rank = nrms.fit_ranker(ranker, train, gains, steps, batch_users=64, lr=1e-3, seed=0, k=k)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    nrms.distil_retriever(softmax, train, clicks, steps, batch_users=64, lr=1e-3, seed=0)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"  fit_policy (k = {k}, {samples} samples): {1e3 * (t1 - t0) / steps:.1f} ms per step, mean reward (nDCG@{k} of a sampled slate) "
          f"{np.mean(r_pol[:10]):.4f} (first ten steps) -> {np.mean(r_pol[-10:]):.4f} (last ten); fit_ranker {1e3 * (t2 - t1) / steps:.1f} ms per "
          f"step; the click softmax {1e3 * (t3 - t2) / steps:.1f} ms per step", flush=True)
    (rp, mp), (rr, mr), (rs, ms) = rows_of(policy), rows_of(ranker), rows_of(softmax)
    for name, m in (("fit_policy", mp), ("fit_ranker", mr), ("the click softmax", ms)):
        print(f"  after {name}: " + "AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % m, flush=True)
    for other, rows in (("fit_ranker", rr), ("click softmax", rs)):
        cmp_ = evaluate.compare_metrics(rp, rows, names=("AUC", "MRR", "nDCG@5", "nDCG@10"), replicates=replicates)
        for name in ("MRR", "nDCG@10"):
            f = cmp_[name]
            print(f"  {name}: fit_policy - {other} = {f['diff']:+.4f} [{f['lo']:+.4f}, {f['hi']:+.4f}], p = {f['p']:.4f} ({replicates} paired "
                  f"replicates over impressions)", flush=True)
    # the third leg: the same trainer with the PL-Rank estimator, one scoring pass a step
    torch.cuda.synchronize()
    ta = time.perf_counter()
    l_plr, r_plr = nrms.fit_policy(plrank, train, gains, steps, k=k, samples=samples, batch_users=64, lr=1e-3, seed=0, estimator="plrank")
    torch.cuda.synchronize()
    tb = time.perf_counter()
    rq, mq = rows_of(plrank)
    print(f"  fit_policy(estimator='plrank') (k = {k}, {samples} samples): {1e3 * (tb - ta) / steps:.1f} ms per step against REINFORCE's "
          f"{1e3 * (t1 - t0) / steps:.1f} in this run; mean nDCG@{k} of the step's own sampled slates {np.mean(r_plr[:10]):.4f} (first ten steps) "
          f"-> {np.mean(r_plr[-10:]):.4f} (last ten) against REINFORCE's {np.mean(r_pol[:10]):.4f} -> {np.mean(r_pol[-10:]):.4f}", flush=True)
    print("  after fit_policy(estimator='plrank'): AUC %.4f MRR %.4f nDCG@5 %.4f nDCG@10 %.4f" % mq, flush=True)
    cmp_ = evaluate.compare_metrics(rq, rp, names=("AUC", "MRR", "nDCG@5", "nDCG@10"), replicates=replicates)
    for name in ("MRR", "nDCG@10"):
        f = cmp_[name]
        print(f"  {name}: plrank - REINFORCE = {f['diff']:+.4f} [{f['lo']:+.4f}, {f['hi']:+.4f}], p = {f['p']:.4f} ({replicates} paired replicates "
              f"over impressions)", flush=True)
    gvar = gradient_variance(fixed, train, gains, k=k, samples=samples)
    print(f"  gradient variance (the untrained model in eval mode, the first 64 lists, 64 values of first_sample, {samples} samples; d_users, summed "
          f"over coordinates): PL-Rank {gvar['plrank'][0]:.4e} (|mean|^2 {gvar['plrank'][1]:.4e}) | REINFORCE with leave-one-out "
          f"{gvar['reinforce'][0]:.4e} (|mean|^2 {gvar['reinforce'][1]:.4e}) | ratio {gvar['plrank'][0] / gvar['reinforce'][0]:.3f}; the two means "
          f"lie {gvar['distance']:.3e} apart", flush=True)
    if not logs:
        return
    # (2) learning from a log the trained DIGAT makes
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    state = {name: v for name, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    depth = int(np.load(os.path.join(golden, "devset_trained_2k.npz"))["depth"])
    pref, news_sub = synthetic.planted_match(full)
    corpus = synthetic.slice_impressions(full, 0, log_users)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth, dropout_rate=0.2)
    teacher = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    teacher.graph_encoder.load_state_dict({name: torch.from_numpy(v) for name, v in state.items()})
    teacher = teacher.to(dev).eval()
    dc = util.DeviceCorpus.from_numpy(corpus, dev)
    who = np.arange(log_users, dtype=np.int64)
    pool = np.arange(1, spec.news_num, dtype=np.int64)
    reward = lambda slates: synthetic.planted_reward(pref[:log_users], news_sub, slates.cpu().numpy(), spec.subtopics_per_category)
    kk = 3
    short = util.recommend(teacher, dc, who, pool, 8 * kk)
    t_log = float(short[1].to(torch.float64).std(dim=1).mean())
    log = util.recommend_slates(teacher, dc, who, pool, kk, t_log, samples=samples, seed=1)
    r_log = reward(log["slates"])
    logged = part(0, log_users)
    ids_h, cnt_h = log["ids"].cpu().numpy().astype(np.int64), log["count"].cpu().numpy().astype(np.int64)

    def judge(model):
        """The student's own slates on the logged shortlists (eval mode, T = 1) and the clipped off-policy value of its likelihoods."""
        model.eval()
        own, lt = [], []
        with torch.no_grad():
            for lo in range(0, log_users, 256):
                sl = slice(lo, lo + 256)
                scores, cnt = nrms._list_scores(model, logged, who[sl], ids_h[sl], cnt_h[sl])
                own.append(util.sample_lists(log["ids"][sl], scores, cnt, kk, 1.0, seed=2, samples=16, streams=torch.as_tensor(who[sl]))[0])
                lt.append(nrms.policy_step(model, logged, who[sl], ids_h[sl], log["slates"][sl], np.zeros((len(who[sl]), samples)), cnt_h[sl])[1])
        value = evaluate.off_policy_value(r_log.reshape(-1), torch.cat(lt).cpu().numpy().reshape(-1), log["logp"].cpu().numpy().reshape(-1),
                                          clip=10.0, units=np.arange(0, log_users * samples + 1, samples), replicates=replicates)
        return float(reward(torch.cat(own)).mean()), value
    print(f"policy demo (2): the trained DIGAT logs {samples} slates of k = {kk} for each of {log_users} held-out impressions from a shortlist of "
          f"{8 * kk} at T_log = {t_log:.4f}; reward = mean planted match; logged mean reward {r_log.mean():.4f}; the student: a fresh NRMS at "
          f"d = 64 with random titles, policy softmax(<user, news>) over the logged shortlist", flush=True)
    before = judge(student)
    t0 = time.perf_counter()
    l_log = nrms.fit_from_logs(student, logged, log, r_log, steps, clip=10.0, users=who, batch_users=64, lr=1e-3, seed=0, temperature=1.0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    after = judge(student)
    for tag, (own, v) in (("before", before), ("after fit_from_logs", after)):
        sn, ip = v["snips"], v["ips"]
        print(f"  {tag}: mean reward of the student's own slates (16 per user) {own:.4f}; on the log, clip 10: IPS {ip['value']:.4f} "
              f"[{ip['lo']:.4f}, {ip['hi']:.4f}] SNIPS {sn['value']:.4f} [{sn['lo']:.4f}, {sn['hi']:.4f}] ess / n {v['ess'] / v['n']:.3f}", flush=True)
    student.train()
    b = np.arange(64)
    zero = np.zeros((64, samples))

    def first_pass():
        with torch.no_grad():
            return nrms.policy_step(student, logged, who[b], ids_h[b], log["slates"][b], zero, cnt_h[b])[0]
    ms_first = timeit(first_pass, iters=10, warm=2)[0]
    print(f"  fit_from_logs: {1e3 * (t1 - t0) / steps:.1f} ms per step of 64 lists, loss {np.mean(l_log[:10]):.4f} -> {np.mean(l_log[-10:]):.4f}; its "
          f"graph-free first scoring pass alone: {ms_first:.1f} ms, {100 * ms_first / (1e3 * (t1 - t0) / steps):.0f} % of a step", flush=True)


def torch_list_quality(ids, count, vectors, category=None, base_ids=None, base_count=None, exposure=None):
    """``evaluate.list_quality``'s figures built only from stock PyTorch: gather + ``torch.bmm``, the upper triangle's sum (in double)
    and max, a sort per list for the categories, a broadcast compare for the overlap, ``torch.bincount`` for the exposure."""
    G, k = ids.shape
    N = int(vectors.shape[0])
    slot = torch.arange(k, device=ids.device)
    el = (slot[None, :] < count[:, None]) & (ids >= 0) & (ids < N)
    safe = torch.where(el, ids, torch.zeros_like(ids))
    out = {"elements": el.sum(dim=1, dtype=torch.int32)}
    rows = vectors[safe]
    gram = torch.bmm(rows, rows.transpose(1, 2))
    pair = (el[:, :, None] & el[:, None, :]).triu(1)
    out["sim_sum"] = torch.where(pair, gram, torch.zeros_like(gram)).sum(dim=(1, 2), dtype=torch.float64)
    out["sim_max"] = torch.where(pair, gram, torch.full_like(gram, float("-inf"))).amax(dim=(1, 2))
    if category is not None:
        big = torch.iinfo(torch.int64).max
        c = torch.where(el, category[safe].to(torch.int64), torch.full_like(safe, big)).sort(dim=1).values
        new = torch.ones_like(c, dtype=torch.bool)
        new[:, 1:] = c[:, 1:] != c[:, :-1]
        out["categories"] = (new & (c != big)).sum(dim=1, dtype=torch.int32)
        run = slot[None, :] - torch.where(new, slot[None, :], torch.zeros_like(c)).cummax(dim=1).values + 1
        out["category_max"] = torch.where(c != big, run, torch.zeros_like(run)).amax(dim=1).to(torch.int32)
    if base_ids is not None:
        bel = (torch.arange(base_ids.shape[1], device=ids.device)[None, :] < base_count[:, None]) & (base_ids >= 0) & (base_ids < N)
        hit = ((ids[:, :, None] == base_ids[:, None, :]) & bel[:, None, :]).any(dim=2)
        out["overlap"] = (hit & el).sum(dim=1, dtype=torch.int32)
    if exposure is not None:
        exposure += torch.bincount(ids[el], minlength=N).to(torch.int32)
        out["exposure"] = exposure
    return out


def bench_list_quality(news_num=65238, d=400, rounds=5):
    """``evaluate.list_quality`` against ``torch_list_quality`` (what the tree had), the two legs in turn in one process, median
    [min, max] of ``rounds`` rounds: G in {64, 4 096} lists of k in {10, 100} ids of a table of ``news_num`` unit rows, the
    exposure histogram always, without and with category (17 values) and base list (the list rolled by k // 2)."""
    from digat_amd import evaluate, util
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    table = util.unit_rows(torch.randn(news_num, d, generator=g).to(dev))
    category = torch.randint(0, 17, (news_num,), generator=g, dtype=torch.int32).to(dev)
    print(f"list-quality: lists of k ids of {news_num} unit rows, d = {d}; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for G in (64, 4096):
        for k in (10, 100):
            ids = torch.randint(0, news_num, (G, k), generator=g).to(dev)
            count = torch.full((G,), k, dtype=torch.int32, device=dev)
            base = torch.cat([ids[:, k // 2:], torch.randint(0, news_num, (G, k // 2), generator=g).to(dev)], dim=1).contiguous()
            for extras in (False, True):
                cat, b, bc = (category, base, count) if extras else (None, None, None)
                ea, eb = (torch.zeros(news_num, dtype=torch.int32, device=dev) for _ in range(2))
                ours = lambda: evaluate.list_quality(ids, count, table, cat, b, bc, ea)
                stock = lambda: torch_list_quality(ids, count, table, cat, b, bc, eb)
                got, want = ours(), stock()
                torch.cuda.synchronize()
                ints = all(torch.equal(got[key], want[key]) for key in got if key not in ("sim_sum", "sim_max"))
                off = float((got["sim_sum"] - want["sim_sum"]).abs().max())
                (a, alo, ahi), (bb, blo, bhi) = alternate(ours, stock, rounds=rounds, iters=5)
                print(f"  G = {G:5d}, k = {k:3d}, category and base list {'yes' if extras else 'no '}: list_quality {a:8.3f} ms [{alo:.3f}, {ahi:.3f}] | "
                      f"gather + bmm + torch reductions {bb:8.3f} ms [{blo:.3f}, {bhi:.3f}] (x{bb / a:.2f}) | integers equal: {ints}, "
                      f"largest |sim_sum difference| {off:.2e}", flush=True)


def stock_bootstrap_sums(values, replicates, generator, budget=1 << 30):
    """Bootstrap sums built only from stock PyTorch: ``torch.randint`` indices, a row gather and ``sum`` over the draws, the
    replicates in chunks whose [chunk, n] int64 indices and [chunk, n, c] float64 rows together stay near ``budget`` bytes.  Its own
    draws (torch's generator), so its sums are another sample of the same distribution, not the kernel's numbers."""
    n, c = values.shape
    per = max(1, budget // (n * (8 + 8 * c)))
    out = torch.empty((replicates, c), dtype=torch.float64, device=values.device)
    for b0 in range(0, replicates, per):
        nb = min(per, replicates - b0)
        idx = torch.randint(0, n, (nb, n), device=values.device, generator=generator)
        out[b0:b0 + nb] = values[idx].sum(dim=1)
    return out


def bench_bootstrap(units=0, columns=0, replicates=0, rounds=5, host_replicates=20):
    """``evaluate.bootstrap_sums`` (one kernel: hash, gather, add in registers) against ``stock_bootstrap_sums`` (what stock torch can
    do) and ``evaluate.bootstrap_sums_host`` (the numpy twin, at ``host_replicates`` replicates: reported as measured, never
    extrapolated), the legs in turn in one process, median [min, max] of ``rounds`` rounds, time and peak device bytes.  Default
    shapes: MIND-small dev's 73 152 impressions x 4 and 8 columns x 1 000 and 10 000 replicates, and 4 096 units x 8 columns."""
    import time
    from digat_amd import evaluate
    dev = torch.device("cuda:0")
    shapes = [(units, columns, replicates)] if units else [(73152, 4, 1000), (73152, 4, 10000), (73152, 8, 1000), (73152, 8, 10000),
                                                            (4096, 8, 1000), (4096, 8, 10000)]
    stat = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base
    print(f"bootstrap: sums [B, c] of B replicates of n draws from values [n, c] float64; ms per call, median [min, max] of {rounds} rounds", flush=True)
    for n, c, B in shapes:
        g = torch.Generator(device="cpu").manual_seed(0)
        host = torch.rand(n, c, generator=g, dtype=torch.float64)
        values = host.to(dev)
        gd = torch.Generator(device=dev).manual_seed(0)
        ours = lambda: evaluate.bootstrap_sums(values, B, seed=1)
        stock = lambda: stock_bootstrap_sums(values, B, gd)
        _lib._workspaces.clear()                        # the cached workspace of the shape before is no part of this call's peak
        (got, pa), (other, pb) = peak(ours), peak(stock)
        # the two legs draw differently: their replicate means agree as two samples of one distribution do
        gm, om = got.mean(dim=0) / n, other.mean(dim=0) / n
        gs = got.std(dim=0) / n
        apart = float(((gm - om).abs() / (gs * (2.0 / B) ** 0.5)).max())
        times = ([], [])
        for _ in range(rounds):
            for leg, fn in zip(times, (ours, stock)):
                leg.append(timeit(fn, iters=3, warm=1)[0])
        (a, alo, ahi), (b, blo, bhi) = (stat(t) for t in times)
        hb = min(B, host_replicates)
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = evaluate.bootstrap_sums_host(host.numpy(), hb, seed=1)
            secs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        evaluate.bootstrap_draws_host(n, hb, seed=1)
        draws_s = time.perf_counter() - t0
        err = float((got[:hb].cpu() - torch.from_numpy(want)).abs().max())
        ws = int(_lib.lib().digat_bootstrap_workspace_bytes(n, c, B))
        print(f"  n = {n:6d}, c = {c:2d}, B = {B:6d}: bootstrap_sums {a:9.3f} ms [{alo:.3f}, {ahi:.3f}] ({n * B / a / 1e6:7.2f} G draws/s, workspace "
              f"{ws / 2**20:.2f} MiB, peak {pa / 2**20:.2f} MiB) | randint + gather + sum {b:9.3f} ms [{blo:.3f}, {bhi:.3f}] (x{b / a:.2f}, peak "
              f"{pb / 2**20:.1f} MiB) | numpy twin at B = {hb}: {1e3 * sorted(secs)[1]:9.1f} ms ({n * hb / sorted(secs)[1] / 1e6:.2f} M draws/s; the draws "
              f"alone {1e3 * draws_s:.1f} ms) | largest |kernel - twin| {err:.2e}, legs' means apart by {apart:.2f} standard errors", flush=True)
        del got, other, values
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "xattn"
    nums = [int(v) for v in sys.argv[2:]]
    if what == "xattn":
        bench_xattn(*nums)
    elif what == "xattn-entry":
        bench_xattn_entry(*nums)
    elif what == "xattn-mind":
        bench_xattn(*nums, density="mind")
    elif what == "msa":
        bench_msa(*nums)
    elif what == "msa-train":
        bench_msa_train(*nums)
    elif what == "cnn":
        bench_cnn(*nums)
    elif what == "cnn-train":
        bench_cnn_train(*nums)
    elif what == "nrms-news":
        bench_nrms_news(*nums)
    elif what == "nrms-user":
        bench_nrms_user(*nums)
    elif what == "nrms-train":
        bench_nrms_train(*nums)
    elif what == "sag":
        bench_sag(*nums)
    elif what == "sag-lists":
        bench_sag_lists(*nums)
    elif what == "topic":
        bench_topic(*nums)
    elif what == "user-graph":
        bench_user_graph(*nums)
    elif what == "train-input":
        bench_train_input(*nums)
    elif what == "ablation-score":
        bench_ablation_score(*nums)
    elif what == "topk":
        bench_topk(*nums)
    elif what == "recommend":
        bench_recommend(*nums)
    elif what == "dot-topk":
        bench_dot_topk(*nums)
    elif what == "shortlist":
        bench_shortlist(*nums)
    elif what == "dot-shortlist":
        bench_dot_shortlist(*nums)
    elif what == "qdot":
        bench_qdot(*nums)
    elif what == "dot-rank":
        bench_dot_rank(*nums)
    elif what == "pool-softmax":
        bench_pool_softmax(*nums)
    elif what == "list-softmax":
        bench_list_softmax(*nums)
    elif what == "list-pairwise":
        bench_list_pairwise(*nums)
    elif what == "diversify":
        bench_diversify(*nums)
    elif what == "list-quality":
        bench_list_quality(*nums)
    elif what == "calibrate":
        bench_calibrate(*nums)
    elif what == "rerank":
        bench_rerank(*nums)
    elif what == "exposure-cap":
        bench_exposure_cap(*nums)
    elif what == "pl-sample":
        bench_pl_sample(*nums)
    elif what == "off-policy":
        demo_off_policy(*nums)
    elif what == "pl-expect":
        bench_pl_expect(*nums)
    elif what == "off-policy-steps":
        demo_off_policy_steps(*nums)
    elif what == "list-pl":
        bench_list_pl(*nums)
    elif what == "policy":
        demo_policy(*nums)
    elif what == "plrank":
        bench_plrank(*nums)
    elif what == "bootstrap":
        bench_bootstrap(*nums)
    elif what == "linear":
        bench_linear(*nums)
    elif what == "gemm":
        bench_gemm(*nums)
