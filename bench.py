#!/usr/bin/env python3
"""bench.py — MIND-shaped dev impressions scored per second through the HIP DIGAT path.

A step = one pass of the hot path over one launch set of B=4096 (impression, candidate) rows — util.LAUNCH_ROWS: four of the
reference's 1024-row dev batches (main.py:42) scored together; the 1024-row figure is extra_workloads[".../reference-batch-1024"]
— of a synthetic MIND-shaped dev set: on-device gather of the batch from the HBM-resident corpus tables (util.py:65-67 of the
reference) + ``Model.inference`` (DIGAT.inference, fp32) + dot-product logits.  Inputs are resident in HBM
before the timed region.  The corpus has the real scale of the data set the workload names (MIND-small: 65 238 news,
MIND-large: 161 013) and no batch is visited twice inside the timed region.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload: N=1 -> BASELINE.json configs[1] (MIND-small default); N>1 -> configs[3]'s shape (MIND-large default), rows
sharded over the ranks, the final all_gather of the scores inside the timed region.  ``--mode train`` times the
DDP training step instead (trainer.py:71-105; RCCL gradient all-reduce).

A plain run does what the headline needs and no more: setup, pre-warm, warm-up, the K timed steps, the result line.  Its
warm-up and timed steps take the same batches of the same seeded corpus every run, and ``--dump-outputs DIR`` writes what
the last timed step returned (rank 0's scores of that batch) to DIR/scores.npy (float32), so that two builds can be compared
output for output.  The AUC matches are not run (the metric says so); ``--full`` runs them.

``--full`` adds everything else: the per-kernel profile of the timed region and the untimed profiling passes behind the
rooflines, the oracle / reference checks, the extra workloads, precisions and batch sizes, the training step, the end-to-end
run, the one-GPU reference of a multi-GPU run and the full result document (bench_detail.json).  Rank 0 prints ONE JSON line
(metric, value, unit, ms_per_step, ...); with ``--full`` it carries these extra objects:
  roofline         the dominant kernel of the step, timed live with HIP events over the timed region
  roofline_xattn   the fused Eq. 8 kernel of the user graph against the HBM roofline (what north_star asks for)
  cpu_baseline     the oracle (unfused reference algorithm, torch-CPU) on a bounded sample, N=1 only
  extra_workloads  (N=1) a few steps of mind-small-stress and mind-large-default in the same invocation
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense fp32 matrix peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 matrix peak (the 5 PF headline is 2:1 sparse)

WORKLOADS = {
    # BASELINE.json configs[1]
    "mind-small-default": dict(sag_neighbors=3, sag_hops=2, depth=3, category_num=17, news_num=65238, dropout=0.2,
                               label="MIND-small default: --graph_encoder=DIGAT neighbors=3 hops=2 (N=10, U=67), "
                                     "d=400, graph_depth=3, fp32 dev inference"),
    # BASELINE.json configs[2]
    "mind-small-stress": dict(sag_neighbors=8, sag_hops=2, depth=7, category_num=17, news_num=65238, dropout=0.2,
                              label="MIND-small stress: neighbors=8 hops=2 (N=65, U=67), d=400, graph_depth=7"),
    # BASELINE.json configs[3] shape (18 categories, 161 013 news)
    "mind-large-default": dict(sag_neighbors=5, sag_hops=2, depth=3, category_num=18, news_num=161013, dropout=0.1,
                               label="MIND-large default shape: neighbors=5 hops=2 (N=26, U=68), d=400, graph_depth=3"),
}
# not a BASELINE config: the MIND-small default shapes with the OTHER adjacency regime real MIND also holds (full histories in 2-4
# categories: 16 adjacency entries per user-graph node instead of 4.8, 79 % of the nodes live instead of 44 %)
WORKLOADS["mind-small-heavy-history"] = dict(WORKLOADS["mind-small-default"], history_profile="heavy",
                                             label="MIND-small default shapes, heavy histories: H = 50 for every user in 2-4 categories "
                                                   "(N=10, U=67, d=400, graph_depth=3)")
MIND_SMALL_DEV_ROWS = 2_740_000      # 73 152 impressions, ~2.74 M candidate rows
MIND_SMALL_DEV_IMPRESSIONS = 73_152
REFERENCE_BATCH = 1024               # the reference's dev batch: batch_size * 16 rows (main.py:42)


def usable_cores() -> int:
    """Host cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="infer", choices=["infer", "train", "e2e"],
                    help="infer: dev scoring (the metric); train: the DDP training step (trainer.py:71-105); e2e: only the end-to-end "
                         "dev run (title tokens -> rank file), which infer --full also appends at N = 1")
    ap.add_argument("--e2e-impressions", type=int, default=MIND_SMALL_DEV_IMPRESSIONS,
                    help="impressions of the end-to-end dev run of --mode e2e and --full (MIND-small dev: 73 152; 0 = skip it)")
    ap.add_argument("--batch", type=int, default=4096,
                    help="rows per step = rows per launch set (util.LAUNCH_ROWS; the reference's dev batch is batch_size*16 = 1024 rows, "
                         "main.py:42: sized for a 24 GB card, rows are independent)")
    ap.add_argument("--workload", default="auto", choices=["auto"] + sorted(WORKLOADS),
                    help="auto: mind-small-default on one GPU (BASELINE configs[1]), mind-large-default on several (configs[3])")
    ap.add_argument("--impressions", type=int, default=40000, help="synthetic impressions per rank (~37 rows each)")
    ap.add_argument("--news", type=int, default=0, help="synthetic news corpus size (0 = the data set's real size)")
    ap.add_argument("--cpu-rows", type=int, default=1536, help="--full: max rows of the CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="--full: time bound of the CPU-baseline sample")
    ap.add_argument("--extra-steps", type=int, default=12, help="--full: timed steps of each extra workload at N=1 (0 = skip)")
    ap.add_argument("--train-precision", default="fp32", choices=["fp32", "bf16"],
                    help="--mode train: bf16 = bf16 matrix-core operands for the large training GEMMs (BASELINE configs[4])")
    ap.add_argument("--per-row-users", action="store_true",
                    help="expand the user tensors per row as the reference's driver does (default: once per impression)")
    ap.add_argument("--train-news-encoder", default="table", choices=["table", "msa"],
                    help="--mode train: 'table' = news representations from a trainable table (graph-encoder step only); 'msa' = the "
                         "reference's full step, MSA news encoder on the titles of 64 x (5 x N + H) news per step")
    ap.add_argument("--fused-user-context", action="store_true",
                    help="compute_user_graph_context as one launch (csrc/digat_ctxfused.inc; measured at parity with the three launches: opt-in)")
    ap.add_argument("--detail", default=None, help="where the full result document goes (default: bench_detail.json next to bench.py)")
    ap.add_argument("--projection", default="auto", choices=["auto", "bf16x6", "bf16x6-pq3", "fp32", "pq-bf16", "pq-bf16-x1", "pq-fp8", "fp16x3"],
                    help="node projections: split-bf16 (fp32-equivalent) on the bf16 matrix cores, or fp32 MFMA; pq-bf16 = BASELINE "
                         "configs[4]: P', Q of the user graph's Eq. 8 stored in bf16 (three bf16 products; -x1: one); pq-fp8: stored as block-scaled e4m3")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: per-kernel profile and rooflines, CPU baseline and AUC matches, extra workloads and "
                         "precisions, training step, end-to-end run, one-GPU reference at N > 1, the full result document")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="--mode infer: write the scores of the last timed step (rank 0) to DIR/scores.npy, float32")
    return ap.parse_args()


def self_launch(args) -> None:
    """``python bench.py --gpus N`` (N > 1) without a launcher: start ``torch.distributed.run`` with one rank per GPU as a CHILD
    process and relay its output and exit code.  This parent never touches the GPU (no HIP call is made before this point:
    replacing or forking a process that has initialised the GPU is what the GPU boxes forbid), so the ranks start clean.
    The launcher path of the task's contract (``python -m torch.distributed.run ... bench.py --gpus N``) sets WORLD_SIZE and
    never comes here."""
    import socket
    import subprocess
    with socket.socket() as sock:                    # a free rendezvous port on the loopback interface
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this image
    print(f"[bench] --gpus {args.gpus} without a launcher: starting {' '.join(cmd[1:6])} ... as a child process", file=sys.stderr, flush=True)
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


class Dist:
    """The control plane of a run: world, rank, barrier, reductions of timing scalars."""

    def __init__(self, args):
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != args.gpus:
            if "WORLD_SIZE" not in os.environ and args.gpus > 1:
                self_launch(args)                   # does not return
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={self.world}")
        assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU path)"
        # test hook (one-GPU boxes): DIGAT_BENCH_TEST_SHARED_GPU=1 puts every rank on cuda:0 and runs the collectives over gloo
        self.shared_gpu = os.environ.get("DIGAT_BENCH_TEST_SHARED_GPU") == "1"
        self.device_index = 0 if self.shared_gpu else self.local_rank
        torch.cuda.set_device(self.device_index)
        self.dev = torch.device("cuda", self.device_index)
        self.ctl_dev = torch.device("cpu") if self.shared_gpu else self.dev
        self.nccl_log = None
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            self.backend = "gloo" if self.shared_gpu else "nccl"                   # nccl = RCCL on ROCm
            if self.backend == "nccl" and "NCCL_DEBUG" not in os.environ:
                # first-run insurance for the 8-GPU node: RCCL's own account of the transports it chose (xGMI P2P / SHM / NET),
                # per rank, to a file; rank 0 condenses its file into the line (rccl_summary)
                import tempfile
                self.nccl_log = os.path.join(tempfile.gettempdir(), f"digat_bench_rccl_{os.environ.get('MASTER_PORT', '0')}_r{self.rank}.log")
                os.environ["NCCL_DEBUG"] = "INFO"
                os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,GRAPH"
                os.environ["NCCL_DEBUG_FILE"] = self.nccl_log
            dist.init_process_group(self.backend)
            self.world_seen = dist.get_world_size()
        else:
            self.backend, self.world_seen = None, 1

    def fence(self):
        torch.cuda.synchronize()
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()

    def reduce(self, values, op="sum"):
        if self.world == 1:
            return [float(v) for v in values]
        import torch.distributed as dist
        t = torch.tensor(list(values), dtype=torch.float64, device=self.ctl_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)
        return [float(v) for v in t.tolist()]

    def close(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()

    def rccl_summary(self):
        """Rank 0's RCCL log condensed: which transports the channels use and how many rings / trees were built."""
        if self.world == 1:
            return None
        if not self.nccl_log:
            return {"backend": self.backend, "log": None}
        import re
        try:
            text = open(self.nccl_log, errors="replace").read()
        except OSError as exc:
            return {"backend": self.backend, "log": self.nccl_log, "error": repr(exc)}
        via = {}
        for m in re.finditer(r"\bvia\s+([A-Za-z0-9_/]+)", text):
            via[m.group(1)] = via.get(m.group(1), 0) + 1
        nranks = re.findall(r"nranks\s+(\d+)", text)
        return {"backend": self.backend, "log": self.nccl_log, "log_bytes": len(text), "channel_transports": via,
                "mentions_xgmi": len(re.findall(r"(?i)xgmi", text)), "nranks_in_log": sorted(set(int(v) for v in nranks)),
                "rings_or_trees": len(re.findall(r"(?m)\b(Ring|Tree|Trees)\b", text)),
                "version_line": next((l.strip()[-120:] for l in text.splitlines() if "version" in l.lower()), None)}

    def device_names(self):
        """Every rank's device as it names itself (rank order): evidence of WHICH GPUs a multi-GPU line ran on."""
        mine = f"{torch.cuda.get_device_name(self.device_index)} (cuda:{self.device_index}, pid {os.getpid()})"
        if self.world == 1:
            return [mine]
        import torch.distributed as dist
        names = [None] * self.world
        dist.all_gather_object(names, mine)
        return names


class SoloView:
    """One rank of a multi-rank run measuring by itself (the other ranks wait at the next fence): same device, no collectives."""

    def __init__(self, D: "Dist"):
        self.rank, self.world, self.dev, self.shared_gpu = D.rank, 1, D.dev, D.shared_gpu
        self.device_index, self.backend, self.world_seen = D.device_index, None, 1

    def fence(self):
        torch.cuda.synchronize()

    def reduce(self, values, op="sum"):
        return [float(v) for v in values]


def build_workload(name, args, D: Dist, impressions, trainable=False):
    """Corpus + model + device tables of one workload; the per-news caches (c_n0, layer-0 tables) are timed as setup."""
    from digat_amd import synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    wl = WORKLOADS[name]
    news_num = args.news or wl["news_num"]
    spec = synthetic.SynthSpec(news_num=news_num, sag_neighbors=wl["sag_neighbors"], sag_hops=wl["sag_hops"],
                               category_num=wl["category_num"], impressions=impressions, seed=D.rank,
                               history_profile=wl.get("history_profile", "mind"))
    corpus = synthetic.make_corpus(spec)       # each rank owns its shard of the dev rows (weak scaling)
    N, H, C, d, L = spec.news_graph_size, spec.max_history_num, spec.category_num, spec.embedding_dim, wl["depth"]
    state = synthetic.make_state_dict(d, C, L, seed=0, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=N, max_history_num=H,
                                category_num=C, graph_depth=L, dropout_rate=wl["dropout"])
    text_encoder = trainable and getattr(args, "train_news_encoder", "table") == "msa"
    if text_encoder:        # the reference's full training step: the MSA news encoder on title text (synthetic tokens, random init)
        cfg.vocabulary_size, cfg.word_embedding_dim, cfg.max_title_length = 30000, 300, 32
        cfg.MSA_head_num, cfg.MSA_head_dim, cfg.attention_dim = 16, 25, 256
        model = Model(cfg)
        model.news_encoder.initialize()
        with torch.no_grad():
            model.news_encoder.word_embedding.weight.mul_(0.1)          # GloVe-like magnitudes
    else:
        model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding), trainable=trainable))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(D.dev)
    model.graph_encoder.projection_mode = args.projection
    model.graph_encoder.fused_user_context = bool(getattr(args, "fused_user_context", False))
    dc = util.DeviceCorpus.from_numpy(corpus, D.dev)
    if text_encoder:
        text, mask = synthetic.make_titles(news_num, cfg.max_title_length, cfg.vocabulary_size, seed=7)
        dc.title_text = torch.from_numpy(text).to(torch.int32).to(D.dev)
        dc.title_mask = torch.from_numpy(mask).to(D.dev)
    W = types.SimpleNamespace(name=name, wl=wl, spec=spec, corpus=corpus, model=model, dc=dc, state=state, cfg=cfg,
                              N=N, H=H, C=C, d=d, L=L, mean_cand=corpus.rows / float(spec.impressions), setup_ms=None)
    if not trainable:
        model.eval()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if hasattr(model.graph_encoder, "pass_rows"):
            model.graph_encoder.pass_rows = args.batch
        util.prepare_news_side(model.graph_encoder, dc, args.batch)     # SA gather + c_n0 + layer-0 tables (setup, untimed)
        torch.cuda.synchronize()
        W.setup_ms = (time.perf_counter() - t0) * 1e3
    tables = {k: getattr(dc, k) for k in ("news_embedding", "SA_news_representations", "c_n0", "news_hpq0", "user_hpq0", "ctxq0", "news_graph",
                                          "user_graph", "history")}
    W.table_bytes = {k: int(v.numel() * v.element_size()) for k, v in tables.items() if v is not None}
    return W


class Scorer:
    """The driver's scoring loop (util.score_rows) over the dev rows in order: the grouped inputs of batch k+1 are gathered
    on a side stream while batch k is scored (util.GroupedBatchPipeline), consecutive batches alternate over three HIP
    streams (util.batch_streams; env DIGAT_BENCH_LANES).  Batches are taken in order and wrap around only when the corpus is exhausted
    (``revisited`` says whether that happened)."""
    CHUNK = 512                                    # batches per pipeline instance (index arrays are built per instance)

    def __init__(self, W, args, D: Dist, keep_scores=False):
        from digat_amd import util
        self.util, self.W, self.B, self.dev = util, W, args.batch, D.dev
        self.per_row = args.per_row_users
        self.nbatches = max(1, W.dc.rows // self.B)
        self.imp_host = W.corpus.row_impression
        self.lanes = util.batch_streams(D.dev, int(getattr(args, "lanes", 0) or os.environ.get("DIGAT_BENCH_LANES", "3")))
        self.nlanes = len(self.lanes)
        self.lane_scores = [torch.empty(self.B, dtype=torch.float32, device=D.dev) for _ in self.lanes]
        self.k, self.base, self.pipe, self.order, self.last = 0, 0, None, None, None
        self.kept = [] if keep_scores else None
        enc = W.model.graph_encoder
        util.apply_corpus_hint(enc, W.dc)            # this corpus's sparse / dense choice (several workloads share the process)
        if hasattr(enc, "pass_rows"):
            # rows per pass name the kernel of the [B,d] linears (util.score_rows does the same); per-news tables made under the
            # other name are rebuilt, untimed
            enc.pass_rows = args.batch
            if W.dc.weights_key is not None and W.dc.weights_key != util.weights_key(enc, W.dc):
                util.prepare_news_side(enc, W.dc, args.batch)
        with torch.cuda.stream(self.lanes[0]):
            W.model.graph_encoder._params()        # split weights / folded queries built before the lanes fork (util.score_rows)

    @property
    def revisited(self):
        return self.k > self.nbatches

    def _start_chunk(self, k):
        util, W, B = self.util, self.W, self.B
        self.base = k
        self.order = [(((k + j) % self.nbatches) * B, min(((k + j) % self.nbatches) * B + B, W.dc.rows)) for j in range(self.CHUNK)]
        if self.pipe is not None:             # the old pipeline's buffers return to the allocator: every lane must be done with them
            self.join()
            with torch.cuda.stream(self.lanes[0]):
                self.pipe.drain()
        enc = W.model.graph_encoder
        self.pipe = None if self.per_row else util.GroupedBatchPipeline(
            W.dc, self.order, self.imp_host, nsets=len(self.lanes),
            news_sparse=(enc.resolved_xattn_mode("news") == "sparse") if hasattr(enc, "resolved_xattn_mode") else None)
        for extra in self.lanes[1:]:
            extra.wait_stream(self.lanes[0])

    def restart(self):
        """Back to batch 0 with a fresh pipeline, built here rather than inside the next step."""
        self.k = 0
        self._start_chunk(0)

    def last_scores(self):
        """What the caller of the last step received: the scores of that step's batch (host copy, after a fence)."""
        lane, n, kept = self.last
        return (kept if kept is not None else self.lane_scores[lane][:n]).float().cpu().numpy()

    def step(self):
        util, W, k = self.util, self.W, self.k
        if self.pipe is None and self.order is None or k - self.base >= self.CHUNK:
            self._start_chunk(k)
        s, e = self.order[k - self.base]
        lane = k % self.nlanes
        with torch.no_grad(), torch.cuda.stream(self.lanes[lane]):
            inputs = self.pipe.take(k - self.base) if self.pipe is not None else None
            if inputs is None:
                out = W.model.inference(*util.gather_batch(W.dc, s, e))
            else:
                out = W.model.inference_grouped(*inputs)
            if self.kept is not None:
                self.kept.append(out)
            else:
                self.lane_scores[lane][:e - s] = out
            if self.pipe is not None:
                self.pipe.scored(k - self.base)
        self.last = (lane, e - s, out if self.kept is not None else None)
        self.k = k + 1
        return e - s

    def join(self):
        for extra in self.lanes[1:]:
            self.lanes[0].wait_stream(extra)


def run_inference(W, args, D: Dist, steps, warmup, with_profile=True, gather_scores=False, keep_last=False):
    """Pre-warm, W warm-up steps, exactly K timed steps between fences -> timing + the library's per-kernel events
    (with_profile) + the scores of the last timed step (keep_last)."""
    from digat_amd import _lib, util
    sc = Scorer(W, args, D, keep_scores=False)
    L = W.L
    # per-kernel HIP events cost the host two hipEventRecord calls per launch (~140 per step): every PROFILE_EVERY-th
    # step of the timed region is recorded, the others run unobserved.  The profiler is set up (thousands of
    # hipEventCreate) BEFORE the warm-up, so that the timed region follows the warm-up without an idle gap.
    PROFILE_EVERY = int(os.environ.get("DIGAT_BENCH_PROFILE_EVERY", "4"))
    ROOF_KINDS = (1 << _lib.KERNEL_KINDS.index("proj")) | (1 << _lib.KERNEL_KINDS.index("xattn"))
    if with_profile:
        # inside the timed region only the two kernels the rooflines are about get their event pairs (the projection GEMM and
        # Eq. 8: ~10 pairs per sampled step); every pair is two marker packets in a queue, and recording all ~70 launches of a
        # sampled step cost the overlapped encoder 3-4 % of throughput (1.273 vs 1.228 ms per step at 300 steps).  The
        # all-kinds breakdown (kernel_ms_per_step) comes from an untimed pass right after, same streams and batches in flight.
        _lib.lib().digat_profile_set_kinds(ROOF_KINDS)
        _lib.profile_start(64 * (steps // PROFILE_EVERY + 2) * (L + 1))
        _lib.lib().digat_profile_pause(1)
    # Setup, untimed: bring the GPU out of its idle power state (the setup above leaves it idle for ~100 ms and the
    # clocks need tens of milliseconds of load to come back: with 5 warm-up steps = 10 ms the first timed steps ran at
    # half speed).  A dev run scores ~2 600 such batches back to back; steady state is what the metric means.
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.3:
        for _ in range(8):
            sc.step()
        torch.cuda.synchronize()
    # the pre-warm took as many batches as the clock allowed: from here on (a fixed number of tuning steps, the warm-up, the
    # timed steps) the batches are the same every run, and so are the scores of the last timed step
    sc.restart()
    # Setup, untimed: how many batches to keep in flight (util.batch_streams: 3 is best at the default shapes, 2 at the stress
    # shape and with bf16 P', Q — the optimum moves with the kernels' lengths, so it is measured, 2 x 30 steps per candidate)
    t_tune = time.perf_counter()
    if "DIGAT_BENCH_LANES" not in os.environ and len(sc.lanes) >= 3:
        trials = {2: [], 3: []}
        for n in (3, 2, 3, 2, 3, 2):               # alternating rounds; the MEDIAN of each setting counts, and two batches in flight
            sc.join()                              # replace three only when clearly better (a coin-flip choice cost 3 % of a run)
            sc.nlanes = n
            for _ in range(max(3, 6 * 1024 // sc.B)):
                sc.step()
            torch.cuda.synchronize()
            t_n = time.perf_counter()
            for _ in range(max(12, 40 * 1024 // sc.B)):
                sc.step()
            torch.cuda.synchronize()
            trials[n].append(time.perf_counter() - t_n)
        sc.join()
        med = {n: sorted(v)[len(v) // 2] for n, v in trials.items()}
        sc.nlanes = 2 if med[2] < 0.98 * med[3] else 3
    torch.cuda.synchronize()
    untimed_s = {"prewarm": round(t_tune - t_pre, 3), "lane_tuning": round(time.perf_counter() - t_tune, 3)}
    for _ in range(warmup):
        sc.step()
    if gather_scores:                      # N > 1: the timed steps keep their scores for the closing all_gather
        sc.kept = []
    D.fence()
    profiled_steps = rows_done = 0
    _lib.lib().digat_profile_marker(1, _lib.stream_ptr())       # landmark for tools/trace_region.py: the timed region begins
    t0 = time.perf_counter()
    for i in range(steps):
        sampled = with_profile and i % PROFILE_EVERY == 0
        if with_profile:
            _lib.lib().digat_profile_pause(0 if sampled else 1)
        profiled_steps += int(sampled)
        rows_done += sc.step()
    gathered, gather_ms = None, None
    if gather_scores:
        # the multi-GPU driver's last act (util.compute_scores): every rank's block of scores to every rank, rank order
        sc.join()
        torch.cuda.synchronize()                      # every score of this rank exists: what follows is the exchange alone
        t_g0 = time.perf_counter()
        with torch.cuda.stream(sc.lanes[0]):
            local = torch.cat(sc.kept) if sc.kept else torch.empty(0, device=D.dev)
            counts = [int(v) for v in D.reduce([float(local.numel()) if r == D.rank else 0.0 for r in range(D.world)])]
            gathered = util.all_gather_scores(local.cpu() if D.shared_gpu else local, counts)
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - t_g0) * 1e3
        sc.kept = None
    D.fence()
    elapsed = time.perf_counter() - t0
    _lib.lib().digat_profile_marker(2, _lib.stream_ptr())       # ... and ends
    out = types.SimpleNamespace(elapsed=elapsed, rows_done=rows_done, profiled_steps=profiled_steps, revisited=sc.revisited,
                                batches_in_flight=sc.nlanes, untimed_s=untimed_s, all_gather_ms=gather_ms,
                                prof=None, prof_iso=None, live_fraction=None, iso_steps=0,
                                gathered_rows=None if gathered is None else int(gathered.numel()),
                                last_scores=sc.last_scores() if keep_last and steps > 0 else None)
    out.prof_all, out.all_steps = None, 0
    if with_profile:
        out.prof = _lib.profile_stop()
        lf = float(_lib.lib().digat_profile_live_row_fraction())
        out.live_fraction = lf if lf >= 0 else None
        # untimed, overlapped as the timed region was: every kind recorded, for the per-kind breakdown
        _lib.lib().digat_profile_set_kinds(0xffffffff)
        out.all_steps = min(steps, 12)
        _lib.profile_start(64 * (out.all_steps + 1) * (L + 1))
        for _ in range(out.all_steps):
            sc.step()
        sc.join()
        torch.cuda.synchronize()
        out.prof_all = _lib.profile_stop()
        # The timed region overlaps the news-graph kernels with the user graph's on a side stream, so the launch
        # durations above include the sharing.  A second, untimed pass on one stream gives each kernel's duration
        # with the chip to itself (reported as roofline.isolated_*; `frac` stays the timed region's).
        enc_iso = W.model.graph_encoder
        prev = enc_iso.side_stream
        enc_iso.side_stream = "off"
        sc.join()
        sc.nlanes = 1                              # ... and every batch on the same caller stream
        out.iso_steps = min(steps, 10)
        _lib.profile_start(64 * (out.iso_steps + 1) * (L + 1))
        for _ in range(out.iso_steps):
            sc.step()
        torch.cuda.synchronize()
        out.prof_iso = _lib.profile_stop()
        enc_iso.side_stream = prev
    sc.join()
    torch.cuda.synchronize()
    return out


def run_training(W, args, D: Dist, steps, warmup):
    """The DDP training step (trainer.py:71-105): 64 behaviours x (1 + 4) candidates per rank and step, Adam, clipping; with
    more than one rank the gradients are all-reduced by DistributedDataParallel over RCCL."""
    from digat_amd.trainer import SyntheticTrainSet, Trainer
    cfg = W.cfg
    cfg.epoch, cfg.batch_size, cfg.lr, cfg.weight_decay, cfg.gradient_clip_norm = 1, 64, 1e-4, 0.0, 1.0
    cfg.train_precision = args.train_precision
    ts = SyntheticTrainSet(W.corpus, 4, seed=D.rank)
    ts.negative_sampling()
    tr = Trainer(W.model, cfg, W.dc, ts, local_rank=(D.device_index if D.world > 1 else -1))
    tr.model.train()
    if D.world > 1 and hasattr(tr.model, "_set_ddp_runtime_logging_sample_rate"):
        tr.model._set_ddp_runtime_logging_sample_rate(1)          # DDP's own timers on every iteration (the all-reduce time below)
    nb = len(ts) // 64
    k = 0

    def step():
        nonlocal k
        idx = (np.arange(64) + 64 * (k % nb)) % len(ts)
        k += 1
        return tr.train_step(idx, read_loss=False)       # the loss stays on the device (Trainer.train sums it there and reads it per epoch)
    # pre-warm (clocks, allocator, code objects): by the clock on one rank; with more ranks every step is a collective (DDP's
    # gradient all-reduce), so every rank must take the SAME number of them — a per-rank clock would leave one rank waiting forever
    if D.world == 1:
        t_pre = time.perf_counter()
        while time.perf_counter() - t_pre < 0.5:
            step()
            torch.cuda.synchronize()
    else:
        for _ in range(24):
            step()
        torch.cuda.synchronize()
    for _ in range(warmup):
        step()
    D.fence()
    if os.environ.get("DIGAT_BENCH_CPROFILE"):         # where the host's time goes (diagnostic; changes the timing)
        import cProfile, pstats
        pr = cProfile.Profile()
        pr.enable()
        for _ in range(20):
            step()
        pr.disable()
        torch.cuda.synchronize()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(25)
    stamps = [] if os.environ.get("DIGAT_BENCH_STAMPS") else None
    if stamps is not None:
        import gc
        gc_log = []
        gc.callbacks.append(lambda phase, info: gc_log.append((time.perf_counter(), phase, info.get("generation"))))
        if os.environ.get("DIGAT_BENCH_STAMPS") == "freeze":
            gc.collect(); gc.freeze()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
        if stamps is not None:
            stamps.append(time.perf_counter())
    enqueue_s = time.perf_counter() - t0         # the host's share: when it is close to `elapsed` the step is host-bound in this run
    D.fence()
    elapsed = time.perf_counter() - t0
    if stamps:
        dt = np.diff(np.array([t0] + stamps)) * 1e3
        print("[bench] host ms per step:", " ".join(f"{v:.1f}" for v in dt), file=sys.stderr)
        starts = {}
        for t, phase, gen in gc_log:
            if phase == "start":
                starts[gen] = t
            elif gen in starts and t - starts[gen] > 2e-3:
                print(f"[bench] gc generation {gen}: {1e3 * (t - starts[gen]):.1f} ms at {1e3 * (starts[gen] - t0):.0f} ms into the timed loop", file=sys.stderr)
    roof = None
    if D.world == 1:
        # untimed: the MFMA launches of three more steps through the library's profiler (forward, input-gradient and
        # weight-gradient GEMMs: 2 M N K each, six bf16 products per fp32 product unless --train-precision bf16)
        from digat_amd import _lib
        _lib.lib().digat_profile_set_kinds(0xffffffff)
        _lib.profile_start(4096)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        prof = _lib.profile_stop()
        nprod = 1.0 if args.train_precision == "bf16" else 6.0
        flops = (prof["proj"]["work"] + prof["linear"]["work"]) / 3.0
        gemm_ms = (prof["proj"]["ms"] + prof["linear"]["ms"]) / 3.0
        gemm_bytes = (prof["proj"]["gemm_bytes"] + prof["linear"]["gemm_bytes"]) / 3.0

        def roof(ms_per_step):
            return {"kernel": "every MFMA launch of the step (forward, input-gradient and weight-gradient GEMMs)", "bound": "mfma",
                    "achieved": nprod * flops / (ms_per_step * 1e-3) / 1e12, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": nprod * flops / (ms_per_step * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, "traffic": None,
                    "algorithmic_flops_per_step": flops, "executed_flops_per_step": nprod * flops,
                    "gemm_launch_ms_per_step": gemm_ms, "gemm_hbm_bytes_per_step": gemm_bytes,
                    "frac_within_the_gemm_launches": nprod * flops / (gemm_ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS if gemm_ms > 0 else None,
                    "note": "a 320-row step is ~300 launches of 4-140 us, back to back on one stream: the step is bound by the latency of "
                            "its many small launches ([B,d] linears, reductions) and by the three 21 440-row products per user-graph layer, "
                            "not by the matrix cores' peak; the user graph's Eq. 8 runs on the entry-wise kernels forward and backward"}
    ddp = None
    if D.world > 1 and hasattr(tr.model, "_get_ddp_logging_data"):
        try:          # DistributedDataParallel's own measurements (nanoseconds, averaged over the sampled iterations)
            log = tr.model._get_ddp_logging_data()
            ddp = {k: round(float(log[k]) / 1e6, 4) for k in ("avg_forward_compute_time", "avg_backward_compute_time", "avg_backward_comm_time",
                                                                "avg_backward_compute_comm_overlap_time") if k in log}
            ddp["unit"] = "ms per step (DistributedDataParallel's timers; avg_backward_comm_time = the gradient all-reduce)"
            ddp["bucket_sizes_bytes"] = str(log.get("bucket_sizes", ""))
        except Exception as exc:          # the logging API is private: report, never fail the run
            ddp = {"error": repr(exc)}
    return types.SimpleNamespace(elapsed=elapsed, rows_done=steps * 64 * 5, loss=float(loss.item()), roofline=roof, ddp=ddp,
                                 enqueue_ms_per_step=enqueue_s / steps * 1e3)


# ---------------------------------------------------------------------------------------------------------------------
def rooflines(W, run, args):
    """roofline objects of the dominant kind and of the user graph's Eq. 8, from the library's per-kernel events."""
    enc = W.model.graph_encoder
    prof, prof_iso = run.prof, run.prof_iso
    kinds = {k: v for k, v in prof.items() if v["launches"] > 0}
    # dominant = the kind with the largest SOLO time per step (the untimed single-stream pass): inside the timed region the
    # chip is shared by three batches and their side streams, and a launch's duration there says how long it waited, not what it cost
    iso_ms = {k: prof_iso[k]["ms"] / max(1, run.iso_steps) for k in kinds if prof_iso.get(k, {}).get("launches", 0) > 0}
    # ... among the kinds that are ONE kernel each (proj: the strip-mined GEMM; topic, pool, agg): "linear" (three different small
    # GEMM kernels in a latency chain) and "glue" are sums over unlike kernels, and Eq. 8 ("xattn") has its own object below
    single = {k: v for k, v in iso_ms.items() if k in ("proj", "topic", "pool", "agg")}
    dom = max(single, key=single.get) if single else (max(iso_ms, key=iso_ms.get) if iso_ms else max(kinds, key=lambda k: kinds[k]["ms"]))
    symbols = {"proj": "gemm_bf16x6s_kernel<3" if getattr(enc, "projection_mode", "") != "fp32"
               else "gemm_f32_kernel<128, 80, 4, 1, 1, 1>",
               "xattn": "xattn_sparse_twin" if enc.resolved_xattn_mode("user") == "sparse" else "xattn_score_kernel",
               "agg": "xattn_agg_kernel", "topic": "topic_pool", "pool": "attn_pool_kernel"}

    def pmc_traffic(kind):
        # HBM traffic comes from separate rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE cannot share a pass) of this very
        # command; their per-launch means are kept under profiles/ and quoted here
        import glob
        if W.name != "mind-small-default":
            return None
        for path in sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc.json")), reverse=True):
            try:
                doc = json.load(open(path))
                table = doc["kernels"]
            except (OSError, ValueError, KeyError):
                continue
            if doc.get("rows_per_step", 1024) != args.batch:      # per-launch bytes belong to the launch size they were counted at
                continue
            # every instantiation of the kind's kernel (the projection GEMM launches as <3,true,2,...> on big row counts and
            # <3,true,1,...> on the small news-side ones): the launch-weighted mean, like the kind's own average launch time
            hits = [(name, v) for name, v in table.items() if symbols.get(kind, "\0") in name]
            if hits:
                n = sum(v["launches"] for _, v in hits)
                return {"bytes_per_launch": sum(v["hbm_bytes_mean"] * v["launches"] for _, v in hits) / max(n, 1),
                        "kernel": max(hits, key=lambda h: h[1]["hbm_bytes_mean"] * h[1]["launches"])[0], "source": os.path.relpath(path, REPO)}
        return None

    def roof_of(kind, v):
        per_launch_ms = v["ms"] / v["launches"]
        rate = v["work"] / (v["ms"] * 1e-3)
        pmode = enc.resolved_projection_mode() if hasattr(enc, "resolved_projection_mode") else getattr(enc, "projection_mode", "fp32")
        if kind == "proj" and pmode != "fp32":
            # the projections run as 6 bf16 MFMA products per fp32 product (exact 3-way operand split; "bf16x6-pq3": 6 for h,
            # 3 for P and Q = 4 on average): price the EXECUTED bf16 flops against the dense bf16 peak, and quote the
            # fp32-equivalent rate
            nprod = {"bf16x6": 6.0, "bf16x6-pq3": 4.0, "pq-bf16": 4.0, "pq-fp8": 4.0, "pq-bf16-x1": 8.0 / 3.0, "fp16x3": 3.0}[pmode]
            if hasattr(enc, "gemm_format") and enc.gemm_format() == 1:          # two fp16 pieces: three products whatever the mode
                nprod = 3.0
            return {"kernel": "proj (gemm_bf16x6s_kernel)", "bound": "mfma", "achieved": nprod * rate / 1e12,
                    "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": nprod * rate / 1e12 / MFMA_BF16_PEAK_TFLOPS,
                    "traffic": pmc_traffic(kind),
                    "mfma_dtype": ("fp16 (2-way split of f32, f32 accumulate; products per fp32 product: %s)" if pmode == "fp16x3" else
                                   "bf16 (3-way split of f32, f32 accumulate; products per fp32 product: %s)")
                                  % {"bf16x6": "6", "bf16x6-pq3": "6 for h, 3 for P and Q", "pq-bf16": "6 for h, 3 for P and Q", "pq-fp8": "6 for h, 3 for P and Q",
                                     "pq-bf16-x1": "6 for h, 1 for P and Q (user graph, layers >= 1)",
                                     "fp16x3": "3 (two fp16 pieces per operand)"}[pmode],
                    # the same launches priced by their ALGORITHMIC flops (2 M N K of the fp32 product) against the fp32 matrix-core
                    # peak, i.e. against the best an fp32-MFMA kernel of the same product could do
                    "fp32_equivalent_tflops": rate / 1e12, "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS,
                    "fp32_equivalent_frac_of_fp32_mfma_peak": rate / 1e12 / MFMA_F32_PEAK_TFLOPS,
                    "algorithmic_flops_per_launch": v["work"] / v["launches"],
                    "executed_flops_per_launch": nprod * v["work"] / v["launches"],
                    "peak_note": "nominal dense bf16 / fp16 peak (2.4 GHz); on random operands the chip holds about 1.9-2.0 GHz "
                                 "(MI355X_MICROARCH.md), i.e. about 2.0 PFLOP/s",
                    "avg_launch_ms": per_launch_ms, "launches": v["launches"]}
        if kind in ("proj", "linear"):
            return {"kernel": kind, "bound": "mfma", "achieved": rate / 1e12, "peak": MFMA_F32_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": rate / 1e12 / MFMA_F32_PEAK_TFLOPS, "traffic": pmc_traffic(kind),
                    "mfma_dtype": "f32", "algorithmic_flops_per_launch": v["work"] / v["launches"],
                    "avg_launch_ms": per_launch_ms, "launches": v["launches"]}
        return {"kernel": kind, "bound": "hbm", "achieved": rate / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": rate / 1e9 / HBM_PEAK_GBS, "traffic": pmc_traffic(kind),
                "algorithmic_bytes_per_launch": v["work"] / v["launches"], "avg_launch_ms": per_launch_ms,
                "launches": v["launches"]}

    def roof(kind):
        """`frac` / `achieved` / `avg_launch_ms` are the SOLO figures (round 6): the kind's launches on a single stream
        (the untimed profiling pass): the only figure a kernel-trace of the same command reproduces.  The durations of the same
        launches INSIDE the timed region, where three passes share the chip, are kept as `*_overlapped`: they measure sharing
        (more passes in flight = higher throughput and LONGER individual launches), not the kernel."""
        out = roof_of(kind, kinds[kind])
        iso = prof_iso.get(kind)
        if iso and iso["launches"] > 0:
            o2 = roof_of(kind, iso)
            out["frac_overlapped"], out["achieved_overlapped"], out["avg_launch_ms_overlapped"] = out["frac"], out["achieved"], out["avg_launch_ms"]
            out["frac"], out["achieved"], out["avg_launch_ms"] = o2["frac"], o2["achieved"], o2["avg_launch_ms"]
            out["isolated_achieved"], out["isolated_frac"] = o2["achieved"], o2["frac"]          # the names of rounds 3-5, same values as frac / achieved
            if "fp32_equivalent_tflops" in o2:
                out["fp32_equivalent_tflops_overlapped"] = out.get("fp32_equivalent_tflops")
                out["fp32_equivalent_tflops"] = o2["fp32_equivalent_tflops"]
                out["isolated_fp32_equivalent_tflops"] = o2["fp32_equivalent_tflops"]
                out["fp32_equivalent_frac_of_fp32_mfma_peak"] = o2["fp32_equivalent_frac_of_fp32_mfma_peak"]
            out["isolated_avg_launch_ms"] = o2["avg_launch_ms"]
            out["note"] = ("frac / achieved / avg_launch_ms: the kind's launches on a single stream (solo; reproducible from profiles/*_solo_kernels.txt); "
                           "*_overlapped: the same launches inside the timed region with three passes in flight — a launch's duration there "
                           "includes the time it shares the chip: a measure of sharing, not of the kernel")
        return out

    rx = None
    if "xattn" in kinds:
        rx = roof("xattn")
        rx["bytes_note"] = ("bytes that must cross HBM once (each distinct row once): layers >= 1 of the user graph: live centres x "
                            "(5 d 4 + n), counted on the device; layer 0 of grouped rows: live nodes of a GROUP x (4 d 4 + n) + live "
                            "(row, centre) x d 4 (output) + K3 per row; the news graph's fused launch at SURVEY 8d's bytes_B; "
                            "launches = user-graph and news-graph Eq. 8 kernels together, `parts` = per kernel")
        # the three Eq. 8 kernels apart (digat_profile_xattn_parts): algorithmic bytes, launch time in the timed region and alone,
        # and the counter bytes of the same kernel from the newest profiles/*_pmc.json
        part_symbol = {"twin": "xattn_sparse_twin", "l0": "xattn_sparse_l0", "news": "xattn_small_lds"}
        parts = {}
        for name, v in kinds["xattn"].get("parts", {}).items():
            if v["launches"] <= 0 or v["ms"] <= 0:
                continue
            e = {"algorithmic_bytes_per_launch": v["work"] / v["launches"], "launches": v["launches"],
                 "avg_launch_us": 1e3 * v["ms"] / v["launches"], "achieved": v["work"] / (v["ms"] * 1e-3) / 1e9,
                 "frac": v["work"] / (v["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
            vi = (prof_iso.get("xattn") or {}).get("parts", {}).get(name)
            if vi and vi["launches"] > 0 and vi["ms"] > 0:
                e["isolated_avg_launch_us"] = 1e3 * vi["ms"] / vi["launches"]
                e["isolated_achieved"] = vi["work"] / (vi["ms"] * 1e-3) / 1e9
                e["isolated_frac"] = e["isolated_achieved"] / HBM_PEAK_GBS
                e["isolated_algorithmic_bytes_per_launch"] = vi["work"] / vi["launches"]
                # frac := the solo fraction (as in roof()); the in-region figures keep the *_overlapped names
                e["frac_overlapped"], e["achieved_overlapped"], e["avg_launch_us_overlapped"] = e["frac"], e["achieved"], e["avg_launch_us"]
                e["frac"], e["achieved"], e["avg_launch_us"] = e["isolated_frac"], e["isolated_achieved"], e["isolated_avg_launch_us"]
            if name in part_symbol:
                symbols["xattn/" + name] = part_symbol[name]
                t = pmc_traffic("xattn/" + name)
                if t:
                    e["traffic"] = t["bytes_per_launch"]
                    e["traffic_source"] = t["source"]
                    e["kernel"] = t["kernel"]
            parts[name] = e
        rx["parts"] = parts
        rx["unit_note"] = "achieved / isolated_achieved in GB/s against the 8 TB/s HBM peak; bytes per launch"
    # per-kind time per step with the batches overlapped as in the timed region: from the untimed all-kinds pass (the timed
    # region records proj and xattn only)
    if getattr(run, "prof_all", None):
        kernel_ms = {k: round(v["ms"] / max(1, run.all_steps), 4) for k, v in run.prof_all.items() if v["launches"] > 0}
    else:
        kernel_ms = {k: round(v["ms"] / max(1, run.profiled_steps), 4) for k, v in kinds.items()}
    iso = {k: round(v["ms"] / max(1, run.iso_steps), 4) for k, v in prof_iso.items() if v["launches"] > 0}
    return roof(dom), rx, kernel_ms, iso


def roofline_step(W, run, ms_per_step):
    """The whole step against the chip: executed matrix-core flops and compulsory HBM bytes of ONE step — every launch of the
    untimed all-kinds pass (same streams, same batches in flight as the timed region) — each divided by its peak; the larger of
    the two times is the floor of a step that overlapped everything perfectly, and frac = floor / measured ms_per_step."""
    prof = getattr(run, "prof_all", None)
    if not prof or not run.all_steps:
        return None
    enc = W.model.graph_encoder
    f16 = hasattr(enc, "gemm_format") and enc.gemm_format() == 1
    pm = enc.resolved_projection_mode() if hasattr(enc, "resolved_projection_mode") else "fp32"
    nprod_proj = 3.0 if f16 else {"bf16x6": 6.0, "bf16x6-pq3": 4.0, "pq-bf16": 4.0, "pq-fp8": 4.0, "pq-bf16-x1": 8.0 / 3.0}.get(pm, 6.0)
    nprod_lin = 3.0 if f16 else 6.0
    steps = float(run.all_steps)
    flops_alg = (prof["proj"]["work"] + prof["linear"]["work"]) / steps
    flops_exec = (nprod_proj * prof["proj"]["work"] + nprod_lin * prof["linear"]["work"]) / steps
    if pm == "fp32":
        flops_exec, mfma_peak = flops_alg, MFMA_F32_PEAK_TFLOPS
    else:
        mfma_peak = MFMA_BF16_PEAK_TFLOPS
    gemm_bytes = (prof["proj"]["gemm_bytes"] + prof["linear"]["gemm_bytes"]) / steps
    other_bytes = sum(prof[k]["work"] for k in ("xattn", "pool", "topic", "glue", "agg")) / steps
    t_mfma = flops_exec / (mfma_peak * 1e12) * 1e3
    t_hbm = (gemm_bytes + other_bytes) / (HBM_PEAK_GBS * 1e9) * 1e3
    floor = max(t_mfma, t_hbm)
    return {"executed_mfma_flops_per_step": flops_exec, "algorithmic_flops_per_step": flops_alg, "mfma_peak_tflops": mfma_peak,
            "mfma_floor_ms": t_mfma, "compulsory_hbm_bytes_per_step": gemm_bytes + other_bytes,
            "hbm_bytes_of_the_gemms": gemm_bytes, "hbm_bytes_of_eq8_pooling_glue": other_bytes, "hbm_peak_gbs": HBM_PEAK_GBS,
            "hbm_floor_ms": t_hbm, "bound": "hbm" if t_hbm >= t_mfma else "mfma", "floor_ms": floor, "ms_per_step": ms_per_step,
            "frac": floor / ms_per_step if ms_per_step > 0 else None,
            "note": "floor = max(executed matrix-core flops / dense 16-bit peak, compulsory HBM bytes / 8 TB/s) of one step; GEMM bytes = "
                    "operand rows in + result rows out (+ epilogue row operands), weights not counted (L2-resident); Eq. 8 / pooling / glue "
                    "bytes as in roofline_xattn; the guide's achievable HBM rate (6.3 TB/s) would raise hbm_floor_ms by 1.27x"}


def cpu_baseline_and_auc(W, args, cpu_rows, cpu_seconds, report_baseline):
    """The oracle (unfused reference algorithm, torch-CPU fp32) on whole impressions of the same dev rows: the reported,
    non-target CPU baseline, and the scores the GPU path is held to (AUC / MRR / nDCG within 1e-4)."""
    from oracle import digat_oracle as O      # the checker / baseline, never the product
    from digat_amd import evaluate, util
    corpus, state, d, H, L = W.corpus, W.state, W.d, W.H, W.L
    imp_np = corpus.row_impression
    cores = usable_cores()
    torch.set_num_threads(cores)
    p = O.as_params(state)
    emb = torch.from_numpy(corpus.news_embedding)
    imp_starts = np.r_[0, np.flatnonzero(np.diff(imp_np)) + 1, corpus.rows]
    # the news the sample touches (candidates only need their own SAG rows): c_n0 for those, not for 65 k news
    need = max(cpu_rows, 64 + 300)         # the first oracle call is made whatever the bound (<= 64 rows or one impression)
    last = int(imp_starts[min(len(imp_starts) - 1, np.searchsorted(imp_starts, need, side="right"))])
    cand_all = np.unique(corpus.row_candidate[:max(last, 1)].astype(np.int64))
    remap = np.zeros(corpus.news_node_ID.shape[0], dtype=np.int64)
    remap[cand_all] = np.arange(len(cand_all))
    ids = torch.from_numpy(corpus.news_node_ID[cand_all].astype(np.int64))
    sa = emb.index_select(0, ids.flatten()).view(ids.shape[0], -1, d)
    masks, graphs = torch.from_numpy(corpus.news_graph_mask[cand_all]), torch.from_numpy(corpus.news_graph[cand_all])
    with torch.no_grad():
        c_n0 = O.news_graph_context(p, sa, masks)        # the per-news cache is setup on both sides (util.py:37-44): untimed
        cpu_scores, n_rows, n_imps = [], 0, 0
        t1 = time.perf_counter()
        while n_imps + 1 < len(imp_starts):
            s = int(imp_starts[n_imps])
            # batch a few impressions together: up to 64 rows per oracle call
            k = n_imps + 1
            while k + 1 < len(imp_starts) and int(imp_starts[k + 1]) - s <= 64:
                k += 1
            e = int(imp_starts[k])
            if (e > cpu_rows and n_rows > 0) or e > last:
                break
            imp = torch.from_numpy(corpus.row_impression[s:e])
            cand = torch.from_numpy(remap[corpus.row_candidate[s:e].astype(np.int64)])
            hist = torch.from_numpy(corpus.history.astype(np.int64)).index_select(0, imp)
            ue = emb.index_select(0, hist.flatten()).view(e - s, H, d)
            cpu_scores.append(O.row_logits(
                p, L, ue, torch.from_numpy(corpus.user_graph).index_select(0, imp),
                torch.from_numpy(corpus.user_category_mask).index_select(0, imp),
                torch.from_numpy(corpus.user_category_indices).index_select(0, imp),
                sa.index_select(0, cand), graphs.index_select(0, cand), masks.index_select(0, cand),
                c_n0.index_select(0, cand)))
            n_rows, n_imps = e, k
            if time.perf_counter() - t1 > cpu_seconds:
                break
        cpu_s = time.perf_counter() - t1
    cpu_scores = torch.cat(cpu_scores).numpy()
    baseline = None
    if report_baseline:
        baseline = {"value": (n_rows / W.mean_cand) / cpu_s, "unit": "impressions/s", "cores": cores,
                    "kind": "port", "rows_per_s": n_rows / cpu_s,
                    "sample": f"first {n_rows} rows ({n_imps} whole impressions) of the same synthetic dev set, "
                              f"unfused reference algorithm (oracle/digat_oracle.py, torch-CPU fp32, B=64 batches), "
                              f"{cpu_s:.1f}s"}
    gpu_scores = util.score_rows(W.model, W.dc, 0, n_rows, args.batch).cpu().numpy()
    lab, ri = corpus.row_label[:n_rows], corpus.row_impression[:n_rows]
    mg = evaluate.scoring(lab, evaluate.impression_ranks(gpu_scores, ri), ri)
    mc = evaluate.scoring(lab, evaluate.impression_ranks(cpu_scores, ri), ri)
    auc_match = {"max_abs_metric_diff": float(np.max(np.abs(np.array(mg) - np.array(mc)))),
                 "max_abs_score_diff": float(np.max(np.abs(gpu_scores - cpu_scores))),
                 "gpu": [round(v, 6) for v in mg], "cpu": [round(v, 6) for v in mc], "rows": int(n_rows), "impressions": int(n_imps),
                 "metrics": ["AUC", "MRR", "nDCG@5", "nDCG@10"], "tolerance": 1e-4}
    return baseline, auc_match, (cpu_scores, n_rows)


def auc_match_trained(args, D, projection=None):
    """"AUC-matched" on a model that ranks: the trained weights of tests/golden/trained_planted_state.npz on the held-out dev split
    of the planted-signal corpus (2 000 impressions, ~74 k rows), scored through this library, against the scores / metrics the
    IMPORTED REFERENCE produced for the same inputs in the build container (tests/golden/devset_trained_2k.npz: AUC 0.644, logits
    of rms ~10).  No oracle is involved: the fixture is the reference's own output."""
    from digat_amd import evaluate, synthetic, util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    golden = os.path.join(REPO, "tests", "golden")
    try:
        fx = {k: v for k, v in np.load(os.path.join(golden, "devset_trained_2k.npz")).items()}
        state = {k: v for k, v in np.load(os.path.join(golden, "trained_planted_state.npz")).items()}
    except OSError:
        return None
    full = synthetic.make_corpus(synthetic.SynthSpec(**synthetic.PLANTED_SPEC))
    corpus = synthetic.slice_impressions(full, 0, synthetic.PLANTED_DEV_IMPRESSIONS)
    spec = corpus.spec
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=int(fx["depth"]),
                                dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(D.dev).eval()
    model.graph_encoder.projection_mode = projection or args.projection
    dc = util.DeviceCorpus.from_numpy(corpus, D.dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores, metrics = util.compute_scores(model, dc, args.batch, labels=corpus.row_label)
    secs = time.perf_counter() - t0
    ref = fx["scores"].astype(np.float64)
    ranks = np.asarray(evaluate.impression_ranks(scores, corpus.row_impression))
    return {"max_abs_metric_diff": float(np.max(np.abs(np.array(metrics) - fx["metrics"]))),
            "gpu": [round(float(v), 6) for v in metrics], "reference": [round(float(v), 6) for v in fx["metrics"]],
            "metrics": ["AUC", "MRR", "nDCG@5", "nDCG@10"], "tolerance": 1e-4,
            "max_abs_score_diff": float(np.max(np.abs(scores - ref))), "score_rms": float(np.sqrt((ref ** 2).mean())),
            "ranks_equal_fraction": float((ranks == fx["ranks"].astype(np.int64)).mean()),
            "rows": int(corpus.rows), "impressions": int(spec.impressions),
            "projection": model.graph_encoder.resolved_projection_mode(), "seconds_incl_setup": round(secs, 3),
            "what": "trained weights (tools/train_planted.py) on the planted-signal dev split vs the imported reference's own scores "
                    "(tests/golden/devset_trained_2k.npz)"}


def run_e2e(args, D):
    """The reference's dev run end to end at MIND-small dev scale (main.py:69-72 times exactly this: util.compute_scores from the
    title tokens to the metrics): MSA news encoder over all 65 238 titles (util.py:24-33), SA gather + c_n0 + layer-0 tables
    (:34-44), every batch of the 73 152 impressions (~2.7 M rows, :51-69), per-impression ranking + AUC / MRR / nDCG on the
    device, the rank file (:70-84).  Synthetic titles and clicks, random-init MSA: a timing run — parity is auc_match's job.
    The reference prints ~600 s for this on an RTX 3090 with real MIND (README.md:64; context, not a target)."""
    import tempfile
    from digat_amd import evaluate, synthetic, util
    from digat_amd.model import Model
    wl = WORKLOADS["mind-small-default"]
    t_gen = time.perf_counter()
    spec = synthetic.SynthSpec(news_num=args.news or wl["news_num"], sag_neighbors=wl["sag_neighbors"], sag_hops=wl["sag_hops"],
                               category_num=wl["category_num"], impressions=args.e2e_impressions, seed=11)
    corpus = synthetic.make_corpus(spec)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=wl["depth"],
                                dropout_rate=wl["dropout"], vocabulary_size=30000, word_embedding_dim=300, max_title_length=32,
                                MSA_head_num=16, MSA_head_dim=25, attention_dim=256)
    torch.manual_seed(0)
    model = Model(cfg)
    model.news_encoder.initialize()
    with torch.no_grad():
        model.news_encoder.word_embedding.weight.mul_(0.1)          # GloVe-like magnitudes
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, wl["depth"], seed=0, bias_std=0.05)
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model = model.to(D.dev).eval()
    model.graph_encoder.projection_mode = args.projection
    model.graph_encoder.fused_user_context = bool(getattr(args, "fused_user_context", False))
    dc = util.DeviceCorpus.from_numpy(corpus, D.dev)
    text, mask = synthetic.make_titles(spec.news_num, cfg.max_title_length, cfg.vocabulary_size, seed=7)
    dc.title_text = torch.from_numpy(text).to(torch.int32).to(D.dev)
    dc.title_mask = torch.from_numpy(mask).to(D.dev)
    gen_s = time.perf_counter() - t_gen
    row_imp = corpus.row_impression

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()
    # a short untimed pass first: code objects, allocator pools, clocks (the reference's 600 s include none of its own start-up either)
    small = util.DeviceCorpus.from_numpy(synthetic.slice_impressions(corpus, 0, 256), D.dev)
    small.title_text, small.title_mask = dc.title_text, dc.title_mask
    util.compute_scores(model, small, REFERENCE_BATCH, labels=corpus.row_label[:small.rows])
    del small
    t0 = clock()
    dc.news_embedding = util.cache_news_representations(model.news_encoder, dc.title_text, dc.title_mask, 8192)      # util.py:24-33
    dc.news_key = tuple((p.data_ptr(), p._version) for p in model.news_encoder.parameters())
    t1 = clock()
    util.prepare_news_side(model.graph_encoder, dc, REFERENCE_BATCH)                                                 # :34-44
    t2 = clock()
    scores = util.score_rows(model, dc, 0, dc.rows, REFERENCE_BATCH, launch_rows=args.batch)                         # :51-69
    t3 = clock()
    ranks, metrics = evaluate.device_ranks_and_metrics(scores, row_imp, corpus.row_label)                            # :70-80, evaluate.py
    t4 = clock()
    with tempfile.NamedTemporaryFile("wb", suffix=".txt", delete=True) as f:                                         # :81-84
        f.write(evaluate.rank_file_bytes(ranks, row_imp))
        f.flush()
        rank_file_bytes = os.path.getsize(f.name)
    t5 = time.perf_counter()
    overflow = bool(model.graph_encoder.range_overflowed())
    total = t5 - t0
    return {"seconds": round(total, 3), "impressions": int(spec.impressions), "rows": int(corpus.rows), "news": int(spec.news_num),
            "impressions_per_s": spec.impressions / total, "rows_per_s": corpus.rows / total,
            "breakdown_s": {"news_encoder_msa_65k_titles": round(t1 - t0, 4), "prepare_news_side": round(t2 - t1, 4),
                            "score_all_batches": round(t3 - t2, 4), "rank_and_metrics_on_device": round(t4 - t3, 4),
                            "rank_file_on_host": round(t5 - t4, 4)},
            "reference_batches": (corpus.rows + REFERENCE_BATCH - 1) // REFERENCE_BATCH,
            "launch_sets": len(util.launch_batches(0, corpus.rows, REFERENCE_BATCH, args.batch)), "rows_per_launch_set": args.batch,
            "rank_file_bytes": int(rank_file_bytes),
            "metrics_random_clicks": [round(float(v), 4) for v in metrics], "fp16x3_range_overflow": overflow,
            "projection": model.graph_encoder.resolved_projection_mode(), "untimed_host_corpus_generation_s": round(gen_s, 1),
            "what": "util.compute_scores' flow from title tokens to the rank file at MIND-small dev scale, one GPU, synthetic data; the "
                    "reference prints ~600 s for it on an RTX 3090 with real MIND (README.md:64): context, not a target",
            "steady_state_rate_with_setup_folded_in_impressions_per_s": None}


PROJECTION_DTYPE = {
    "bf16x6": "f32 (matrix-core products of operands split into three bf16 pieces, six products, f32 accumulation)",
    "fp16x3": "f32 (matrix-core products of operands split into two fp16 pieces, three products, f32 accumulation; error against "
              "fp64 at or below an fp32 fma chain's: tests/test_hip_lowprec.py)",
}


def workload_config(W, args, D):
    enc = W.model.graph_encoder
    return {"workload": W.wl["label"], "projection": args.projection + ("" if args.projection != "auto" else " -> " + enc.resolved_projection_mode()),
            "projection_format": PROJECTION_DTYPE.get(enc.resolved_projection_mode(), enc.resolved_projection_mode()),
            "user_side": "per row" if args.per_row_users else "once per impression (row_group index)",
            "user_graph_eq8": enc.resolved_xattn_mode("user") + " (chosen from the corpus: mean adjacency entries per node)",
            "news_graph_eq8": ("small-graph kernel (n <= 16)" if W.N <= 16 else enc.resolved_xattn_mode("news")),
            "rows_per_step": args.batch, "reference_dev_batch_rows": REFERENCE_BATCH, "N": W.N, "U": W.H + W.C, "d": W.d, "graph_depth": W.L,
            "news_num": int(W.spec.news_num), "impressions_per_rank": int(W.spec.impressions), "rows_per_rank": int(W.corpus.rows),
            "device_table_bytes": W.table_bytes,
            "mean_candidates_per_impression": round(W.mean_cand, 3),
            "parallelism": f"dp{D.world} (row shards, no data-path collective"
                           + ("; one all_gather of the scores closes the timed region)" if D.world > 1 else ")"),
            # the collective backend of this run and the number of ranks it rendezvoused ("nccl" is RCCL on ROCm; "gloo" only
            # under the one-GPU test hook DIGAT_BENCH_TEST_SHARED_GPU)
            "backend": D.backend, "ranks_in_process_group": D.world_seen}


def _r(v, nd=4):
    """Rounded copy for the compact line (numbers only)."""
    if isinstance(v, float):
        return float(f"{v:.{nd}g}") if abs(v) < 1 else round(v, nd)
    return v


def compact_line(out):
    """The driver's line: the contract fields, the rooflines, the CPU baseline and the parity checks of the full document in <= 4 KB
    (the full document goes to bench_detail.json: round 4's 26 KB single line did not survive the driver's 8 KB stdout tail)."""
    def pick(dct, keys):
        return None if dct is None else {k: _r(dct[k]) for k in keys if k in dct and dct[k] is not None}
    cfg = out.get("config") or {}
    c = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                 "vs_baseline", "dtype", "data", "valid")}
    c["value"], c["ms_per_step"] = _r(c["value"], 2), _r(c["ms_per_step"], 4)
    c["config"] = {k: cfg[k] for k in ("workload", "projection", "rows_per_step", "N", "U", "d", "graph_depth", "news_num", "parallelism",
                                       "backend", "ranks_in_process_group") if k in cfg}
    roof = out.get("roofline")
    if roof:
        r = pick(roof, ("kernel", "bound", "achieved", "peak", "unit", "frac", "frac_overlapped", "achieved_overlapped", "avg_launch_ms",
                        "avg_launch_ms_overlapped", "launches"))
        r["frac_is"] = "solo: the kind's launches on a single stream; *_overlapped: inside the timed region, three passes sharing the chip"
        t = roof.get("traffic")
        r["traffic"] = None if not t else _r(float(t["bytes_per_launch"]), 0)
        if t:
            r["traffic_unit"] = ("HBM bytes per launch, 2*FETCH_SIZE+WRITE_SIZE (%s; factors 2.0 / 1.0 calibrated on known byte counts in this "
                                 "kernel's access shapes: profiles/r06_fetch_calib.json)" % t.get("source", "profiles/"))
        for k in ("algorithmic_flops_per_launch", "executed_flops_per_launch"):
            if k in roof:
                r[k] = _r(float(roof[k]), 0)
        c["roofline"] = r
    rx = out.get("roofline_xattn")
    if rx:
        x = pick(rx, ("bound", "achieved", "peak", "unit", "frac", "frac_overlapped", "achieved_overlapped"))
        x["parts"] = {}
        for name, e in (rx.get("parts") or {}).items():
            x["parts"][name] = {"us": _r(e["avg_launch_us"], 1), "frac": _r(e["frac"], 3),
                                "us_overlapped": _r(e.get("avg_launch_us_overlapped"), 1) if e.get("avg_launch_us_overlapped") else None,
                                "frac_overlapped": _r(e.get("frac_overlapped"), 3) if e.get("frac_overlapped") else None,
                                "alg_MB": _r(e.get("isolated_algorithmic_bytes_per_launch", e["algorithmic_bytes_per_launch"]) / 1e6, 1),
                                "pmc_MB": _r(e["traffic"] / 1e6, 1) if e.get("traffic") else None}
        c["roofline_xattn"] = x
    rs = out.get("roofline_step")
    if rs:
        c["roofline_step"] = pick(rs, ("frac", "floor_ms", "bound", "mfma_floor_ms", "hbm_floor_ms"))
    cb = out.get("cpu_baseline")
    c["cpu_baseline"] = None if cb is None else {**pick(cb, ("value", "unit", "cores", "kind")), "sample": cb["sample"][:150]}
    am, at = out.get("auc_match"), out.get("auc_match_trained")
    c["auc_match"] = pick(am, ("max_abs_metric_diff", "tolerance", "rows", "max_abs_score_diff"))
    c["auc_match_trained"] = pick(at, ("max_abs_metric_diff", "tolerance", "rows", "ranks_equal_fraction"))
    c["fp16x3_range_overflow"] = out.get("fp16x3_range_overflow")
    for k in ("per_rank_impressions_per_s", "scaling_efficiency", "all_gather_ms_by_rank", "devices", "rccl"):
        if out.get(k) is not None and out["n_gpus"] > 1:
            c[k] = out[k]
    if out.get("n1_same_workload"):
        c["n1_same_workload"] = pick(out["n1_same_workload"], ("value", "unit", "ms_per_step"))
    if out.get("configs4_inference"):
        c["configs4_inference"] = out["configs4_inference"]
    ex = out.get("extra_workloads")
    if ex:
        # one number per extra workload (impressions/s unless the key says otherwise) + its own oracle check where it has one
        cx = {}
        for k, v in ex.items():
            if "error" in v:
                cx[k] = "error"
                continue
            e = {"value": _r(v["value"], 1), "ms": _r(v.get("ms_per_step"), 3)}
            if v.get("unit") != "impressions/s":
                e["unit"] = v.get("unit")
            if v.get("auc_match"):
                e["auc_diff"] = _r(v["auc_match"]["max_abs_metric_diff"])
            if v.get("max_abs_metric_diff_vs_reference_trained_2k") is not None:
                e["drift_trained"] = _r(v["max_abs_metric_diff_vs_reference_trained_2k"])
            if "one_stream" in v:
                e["three_streams"] = _r(v["three_streams"]["value"], 1)
            for rk in ("roofline", "roofline_xattn", "roofline_step"):
                if isinstance(v.get(rk), dict) and v[rk].get("frac") is not None:
                    e[rk[9:] or "roof"] = _r(v[rk]["frac"], 3)
            cx[k] = e
        c["extra_workloads"] = cx
    if out.get("e2e"):
        c["e2e_seconds"] = out["e2e"]["seconds"]
    c["detail"] = out.get("detail_file")
    return c


def emit(out, args):
    """Write the full document to bench_detail.json (next to bench.py, and under gpurun_out/ when that directory exists) and print
    the compact line as the ONLY line on stdout.  Without --full the document is written only where --detail says."""
    paths = [os.path.join(REPO, "bench_detail.json")]
    if os.path.isdir(os.path.join(REPO, "gpurun_out")):
        paths.append(os.path.join(REPO, "gpurun_out", "bench_detail.json"))
    if getattr(args, "detail", None):
        paths = [args.detail]
    elif not args.full:
        paths = []
    written = None
    for path in paths:
        try:
            with open(path, "w") as f:
                json.dump(out, f)
                f.write("\n")
            written = written or path
        except OSError as exc:
            print(f"[bench] could not write {path}: {exc}", file=sys.stderr)
    out["detail_file"] = os.path.relpath(written, REPO) if written else None
    line = json.dumps(compact_line(out), separators=(",", ":"))
    if len(line) > 6000:          # the driver reads the tail of stdout: never let the line outgrow it again
        c = compact_line(out)
        c.pop("extra_workloads", None)
        line = json.dumps(c, separators=(",", ":"))
    print(line, flush=True)


def main():
    args = parse_args()
    if args.dump_outputs and args.mode != "infer":
        raise SystemExit("--dump-outputs: --mode infer only")
    D = Dist(args)
    name = args.workload if args.workload != "auto" else ("mind-small-default" if D.world == 1 else "mind-large-default")

    if args.mode == "train":
        W = build_workload(name, args, D, min(args.impressions, 4096), trainable=True)
        run = run_training(W, args, D, args.steps, args.warmup)
        elapsed = D.reduce([run.elapsed], "max")[0]
        rows = D.reduce([run.rows_done])[0]
        if D.rank == 0:
            print(json.dumps({
                "metric": "DIGAT training rows/sec (DDP step: forward, backward, gradient all-reduce, clip, Adam)",
                "value": rows / elapsed, "unit": "rows/s", "n_gpus": D.world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "f32" if args.train_precision == "fp32" else "bf16 matrix-core operands, f32 master weights / accumulation",
                "data": "synthetic",
                "config": {"workload": W.wl["label"].replace("dev inference", "training").replace("fp32 ", ""), "behaviours_per_rank_step": 64,
                           "candidates_per_behaviour": 5, "rows_per_rank_step": 320, "dropout": W.wl["dropout"],
                           "news_encoder": ("MSA on title text: %d titles x 32 tokens per rank and step" % (64 * (5 * W.N + W.H))
                                            if args.train_news_encoder == "msa" else "trainable table of news representations"),
                           "parallelism": f"ddp{D.world} (DistributedDataParallel, RCCL all-reduce of the gradients)"},
                "final_loss": run.loss,
                # the host's enqueue time per step (no synchronisation inside the loop): close to ms_per_step = this run was host-bound
                "host_enqueue_ms_per_step": run.enqueue_ms_per_step,
                # N > 1: the gradient all-reduce as DistributedDataParallel itself times it; N = 1: the step's MFMA launches against the peak
                "ddp_timers": run.ddp, "backend": D.backend, "ranks_in_process_group": D.world_seen,
                "roofline": run.roofline(elapsed / args.steps * 1e3) if run.roofline else None}))
        D.close()
        return

    if args.mode == "e2e":
        if D.world != 1:
            raise SystemExit("--mode e2e is a one-GPU run")
        e2e = run_e2e(args, D)
        print(json.dumps({"metric": "MIND-small dev run end to end (title tokens -> rank file), seconds", "value": e2e["seconds"], "unit": "s",
                          "n_gpus": 1, "steps": e2e["launch_sets"], "warmup": 0,
                          "ms_per_step": e2e["breakdown_s"]["score_all_batches"] / e2e["launch_sets"] * 1e3,
                          "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": WORKLOADS["mind-small-default"]["label"]}, "e2e": e2e}))
        D.close()
        return

    W = build_workload(name, args, D, args.impressions)
    from digat_amd import util as _util
    _util.freeze_host_heap()      # the synthetic corpus's host structures out of the garbage collector's walks (util.compute_scores does the same)
    run = run_inference(W, args, D, args.steps, args.warmup, with_profile=args.full, gather_scores=D.world > 1,
                        keep_last=bool(args.dump_outputs) and D.rank == 0)
    if run.last_scores is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "scores.npy"), run.last_scores)
    range_overflow = bool(W.model.graph_encoder.range_overflowed())
    elapsed = D.reduce([run.elapsed], "max")[0]
    rows_total, rows_all, imps_all = D.reduce([run.rows_done, W.corpus.rows, W.spec.impressions])
    mean_cand = rows_all / imps_all                       # candidates per impression over every rank's shard
    # every rank's own rate over its own clock (rows / its elapsed time): with no collective in the data path the job's rate
    # is their sum up to the slowest rank's tail; compare with the single-GPU rate of the SAME workload (the N = 1 line's
    # extra_workloads["mind-large-default"]) — the N = 1 headline is the MIND-small workload, BASELINE configs[1]
    per_rank = D.reduce([(run.rows_done / run.elapsed) if r == D.rank else 0.0 for r in range(D.world)])
    lanes_by_rank = D.reduce([float(run.batches_in_flight) if r == D.rank else 0.0 for r in range(D.world)])
    gather_ms_by_rank = D.reduce([float(run.all_gather_ms or 0.0) if r == D.rank else 0.0 for r in range(D.world)])
    devices = D.device_names()
    # N > 1 scores the MIND-large workload (BASELINE configs[3]) while the N = 1 headline is MIND-small (configs[1]): dividing one by
    # the other is not a scaling efficiency.  So the N > 1 line carries its OWN one-GPU reference: after the timed region rank 0
    # scores the same workload, same steps, alone (the other ranks wait at the fence below, their GPUs idle).
    n1_same = None
    if D.world > 1 and args.full:
        D.fence()
        if D.rank == 0:
            rs = run_inference(W, args, SoloView(D), args.steps, args.warmup, with_profile=False, gather_scores=False)
            n1_same = {"value": (rs.rows_done / W.mean_cand) / rs.elapsed, "unit": "impressions/s", "ms_per_step": rs.elapsed / args.steps * 1e3,
                       "steps": args.steps, "batches_in_flight": rs.batches_in_flight,
                       "what": "rank 0 alone on the same workload and shard, right after the timed region (other ranks idle at a barrier)"}
        D.fence()
    if D.rank != 0:
        D.close()
        return

    roof_dom = roof_x = kernel_ms = kernel_iso = None
    if args.full:
        roof_dom, roof_x, kernel_ms, kernel_iso = rooflines(W, run, args)
    cpu_baseline = auc_match = cpu_sample = None
    if args.full and args.cpu_rows > 0:
        # N = 1: the reported CPU baseline (~20 s) and the AUC match on its rows; N > 1: a short AUC match only
        rows = args.cpu_rows if D.world == 1 else min(args.cpu_rows, 384)
        secs = args.cpu_seconds if D.world == 1 else min(args.cpu_seconds, 6.0)
        cpu_baseline, auc_match, cpu_sample = cpu_baseline_and_auc(W, args, rows, secs, report_baseline=D.world == 1)
    trained = auc_match_trained(args, D) if args.full and args.cpu_rows > 0 else None
    matched = (auc_match is not None and auc_match["max_abs_metric_diff"] <= auc_match["tolerance"]
               and (trained is None or trained["max_abs_metric_diff"] <= trained["tolerance"]) and not range_overflow)

    extra = None
    if args.full and D.world == 1 and args.extra_steps > 0 and args.workload == "auto":
        # BASELINE configs[2] and the configs[3] shape, a few steps each, in the same invocation (same method, fewer steps)
        extra = {}
        if args.batch != REFERENCE_BATCH:
            # the headline's workload in the reference's own chunking: one launch set per 1024-row dev batch (main.py:42)
            import copy
            a1k = copy.copy(args)
            a1k.batch = REFERENCE_BATCH
            n1k = args.extra_steps * 10                    # 120 short steps by default: a 48-step sample scattered by 8 % run to run
            r1k = run_inference(W, a1k, D, n1k, 5, with_profile=False)
            extra["mind-small-default/reference-batch-1024"] = {
                "value": (r1k.rows_done / W.mean_cand) / r1k.elapsed, "unit": "impressions/s", "rows_per_s": r1k.rows_done / r1k.elapsed,
                "ms_per_step": r1k.elapsed / n1k * 1e3, "rows_per_step": REFERENCE_BATCH, "steps": n1k,
                "batches_in_flight": r1k.batches_in_flight,
                "what": "util.score_rows(..., launch_rows=1024): every reference dev batch its own pass through the encoder"}
        if True:
            # What INTEGRATION.md section 1's two-line swap delivers to the REFERENCE's own driver (util.py:51-69): Model.inference on
            # expanded per-row user tensors, one 1024-row dev batch per call, no grouping, no per-news layer-0 / query tables, one
            # stream — and the same calls issued over three alternating streams (a driver change of a few lines)
            import copy
            ad = copy.copy(args)
            ad.batch, ad.per_row_users = REFERENCE_BATCH, True
            nd = args.extra_steps * 6
            drop = {}
            for lanes, tag in ((1, "one_stream"), (3, "three_streams")):
                ad.lanes = lanes
                os.environ["DIGAT_BENCH_LANES"] = str(lanes)      # no lane tuning inside run_inference: the lane count IS the variant
                try:
                    rd = run_inference(W, ad, D, nd, 5, with_profile=False)
                finally:
                    del os.environ["DIGAT_BENCH_LANES"]
                drop[tag] = {"value": (rd.rows_done / W.mean_cand) / rd.elapsed, "ms_per_step": rd.elapsed / nd * 1e3,
                             "rows_per_s": rd.rows_done / rd.elapsed, "steps": nd}
            extra["mind-small-default/drop-in"] = {
                "value": drop["one_stream"]["value"], "unit": "impressions/s", "rows_per_step": REFERENCE_BATCH, **drop,
                "what": "the reference's driver loop unchanged except graphEncoders.DIGAT -> digat_amd.graphEncoders.DIGAT (INTEGRATION.md "
                        "section 1): Model.inference(expanded [1024, ...] user tensors, cached c_n0) per dev batch — digat_encoder_fwd, no "
                        "row_group, no per-news tables; inputs gathered on the device (the reference's DataLoader is host-side and not part "
                        "of this number)"}
        if args.projection in ("auto", "bf16x6") and cpu_sample is not None:
            # BASELINE configs[4], inference half: the same workload with P', Q of Eq. 8 stored in bf16 ("pq-bf16") and as
            # block-scaled e4m3 ("pq-fp8").  Drift is measured where "AUC-matched" means something — the trained model's 2 000
            # impressions against the imported reference's own metrics (tests/golden/devset_trained_2k.npz) — and, for reference,
            # on the random-click rows of the CPU sample against the fp32 oracle (41 impressions: a noisy yardstick)
            from digat_amd import evaluate, util
            cpu_scores, n_rows = cpu_sample
            lab, ri = W.corpus.row_label[:n_rows], W.corpus.row_impression[:n_rows]
            mc = evaluate.scoring(lab, evaluate.impression_ranks(cpu_scores, ri), ri)
            for pm_low, what in (("pq-bf16", "bf16"), ("pq-fp8", "block-scaled OCP e4m3 (one fp32 scale per row and 80-channel strip)")):
                W.model.graph_encoder.projection_mode = pm_low
                r4 = run_inference(W, args, D, args.extra_steps, 3, with_profile=False)
                sc = util.score_rows(W.model, W.dc, 0, n_rows, args.batch).cpu().numpy()
                mg = evaluate.scoring(lab, evaluate.impression_ranks(sc, ri), ri)
                tr4 = auc_match_trained(args, D, projection=pm_low)
                extra["mind-small-default/" + pm_low] = {
                    "value": (r4.rows_done / W.mean_cand) / r4.elapsed, "unit": "impressions/s", "rows_per_s": r4.rows_done / r4.elapsed,
                    "ms_per_step": r4.elapsed / args.extra_steps * 1e3, "steps": args.extra_steps, "batches_in_flight": r4.batches_in_flight,
                    "dtype": "f32 with P', Q of Eq. 8 (user graph, layers >= 1) stored as " + what,
                    "max_abs_metric_diff_vs_reference_trained_2k": None if tr4 is None else tr4["max_abs_metric_diff"],
                    "metric_diffs_vs_reference_trained_2k": None if tr4 is None else
                    [round(abs(a - b), 7) for a, b in zip(tr4["gpu"], tr4["reference"])],
                    "ranks_equal_fraction_trained_2k": None if tr4 is None else tr4["ranks_equal_fraction"],
                    "within_1e-4": None if tr4 is None else bool(tr4["max_abs_metric_diff"] <= 1e-4),
                    "max_abs_metric_diff_vs_fp32_oracle_random_clicks": float(np.max(np.abs(np.array(mg) - np.array(mc)))),
                    "mean_rel_score_diff_vs_fp32_oracle": float(np.mean(np.abs(sc - cpu_scores) / (np.abs(cpu_scores) + 1e-3))),
                    "rows_compared_random_clicks": int(n_rows),
                    "projection_gemm_result_bytes_per_row": {"pq-bf16": 4 * W.d + 2 * 2 * W.d, "pq-fp8": 4 * W.d + 2 * 448}[pm_low] if W.d == 400 else None}
            # the same workload under the OTHER operand format of the matrix-core GEMMs: "bf16x6" (three bf16 pieces, six products, no
            # range limit) when the headline ran "fp16x3" (two fp16 pieces, three products; what "auto" picks for weights below 32)
            W.model.graph_encoder.projection_mode = args.projection
            other_pm = "bf16x6" if W.model.graph_encoder.resolved_projection_mode() == "fp16x3" else "fp16x3"
            W.model.graph_encoder.projection_mode = other_pm
            util.prepare_news_side(W.model.graph_encoder, W.dc, args.batch)
            r5 = run_inference(W, args, D, args.extra_steps, 3, with_profile=False)
            sc = util.score_rows(W.model, W.dc, 0, n_rows, args.batch).cpu().numpy()
            mg = evaluate.scoring(lab, evaluate.impression_ranks(sc, ri), ri)
            extra["mind-small-default/" + other_pm] = {
                "value": (r5.rows_done / W.mean_cand) / r5.elapsed, "unit": "impressions/s", "rows_per_s": r5.rows_done / r5.elapsed,
                "ms_per_step": r5.elapsed / args.extra_steps * 1e3, "steps": args.extra_steps, "batches_in_flight": r5.batches_in_flight,
                "dtype": PROJECTION_DTYPE[other_pm],
                "max_abs_metric_diff_vs_fp32_oracle": float(np.max(np.abs(np.array(mg) - np.array(mc)))),
                "mean_rel_score_diff_vs_fp32_oracle": float(np.mean(np.abs(sc - cpu_scores) / (np.abs(cpu_scores) + 1e-3))),
                "rows_compared": int(n_rows)}
            W.model.graph_encoder.projection_mode = args.projection
            util.prepare_news_side(W.model.graph_encoder, W.dc, args.batch)
        for other in ("mind-small-stress", "mind-large-default", "mind-small-heavy-history"):
            W2 = build_workload(other, args, D, 4096)
            r2 = run_inference(W2, args, D, args.extra_steps, 3, with_profile=True)
            roof2, roofx2, kms2, kiso2 = rooflines(W2, r2, args)
            extra[other] = {"value": (r2.rows_done / W2.mean_cand) / r2.elapsed, "unit": "impressions/s",
                            "rows_per_s": r2.rows_done / r2.elapsed, "ms_per_step": r2.elapsed / args.extra_steps * 1e3,
                            "steps": args.extra_steps, "batches_in_flight": r2.batches_in_flight, "setup_ms": round(W2.setup_ms, 1),
                            "roofline": roof2, "roofline_xattn": roofx2, "roofline_step": roofline_step(W2, r2, r2.elapsed / args.extra_steps * 1e3),
                            "kernel_ms_per_step": kms2,
                            "kernel_ms_per_step_single_stream": kiso2, "live_row_fraction": r2.live_fraction,
                            "config": workload_config(W2, args, D)}
            if other != "mind-small-heavy-history" and args.cpu_rows > 0:
                # configs[2] / configs[3]: news graphs of 65 / 26 nodes take layer 0 from the per-news table through the sparse kernel's
                # group indirection — hold this workload's scores to the fp32 oracle too (a few whole impressions, <= 384 rows)
                _, am2, _ = cpu_baseline_and_auc(W2, args, min(args.cpu_rows, 384), min(args.cpu_seconds, 12.0), report_baseline=False)
                extra[other]["auc_match"] = am2
                extra[other]["news_layer0_table_in_place"] = W2.dc.news_hpq0 is not None
            if other == "mind-small-heavy-history":
                # the adjacency regime decides the Eq. 8 variant: say which one ran, time the other one too, and hold the scores of a
                # ~1 500-row sample to the fp32 oracle (the same criterion as the headline's auc_match)
                enc2 = W2.model.graph_encoder
                ug = W2.corpus.user_graph
                extra[other]["adjacency_entries_per_node"] = round(float(ug.sum()) / (ug.shape[0] * ug.shape[1]), 2)
                chosen = enc2.resolved_xattn_mode("user")
                alt = "dense" if chosen == "sparse" else "sparse"
                enc2.user_xattn_mode = alt
                r2b = run_inference(W2, args, D, args.extra_steps, 3, with_profile=False)
                enc2.user_xattn_mode = "auto"
                extra[other]["user_graph_eq8_variants"] = {chosen + " (chosen)": round(r2.elapsed / args.extra_steps * 1e3, 4),
                                                           alt: round(r2b.elapsed / args.extra_steps * 1e3, 4), "unit": "ms per step"}
                if args.cpu_rows > 0:
                    _, am2, _ = cpu_baseline_and_auc(W2, args, min(args.cpu_rows, 1536), min(args.cpu_seconds, 20.0), report_baseline=False)
                    extra[other]["auc_match"] = am2
            del W2, r2
            torch.cuda.empty_cache()
        # the DDP training step of the same shapes (trainer.py:71-105): forward, backward, clip, Adam — `bench.py --mode train` as a CHILD
        # process (the step is ~560 small launches and sits close to being host-bound: inside this process, after the workloads above,
        # it measured anywhere between 7.3 and 16 ms on the same kernels; a fresh process is what a training run is)
        try:
            import subprocess
            nt = max(4, args.extra_steps)
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", "train", "--steps", str(nt), "--warmup", "2", "--impressions", "4096",
                   "--train-precision", args.train_precision]
            if args.news:
                cmd += ["--news", str(args.news)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            tl = json.loads([l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1])
            extra["mind-small-default/train-step"] = {"value": tl["value"], "unit": "rows/s", "ms_per_step": tl["ms_per_step"],
                                                      "rows_per_step": 320, "steps": nt, "final_loss": tl["final_loss"],
                                                      "dtype": "f32 (bf16x6 matrix-core products, f32 accumulation)",
                                                      "what": "64 behaviours x (1 + 4) candidates, graph encoder + trainable news table, dropout 0.2; "
                                                              "timed in a child process (`bench.py --mode train`)",
                                                      "roofline": tl.get("roofline")}
        except Exception as exc:          # the headline must not depend on the training leg
            extra["mind-small-default/train-step"] = {"error": repr(exc)}

    e2e = None
    if args.full and D.world == 1 and args.e2e_impressions > 0 and args.workload == "auto" and args.extra_steps > 0:
        del W.dc.news_hpq0, W.dc.SA_news_representations           # 4 GB of the headline workload's tables: the e2e run builds its own
        W.dc.news_hpq0 = W.dc.SA_news_representations = None
        torch.cuda.empty_cache()
        e2e = run_e2e(args, D)
        # the steady-state rate of the headline with the once-per-run setup (news encoder + per-news tables) folded in, over a
        # MIND-small dev run: what a whole dev run sustains, next to `value` (the step alone)
        step_s = elapsed / args.steps
        nb = MIND_SMALL_DEV_ROWS / args.batch
        setup_s = e2e["breakdown_s"]["news_encoder_msa_65k_titles"] + e2e["breakdown_s"]["prepare_news_side"]
        e2e["steady_state_rate_with_setup_folded_in_impressions_per_s"] = MIND_SMALL_DEV_IMPRESSIONS / (nb * step_s + setup_s)

    # BASELINE configs[4], inference half, decided from the two extras above: the reduced-precision setting that stays within the
    # reference's 1e-4 on the trained, reference-pinned dev set, and what the fp8 storage costs
    configs4 = None
    if extra and "mind-small-default/pq-bf16" in extra and "mind-small-default/pq-fp8" in extra:
        b16, f8 = extra["mind-small-default/pq-bf16"], extra["mind-small-default/pq-fp8"]
        def verdict(v):
            dr = v["max_abs_metric_diff_vs_reference_trained_2k"]
            return "not measured" if dr is None else ("%.1e (%s 1e-4)" % (dr, "within" if dr <= 1e-4 else "OVER"))
        configs4 = ("pq-bf16: drift %s, %.0f imp/s; pq-fp8 (block-scaled e4m3 storage of P', Q; no fp8 MFMA: the operands feed a relu, not "
                    "a product): drift %s, %.0f imp/s, opt-in" % (verdict(b16), b16["value"], verdict(f8), f8["value"]))
    nb_corpus = max(1, W.corpus.rows // args.batch)
    out = {
        "metric": "MIND dev impressions scored/sec (AUC-matched)" if matched else
                  "MIND dev impressions scored/sec" + (" (AUC match FAILED)" if auc_match is not None else " (AUC match not run)"),
        "value": (rows_total / mean_cand) / elapsed,
        "unit": "impressions/s",
        "n_gpus": D.world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        # fp32 data and fp32-grade arithmetic; how the >= 2048-row GEMMs form their fp32 products on the matrix cores is
        # config.projection / config.projection_format
        "dtype": ("f32 with P', Q of the user graph's Eq. 8 as block-scaled e4m3 (configs[4])" if args.projection == "pq-fp8" else
                  "f32" if not args.projection.startswith("pq-bf16") else "f32 with P', Q of the user graph's Eq. 8 in bf16 (configs[4])"),
        "data": "synthetic",
        "valid": bool(matched or auc_match is None),
        "config": workload_config(W, args, D),
        "rows_per_s": rows_total / elapsed,
        "batch_revisited_in_timed_region": bool(run.revisited),
        # consecutive batches alternate over this many HIP streams (util.batch_streams); chosen between 2 and 3 by a short
        # measurement before the warm-up unless DIGAT_BENCH_LANES says
        "batches_in_flight": run.batches_in_flight if D.world == 1 else [int(v) for v in lanes_by_rank],
        "per_rank_impressions_per_s": None if D.world == 1 else [round(v / mean_cand, 1) for v in per_rank],
        # N > 1 only: the one-GPU rate of THIS workload measured in this run, and value / (N x that); the closing all_gather of
        # the scores (inside the timed region) per rank; the devices the ranks ran on
        "n1_same_workload": n1_same,
        "scaling_efficiency": None if n1_same is None else ((rows_total / mean_cand) / elapsed) / (D.world * n1_same["value"]),
        "all_gather_ms_by_rank": None if D.world == 1 else [round(v, 3) for v in gather_ms_by_rank],
        "devices": devices,
        # prepare_news_side (SA gather, c_n0, the layer-0 tables): once per dev run and weight version, outside the timed region
        "setup_ms": round(W.setup_ms, 1),
        # untimed, before the warm-up: clocks out of idle (pre-warm) and the choice between two and three launch sets in flight
        "untimed_seconds_before_the_timed_region": run.untimed_s,
        "setup_ms_per_step_amortised": {"over_this_corpus": round(W.setup_ms / nb_corpus, 4),
                                        "over_mind_small_dev": round(W.setup_ms / (MIND_SMALL_DEV_ROWS / args.batch), 4)},
        "roofline": roof_dom,
        "roofline_xattn": roof_x,
        # the whole step against the chip: executed matrix-core flops and compulsory HBM bytes, each / peak, vs ms_per_step
        "roofline_step": roofline_step(W, run, elapsed / args.steps * 1e3) if args.full else None,
        "kernel_ms_per_step": kernel_ms,
        "kernel_ms_per_step_single_stream": kernel_iso,
        # rows projected / rows nominal over the row-list launches (user-graph layers >= 1 and featureAffine): the encoder
        # leaves out nodes and topic buckets that cannot reach its outputs; the proj roofline prices EXECUTED flops
        "live_row_fraction": run.live_fraction,
        "cpu_baseline": cpu_baseline,
        "auc_match": auc_match,
        # the same criterion on a model that RANKS (trained weights, planted-signal corpus), against the imported reference's scores
        "auc_match_trained": trained,
        "fp16x3_range_overflow": range_overflow,
        "configs4_inference": configs4,
        "rccl": D.rccl_summary(),
        "extra_workloads": extra,
        # the whole dev run of util.compute_scores at MIND-small dev scale, from title tokens to the rank file (seconds)
        "e2e": e2e,
    }
    emit(out, args)
    D.close()
    if (auc_match is not None or trained is not None) and not matched:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
