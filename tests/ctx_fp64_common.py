"""Shared by tests/test_ctx_fp64_cpu.py and tests/test_hip_ctx_fp64.py: the context stage (compute_news_graph_context,
compute_user_graph_context: csrc/digat_context.inc, csrc/digat_ctxfused.inc and the context part of csrc/digat_encoder.inc) — the
case lists both files run, the inputs of a case, the fp64 references and the comparison.  The CPU file pins the references to the
golden fixtures and to the oracle and holds fp32 arithmetic alone to a quarter (BLAS sums) / half (scores summed as one fp32 chain
over the channels) of the tolerance on the cases listed here; the GPU file holds the HIP kernels to the whole of it.

Blocks:
  A  attention pooling alone (digat_pool_fwd: launch_pool's eight attn_pool_resident_kernel<NPW, U> and attn_pool_kernel)
  B  topic pooling alone (digat_topic_pool_fwd / digat_topic_pool_lists_fwd: topic_pool_resident_kernel<13 | 16>, topic_pool_kernel)
  C  the per-function entries whole (digat_news_ctx_fwd, digat_user_ctx_fwd / _grouped) against the oracle on double parameters
  D  user_ctx_fused_kernel alone (digat_user_ctx_fused_fwd)

Inputs of the kernel-alone blocks (A, B, D): features N(0, 1) fp32; the folded query is given directly as gain x N(0, 1) — no
GEMM in front — so that the scores x . kq / sqrt(d) have a standard deviation of about the gain.  Two gains: 1 and 4 (near-uniform
attention hides score errors; from about 8 on fp32 itself leaves the tolerance).  Three cases take 2 in place of 4 (GAIN_DOWN): at
4 the scores summed as one fp32 chain over the channels alone spent more than the half of the tolerance the CPU file allows them —
0.589 (alpha, pooling n = 13, d = 800), 0.554 (pooling n = 128, d = 1024) and 0.521 (topic pooling H = 256, d = 512).  The
tolerance stays; the case's gain comes down.

The references evaluate one row at a time in torch, on the GPU when there is one (eq8_fp64_common.ref_device), in the dtype they are
asked for: fp64 is the reference, fp32 the CPU file's budget."""
import functools
import math
import zlib

import numpy as np
import torch

from eq8_fp64_common import ALPHA_TOL, close, ref_device       # noqa: F401  (re-exported)
from oracle import digat_oracle as O

OUT_TOL = dict(rtol=2e-5, atol=2e-5)            # context outputs: tests/test_hip_user_ctx0.py, tests/test_hip_train_primitives.py
FUSED_VS_LAUNCHES = dict(rtol=2e-6, atol=2e-6)  # tests/test_hip_parity.py: the one launch against the three it replaces
GAINS = (1.0, 4.0)
GAIN_DOWN = {("pool", 13, 800): 2.0, ("pool", 128, 1024): 2.0, ("topic", 256, 18, 512): 2.0}      # see the module docstring


def gains(*case):
    """The two gains of a case of block A ("pool", n, d) or B ("topic", H, C1, d)."""
    return GAINS[0], GAIN_DOWN.get(case, GAINS[1])
NAN = float("nan")
MAX_NODES = 128                                 # DIGAT_MAX_NODES


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _dev_f(t, dtype):
    return t.to(ref_device(), dtype)


# ---- the launchers' conditions, restated (test ids and two assertions of the CPU file only) ----------------------------------------
def route_pool(n, d):
    """launch_pool (csrc/digat_context.inc:146-173): d / 4 <= 128 and n <= 68 take attn_pool_resident_kernel<NPW, U> with U = 1 up to
    d / 4 = 64 (:154) and NPW = 3, 5, 7, 17 by n <= 12, 20, 28 (:155-158, :162-165); everything else attn_pool_kernel (:170)."""
    if d // 4 <= 128 and n <= 68:
        return f"resident<{3 if n <= 12 else 5 if n <= 20 else 7 if n <= 28 else 17},{1 if d // 4 <= 64 else 2}>"
    return "attn_pool_kernel"


def route_topic(H, C1, d):
    """launch_topic_args (csrc/digat_context.inc:452-474): (kernel, 16-row category tiles).  H <= 64 with H <= 52 or at most eight
    64-channel groups takes the resident kernel (:465), <13> up to H = 52 (:467), <16> beyond (:468); else topic_pool_kernel (:470)."""
    groups, ct = (d + 63) // 64, (C1 + 15) // 16
    if H <= 64 and (H <= 52 or groups <= 8):
        return ("resident<13>" if H <= 52 else "resident<16>"), ct
    return "topic_pool_kernel", ct


def fused_ok(H, C1, d):
    """ctxfused_ok (csrc/digat_ctxfused.inc:508-510)."""
    return 1 <= H <= 52 and C1 <= 20 and d % 8 == 0 and 192 < d <= 448


# ---- A: attention pooling ---------------------------------------------------------------------------------------------------------
# n: 1; 2; 4 | 5 one | two slots per wave; 11, 12 | 13 NPW 3 | 5; 18, 20 | 21 NPW 5 | 7; 26, 28 | 29 NPW 7 | 17; 63, 64 | 65 one | two
# mask ballots; 67, 68 | 69 resident | attn_pool_kernel; 82; 127, 128 the limit
POOL_N = (1, 2, 4, 5, 10, 11, 12, 13, 18, 20, 21, 26, 28, 29, 63, 64, 65, 67, 68, 69, 82, 127, 128)
# d: 4; 36 (d / 4 odd); 252 | 256 | 260 U = 1 | 2; 400; 512 | 516 resident | attn_pool_kernel; 800; 1024
POOL_D = (4, 36, 252, 256, 260, 400, 512, 516, 800, 1024)
POOL_N_ALL_D = (10, 12, 13, 20, 21, 28, 29, 68, 69, 128)
POOL_D_ALL_N = (36, 400)
POOL_SHAPES = sorted({(n, d) for n in POOL_N for d in POOL_D_ALL_N} | {(n, d) for n in POOL_N_ALL_D for d in POOL_D})
POOL_LD = ((12, 36), (20, 36), (28, 36), (68, 36), (12, 400), (20, 400), (28, 400), (68, 400))     # one per (NPW, U): ld_b = n d + 8, NaN in the gap
POOL_LD_PAD = 8


def pool_masks(n, g):
    """bool [B, n], B = 5 (6 for n > 64): every node unmasked; about 60 %; only node 0; only node n - 1; none (uniform weights);
    n > 64: only nodes >= 64."""
    some = torch.rand(n, generator=g) < 0.6
    some[int(torch.randint(n, (1,), generator=g))] = True
    rows = [torch.ones(n, dtype=torch.bool), some, torch.arange(n) == 0, torch.arange(n) == n - 1, torch.zeros(n, dtype=torch.bool)]
    if n > 64:
        high = (torch.rand(n, generator=g) < 0.5) & (torch.arange(n) >= 64)
        high[64 + int(torch.randint(n - 64, (1,), generator=g))] = True
        rows.append(high)
    return torch.stack(rows)


@functools.lru_cache(maxsize=8)
def pool_inputs(n, d, gain):
    """fp32 (feat [B, n, d], kq [B, d], mask bool [B, n], addend [B, d]).  Wherever a row has an unmasked node its masked nodes hold
    NaN: a masked node weighs exactly 0 and its row must not be read into any sum.  Cached: callers leave them unchanged."""
    g = _gen("pool", n, d, gain)
    mask = pool_masks(n, g)
    B = mask.shape[0]
    feat, kq, addend = torch.randn(B, n, d, generator=g), gain * torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    feat[(~mask) & mask.any(dim=1, keepdim=True)] = NAN
    return feat, kq, mask, addend


def _chain_scores(x, kq):
    """x [B, n, d] . kq [B, d] summed as ONE chain over the channels in x's dtype (a product, then an add, per channel)."""
    s = torch.zeros(x.shape[:2], dtype=x.dtype, device=x.device)
    for c in range(x.shape[2]):
        s = s + x[:, :, c] * kq[:, c:c + 1]
    return s


def pool_eval(feat, kq, mask, dtype=torch.float64, chain=False):
    """(out [B, d], alpha [B, n]) of ScaledDotProductAttention on a folded query (layers.py:199-206), row by row in ``dtype``: the
    scores of the unmasked nodes, softmax over them, the weighted sum of their rows; the mean of every row when none is unmasked.  Masked
    rows are not touched.  ``chain``: the scores summed as one chain over the channels instead of by torch's matmul."""
    B, n, d = feat.shape
    x_all, k_all, m_all = _dev_f(torch.nan_to_num(feat), dtype), _dev_f(kq, dtype), mask.to(ref_device()).bool()
    S = _chain_scores(x_all, k_all) if chain else None
    out, alpha = torch.zeros(B, d, dtype=dtype, device=x_all.device), torch.zeros(B, n, dtype=dtype, device=x_all.device)
    for b in range(B):
        if not bool(m_all[b].any()):                     # every score is -1e9: the weights are 1 / n whatever the scores were
            out[b], alpha[b] = x_all[b].mean(dim=0), 1.0 / n
            continue
        m = m_all[b]
        x = x_all[b][m]
        s = (S[b][m] if chain else x @ k_all[b]) / math.sqrt(d)
        a = torch.softmax(s, dim=0)
        out[b], alpha[b, m] = a @ x, a
    return out.cpu(), alpha.cpu()


# ---- B: topic pooling -------------------------------------------------------------------------------------------------------------
# H: 0 (no load is issued: every request of topic_pool_resident_kernel<13> sits behind s < nsteps = 0 or tid < H, csrc/digat_context.inc
# :356, :361, :364); 1; 3, 4 | 5 one | two MFMA steps; 48, 51, 52 | 53 resident<13> | <16>; 60, 61, 63, 64 step 15 | 65 resident |
# topic_pool_kernel; 100; 255, 256 the limit
TOPIC_H = (0, 1, 3, 4, 5, 48, 50, 51, 52, 53, 60, 61, 63, 64, 65, 100, 255, 256)
# C1: 1, 2, 6; 16 | 17, 32 | 33, 48 | 49 one .. four category tiles; 18 (MIND); 64 the limit
TOPIC_C1 = (1, 2, 6, 16, 17, 18, 32, 33, 48, 49, 64)
# d: 4; 36; 60 | 64 | 68 one | two waves; 400; 512 | 516 eight | nine waves (H = 53 .. 64: resident<16> | topic_pool_kernel); 800; 1024
TOPIC_D = (4, 36, 60, 64, 68, 400, 512, 516, 800, 1024)
TOPIC_H_ALL_D = (50, 52, 53, 64, 65, 256)
TOPIC_H_ALL_C1 = (52, 64, 256)
TOPIC_D_ELSE, TOPIC_C1_ELSE = (36, 400), 18
TOPIC_SHAPES = sorted({(H, TOPIC_C1_ELSE, d) for H in TOPIC_H for d in TOPIC_D_ELSE} | {(H, TOPIC_C1_ELSE, d) for H in TOPIC_H_ALL_D for d in TOPIC_D}
                      | {(H, C1, d) for H in TOPIC_H_ALL_C1 for C1 in TOPIC_C1 for d in TOPIC_D_ELSE})
TOPIC_EXTRA_NODES = 2          # U = H + 2: the topic rows behind the history hold NaN and are never read


def topic_rows(H, C1, g):
    """int64 [7, H]: a right-padded MIND-like history (the padding bucket C1 - 1 is a category like any other); every slot in one
    category; every category that fits read at least once (arange(H) % C1: every tile); sorted runs; a one-item history (the other
    indices out of range); indices out of range (-1 and C1 + 1, dropped) among valid ones; a category with exactly one member."""
    r = lambda: torch.randint(0, C1, (H,), generator=g)
    padded = r()
    padded[H - H // 3:] = C1 - 1
    one_item = torch.full((H,), -1, dtype=torch.int64)
    one_item[:1] = 2 % C1
    out_of_range = r()
    out_of_range[torch.arange(H) % 3 == 1] = -1
    out_of_range[torch.arange(H) % 3 == 2] = C1 + 1
    lone = torch.zeros(H, dtype=torch.int64)
    lone[H // 2:H // 2 + 1] = 1 % C1
    return torch.stack([padded, torch.full((H,), 3 % C1, dtype=torch.int64), torch.arange(H) % C1, torch.sort(r()).values, one_item, out_of_range, lone])


@functools.lru_cache(maxsize=8)
def topic_inputs(H, C1, d, gain):
    """fp32 (Xu [B, H + 2, d] with NaN in the two rows behind the history, kq [B, d], idx int64 [B, H]).  Cached."""
    g = _gen("topic", H, C1, d, gain)
    idx = topic_rows(H, C1, g)
    B = idx.shape[0]
    Xu, kq = torch.randn(B, H + TOPIC_EXTRA_NODES, d, generator=g), gain * torch.randn(B, d, generator=g)
    Xu[:, H:] = NAN
    return Xu, kq, idx


def topic_eval(x, kq, idx, C1, dtype=torch.float64, live=None, chain=False):
    """(T [B, C1, d], empty bool [B, C1]) of scatter_softmax + scatter_sum (graphEncoders.py:126-130) on a folded query, row by row
    in ``dtype``: a_t = x_t . kq / sqrt(d), softmax within the slots of equal category, the weighted sum per category; indices
    outside [0, C1) are dropped, an empty category is a zero row.  ``live`` (bool [B, H]): pools where(live, x, 0) — a dead slot
    scores 0, stays a member of its category and adds a zero row, whatever its row holds."""
    B, H, d = x.shape
    dev = ref_device()
    x_all = torch.nan_to_num(x) if live is None else torch.where(live.bool().unsqueeze(2), torch.nan_to_num(x), torch.zeros(()))
    x_all, k_all, idx = _dev_f(x_all, dtype), _dev_f(kq, dtype), idx.to(dev)
    S = _chain_scores(x_all, k_all) if chain else None
    cats = torch.arange(C1, device=dev).unsqueeze(1)
    T, empty = torch.zeros(B, C1, d, dtype=dtype, device=dev), torch.ones(B, C1, dtype=torch.bool, device=dev)
    for b in range(B):
        member = idx[b].unsqueeze(0) == cats                                                    # [C1, H]
        has = member.any(dim=1)
        s = (S[b] if chain else x_all[b] @ k_all[b]) / math.sqrt(d)
        a = torch.softmax(s.unsqueeze(0).expand(C1, H).masked_fill(~member, -float("inf")), dim=1)
        a = torch.where(member, a, torch.zeros((), dtype=dtype, device=dev))                     # an empty category: softmax of nothing
        T[b], empty[b] = a @ x_all[b], ~has
    return T.cpu(), empty.cpu()


TOPIC_LIST_ROWS = 8
TOPIC_LIVE_PAD = 3             # live_ld = H + 3


def topic_hlasts(H):
    """1 + the last live slot of the eight list rows: 0, 1, 4k - 1, 4k, 4k + 1 and H, then H and 4k + 1 again for the rows with dead
    slots among the live ones; 4k about H / 2."""
    k4 = 4 * max(1, H // 8)
    return [min(max(v, 0), H) for v in (0, 1, k4 - 1, k4, k4 + 1, H, H, k4 + 1)]


@functools.lru_cache(maxsize=8)
def topic_list_inputs(H, C1, d, gain):
    """The per-row list call: fp32 Xu [8, H + 2, d], kq, idx, live uint8 [8, H + 3] (the pad bytes are 0xEE), hlast int32 [8].  Row
    r is live below topic_hlasts(H)[r]; row 6 has one dead slot in the middle of live ones, row 7 random dead slots (never the last
    live one).  Dead rows and the rows behind the history hold NaN."""
    g = _gen("topic-lists", H, C1, d, gain)
    idx = torch.cat([topic_rows(H, C1, g), torch.randint(0, C1, (1, H), generator=g)])
    B = TOPIC_LIST_ROWS
    hl = topic_hlasts(H)
    live = torch.arange(H).unsqueeze(0) < torch.tensor(hl).unsqueeze(1)
    if hl[6] >= 3:
        live[6, hl[6] // 2] = False
    if hl[7] >= 2:
        live[7, :hl[7] - 1] &= torch.rand(hl[7] - 1, generator=g) < 0.7
    Xu, kq = torch.randn(B, H + TOPIC_EXTRA_NODES, d, generator=g), gain * torch.randn(B, d, generator=g)
    Xu[:, H:] = NAN
    Xu[:, :H][~live] = NAN
    flags = torch.full((B, H + TOPIC_LIVE_PAD), 0xEE, dtype=torch.uint8)
    flags[:, :H] = live.to(torch.uint8)
    return Xu, kq, idx, flags, torch.tensor(hl, dtype=torch.int32)


TOPIC_GROUP_OF_ROW = (1, 0, 1, 1, 0)            # two groups, not in contiguous runs


@functools.lru_cache(maxsize=8)
def topic_group_inputs(H, C1, d, gain):
    """The grouped list call: fp32 Xg [2, H + 2, d], row_group int32 [5], and per row kq, idx, live uint8 [5, H + 3], hlast.  The rows
    of a group share its nodes and therefore its flags: group 0 is live below 4k + 1 with a dead slot in the middle, group 1 is
    live throughout."""
    g = _gen("topic-groups", H, C1, d, gain)
    rg = torch.tensor(TOPIC_GROUP_OF_ROW, dtype=torch.int32)
    hl_g = [topic_hlasts(H)[4], H]
    live_g = torch.arange(H).unsqueeze(0) < torch.tensor(hl_g).unsqueeze(1)
    if hl_g[0] >= 3:
        live_g[0, hl_g[0] // 2] = False
    idx = topic_rows(H, C1, g)[[0, 2, 3, 5, 6]]
    Xg, kq = torch.randn(2, H + TOPIC_EXTRA_NODES, d, generator=g), gain * torch.randn(5, d, generator=g)
    Xg[:, H:] = NAN
    Xg[:, :H][~live_g] = NAN
    flags = torch.full((5, H + TOPIC_LIVE_PAD), 0xEE, dtype=torch.uint8)
    flags[:, :H] = live_g[rg.long()].to(torch.uint8)
    return Xg, rg, kq, idx, flags, torch.tensor(hl_g, dtype=torch.int32)[rg.long()].contiguous()


# ---- C: the per-function entries whole ------------------------------------------------------------------------------------------
NEWS_N, NEWS_D = (1, 10, 13, 26, 65, 69, 128), (36, 64, 400, 516)
NEWS_SHAPES = [(N, d) for N in NEWS_N for d in NEWS_D]
USER_H, USER_C1, USER_D = (5, 50, 53, 65), (6, 13, 18, 21, 29), (64, 400, 516)      # C + 1 = 6, 13 | 18 | 21 | 29: NPW 3 | 5 | 7 | 17 of the final pooling
USER_SHAPES = [(H, C1, d) for H in USER_H for C1 in USER_C1 for d in USER_D]
BIG_ROWS = 2048                # from this many GEMM rows on the entries take the tiled GEMM family
ROWS = 3                       # rows of a small call


@functools.lru_cache(maxsize=4)
def ctx_state(d, C):
    """DIGAT parameters at width d with C topics: a function of (d, C)."""
    from digat_amd import synthetic
    return synthetic.make_state_dict(d, C, 1, seed=5000 + 7 * d + C, bias_std=0.05)


def f64_params(state):
    return {k: torch.as_tensor(v).double() for k, v in state.items()}


@functools.lru_cache(maxsize=4)
def news_inputs(N, d):
    """fp32 (X [3, N, d], mask bool [3, N], addend [3, d]): every node unmasked; about 60 %; only node N - 1."""
    g = _gen("news", N, d)
    mask = pool_masks(N, g)[[0, 1, 3]]
    return torch.randn(ROWS, N, d, generator=g), mask, torch.randn(ROWS, d, generator=g)


def ctx0_users(H, C1, g):
    """(idx int64 [5, H], mask bool [5, C1]) — the users of tests/test_hip_user_ctx0.py:_case: reads every category it can, every
    bucket unmasked; an empty history (every index out of range) with some buckets unmasked; one item; two categories read of which
    one is masked, and an unread one unmasked; every bucket masked (uniform weights), on a right-padded history."""
    idx = torch.empty(5, H, dtype=torch.int64)
    idx[0] = torch.arange(H) % C1
    idx[1] = torch.tensor([C1 + 1, -1] * H)[:H]
    idx[2] = -1
    idx[2, 0] = 2
    idx[3] = torch.where(torch.rand(H, generator=g) < 0.5, 1, 3)
    idx[3, 0], idx[3, H - 1] = 1, 3
    idx[4] = torch.randint(0, C1, (H,), generator=g)
    idx[4, H // 2:] = C1 - 1
    mask = torch.zeros(5, C1, dtype=torch.bool)
    mask[0] = True
    mask[1, [0, 3]] = True
    mask[2, 2] = True
    mask[3, [3, 4]] = True
    return idx, mask


@functools.lru_cache(maxsize=4)
def user_inputs(H, C1, d):
    """fp32 (Xu [5, H + C1 - 1, d], mask bool [5, C1], idx int64 [5, H], c_n [5, d], addend [5, d]) of ctx0_users."""
    g = _gen("user", H, C1, d)
    idx, mask = ctx0_users(H, C1, g)
    return torch.randn(5, H + C1 - 1, d, generator=g), mask, idx, torch.randn(5, d, generator=g), torch.randn(5, d, generator=g)


USER_GROUP_OF_ROW = (3, 0, 4, 3, 1, 2, 0)       # seven rows over the five users as groups


def user_context(p, Xu, cat_mask, cat_idx, c_n, H):
    """oracle.user_graph_context in the dtype of its arguments, for indices outside [0, C + 1) too: torch_scatter's restatement
    cannot index a bucket that does not exist, so such slots go to one EXTRA bucket, which is dropped behind the pooling (the
    kernels drop the slots); the rest is the oracle's own lines (oracle/digat_oracle.py:127-129).  The CPU file holds this to
    oracle.user_graph_context where every index is valid."""
    C1 = p["topic_node_embedding"].shape[0] + 1
    q = dict(p, topic_node_embedding=torch.zeros(C1, Xu.shape[2], dtype=Xu.dtype))
    idx = torch.where((cat_idx >= 0) & (cat_idx < C1), cat_idx, torch.full_like(cat_idx, C1))
    topics = O.topic_pooling(q, Xu, idx, c_n, H)[:, :C1]
    topics = torch.relu(O._linear(topics, p, "featureAffine")) + topics
    return O.scaled_dot_attention(p, "userAttention", topics, c_n, cat_mask)


# ---- D: the one-launch user context alone --------------------------------------------------------------------------------------
FUSED_D = (240, 320, 400)      # d % 8 == 0 within (192, 448]: four, five and seven waves
FUSED_H = (1, 4, 5, 49, 51, 52)
FUSED_C1 = (6, 16, 17, 18, 20)
FUSED_B = (1, 2, 3, 5, 8)      # a last workgroup of 1 .. 3 rows and whole ones (four rows per workgroup)
FUSED_CASES = [(H, C1, d, FUSED_B[(i + j + k) % 5]) for i, H in enumerate(FUSED_H) for j, C1 in enumerate(FUSED_C1) for k, d in enumerate(FUSED_D)]
FUSED_REFUSED = ((53, 18, 400), (50, 21, 400), (50, 18, 192), (50, 18, 456), (50, 18, 244))
# The one launch against the three (FUSED_VS_LAUNCHES) is run at gain 1 only.  Both routes compute the topic scores with the same
# arithmetic; they differ in featureAffine's product (fp16x3 | fp32) and in the ORDER in which the final pooling sums its scores over
# the channels.  A d-term fp32 sum of magnitude ~ gain sqrt(d) moves by about sqrt(d) ulp(gain sqrt(d)) / sqrt(d) ~ gain 1e-6 with
# the order, which the softmax hands to the output as a relative error of that size: at gain 4 the order alone is worth the 2e-6
# the bound allows, which tests/test_hip_parity.py set on queries of unit scale.  Against fp64 (OUT_TOL) both gains are run.
FUSED_LAUNCHES_GAIN = 1.0


def fused_users(H, C1, g):
    """(idx [8, H], mask bool [8, C1]): a user reading all C categories, every bucket unmasked [min(H, C) slots: 16 .. 19 of them at
    C + 1 = 17 .. 20 — more than the row's tile of 16]; ctx0_users' empty history; its one item; an all-masked user with all C + 1
    buckets present [min(H, C + 1) slots]; ctx0_users' reader of everything, its masked / unread pair and its all-masked padded
    history; a random history under a 60 % mask.  In this order rows 0, 3 and 4 overflow the tile (H >= C + 1 >= 17) and share
    their workgroups with rows that do not."""
    ci, cm = ctx0_users(H, C1, g)
    C = C1 - 1
    idx = torch.stack([torch.arange(H) % max(C, 1), ci[1], ci[2], torch.arange(H) % C1, ci[0], ci[3], ci[4], torch.randint(0, C1, (H,), generator=g)])
    some = torch.rand(C1, generator=g) < 0.6
    some[0] = True
    mask = torch.stack([torch.ones(C1, dtype=torch.bool), cm[1], cm[2], torch.zeros(C1, dtype=torch.bool), cm[0], cm[3], cm[4], some])
    return idx, mask


@functools.lru_cache(maxsize=8)
def fused_inputs(H, C1, d, B, gain, lists=False):
    """dict of fp32 x [B, H, d], kq_t = gain N(0, 1), kq_u = kq_t[:, perm] (digat_user_ctx_fwd derives both from ONE c_n: identity
    K / Q for the topic query, a permutation for the user query, as tests/test_hip_user_ctx0.py does), idx, mask, Fa = N(0, 1) /
    sqrt(d), bFa = 0.3 N(0, 1) (relu(b) has zeros and positive entries), addend; with ``lists``: live uint8 [B, H + 1] (pad 0xEE),
    hlast int32 [B] and NaN in the dead rows — rows live below H, 4k + 1, 1, 4k, 0, 4k - 1, H, 4k + 1, row 6 with a dead slot in
    the middle."""
    g = _gen("fused", H, C1, d, B, gain, lists)
    idx, mask = fused_users(H, C1, g)
    idx, mask = idx[:B].contiguous(), mask[:B].contiguous()
    x, kq_t = torch.randn(B, H, d, generator=g), gain * torch.randn(B, d, generator=g)
    perm = torch.randperm(d, generator=g)
    c = dict(x=x, kq_t=kq_t, kq_u=kq_t[:, perm].contiguous(), perm=perm, idx=idx, mask=mask, Fa=torch.randn(d, d, generator=g) / math.sqrt(d),
             bFa=0.3 * torch.randn(d, generator=g), addend=torch.randn(B, d, generator=g))
    if lists:
        h = topic_hlasts(H)
        hl = [h[5], h[4], h[1], h[3], h[0], h[2], h[6], h[7]][:B]
        live = torch.arange(H).unsqueeze(0) < torch.tensor(hl).unsqueeze(1)
        if B > 6 and hl[6] >= 3:
            live[6, hl[6] // 2] = False
        x[~live] = NAN
        flags = torch.full((B, H + 1), 0xEE, dtype=torch.uint8)
        flags[:, :H] = live.to(torch.uint8)
        c.update(live=flags, hlast=torch.tensor(hl, dtype=torch.int32))
    return c


def fused_eval(c, C1, dtype=torch.float64):
    """compute_user_graph_context (graphEncoders.py:123-134) from the two folded queries, row by row in ``dtype``: topic_eval, then
    T' = relu(T Fa^T + b) + T, the scores T' . kq_u / sqrt(d) with -1e9 on the masked buckets, softmax, the weighted sum of T'."""
    d = c["x"].shape[2]
    live = c["live"][:, :c["x"].shape[1]] if "live" in c else None
    T = _dev_f(topic_eval(c["x"], c["kq_t"], c["idx"], C1, dtype, live=live)[0], dtype)
    Fa, b, kq_u, mask = _dev_f(c["Fa"], dtype), _dev_f(c["bFa"], dtype), _dev_f(c["kq_u"], dtype), c["mask"].to(ref_device())
    out = torch.empty(T.shape[0], d, dtype=dtype, device=T.device)
    for r in range(T.shape[0]):
        T2 = torch.relu(T[r] @ Fa.T + b) + T[r]
        s = ((T2 @ kq_u[r]) / math.sqrt(d)).masked_fill(~mask[r], O.MASK_FILL)
        out[r] = torch.softmax(s, dim=0) @ T2
    return out.cpu()
