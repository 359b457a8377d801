"""Shared by tests/test_step_fp64_cpu.py and tests/test_hip_step_fp64.py: what is left of a training step once the attention side is
held — the vanilla-GAT layer (csrc/digat_gat.inc), the two table-gradient paths (csrc/digat_news_train.inc) and the step's head and
tail (csrc/digat_train.inc: row logits, click loss, clipping + Adam) — the case lists both files run, the inputs of a case, the
references and the comparison.  No reference value comes from the library.  The CPU file pins the references to the oracle and the
golden fixtures and holds the stock fp32 formulations to HALF of the tolerance on every case listed here; the GPU file holds the
HIP kernels to the whole of it.

Blocks:
  A  the GAT layer: digat_gat_fwd and the pair digat_gat_fwd_train / digat_gat_bwd against ``gat_fp64`` under torch autograd on
     double copies of the fp32 inputs, the attention dropout drawn from the kernels' hash (oracle.hash_dropout)
  B  digat_embedding_bwd (sorted) and digat_embedding_bwd_unsorted alone: integer-valued rows against an int64 index_add_ bit for
     bit, normal rows against an fp64 index_add_ under the recursive-summation bound count 2^-24 sum|rows| per element
  C  digat_row_logits / _bwd, digat_click_loss / training.ClickLoss against fp64, optim.ClipAdam against an fp64 restatement of
     clip_grad_norm_ + Adam

Tolerances are the project's: eq8_fp64_common's OUT_TOL / TRAIN_OUT_TOL / GRAD_TOL for block A, the figures of
tests/test_hip_training.py's test_step_head_and_tail_match_torch_autograd and test_clip_adam_matches_clip_grad_norm_and_torch_adam for
block C (with that file's floor: relative to max(|want|, 5 % of the tensor's scale)); block B has the exact / derived rule above."""
import functools
import zlib

import numpy as np
import torch

import eq8_fp64_common as E
from eq8_fp64_common import GRAD_TOL, OUT_TOL, TRAIN_OUT_TOL, Case, adjacency, close, ref_device      # noqa: F401  (re-exported)
from oracle import digat_oracle as O

NAN = float("nan")
OK, ERR_ARG, ERR_SHAPE = 0, 1, 2
HALF = 0.5
F = torch.nn.functional


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ==== A: the GAT layer ==============================================================================================================
GAT_KINDS = ("mixed", "full", "twins", "none")          # eq8_fp64_common.adjacency's
# n: 1; 2; 16 | 17; 63 | 64 | 65 one | two neighbours per lane of gat_alpha_kernel; 67 the user graph; 112 | 113 the score backward's
# chunk size (launch_ds); 127 | 128 the limit
GAT_N = (1, 2, 16, 17, 63, 64, 65, 67, 112, 113, 127, 128)
GAT_D_ALL_N = (36, 256)
# d: 4; 64; 252 | 256 | 260: d / 4 = 63 | 64 | 65, one | two steps of gat_node_scores_kernel's lane loop, and 256 | 260 one | two
# steps of gat_score_bwd_kernel's channel loop; 400; 512; 1024 the limit | 1028 beyond it
GAT_D = (4, 64, 252, 256, 260, 400, 512, 1024, 1028)
GAT_N_ALL_D = (10, 67)
GAT_SHAPES = sorted({(n, d) for n in GAT_N for d in GAT_D_ALL_N} | {(n, d) for n in GAT_N_ALL_D for d in GAT_D})
# d = 1028: the aggregation kernel the layer ends in serves up to 16 groups of 64 channels (eq8_agg_route's upto_1024); all three
# entries refuse the shape with DIGAT_ERR_SHAPE before any launch (include/digat_hip.h).  The references of these cases are still
# built and pinned on the CPU; the GPU file asserts the code.
GAT_REFUSED = {d: ERR_SHAPE for d in GAT_D if d > 1024}
GAT_CASES = [Case(n, d, E._batch(n, d), k) for n, d in GAT_SHAPES for k in GAT_KINDS]                 # B = 1 .. 3, fixed per shape
# B n >= 2048 with d % 80 == 0: the bf16x6 routes of t_linear_fwd, t_linear_bwd_input and t_linear_bwd_weight inside the pair
GAT_X3 = [Case(67, 80, 32, "mixed"), Case(17, 240, 121, "mixed")]
GAT_P = (0.0, 0.3)
GAT_SEED = 4242                 # the attention dropout's seed of every case
GAT_FULL_GAIN = 2.0             # the largest gain on a1 / a2 of the dense cases (see gat_gain)


def gat_gain(case):
    """The gain on a1 and a2 of the dense kinds (`full`, and `twins`: a history in one category is a clique), after
    eq8_fp64_common.train_gain: GAT_FULL_GAIN up to d = 64, 8 GAT_FULL_GAIN / sqrt(d) beyond, so that attention over a hundred entries
    is far from uniform.  Eq. 8's cases take 8; here the score is a1 . h_j + a2 . h_i, and the gradient of a2 sums ds_ij over the
    neighbours j of a centre — a softmax gradient, which sums to zero but for leaky_relu's two slopes and the mask.  At gain 8 that
    cancellation alone left the fp32 oracle at 0.77 - 2.09 of GRAD_TOL on a2 ((127, 36), (10, 64), (10, 260), `full`), at gain 4 still
    at 2.96 ((113, 36), `twins`); the tolerance stays, the gain came down until the fp32 oracle was within half on every case, at 2
    (tests/test_step_fp64_cpu.py).  `mixed`
    and `none` take no gain."""
    return min(GAT_FULL_GAIN, 8.0 * GAT_FULL_GAIN / case.d ** 0.5) if case.kind in ("full", "twins") else 1.0


def gat_fp64(X, A, W, bW, a1, a2, drop=None):
    """oracle.gat_layer restated on plain tensors, in the dtype of its arguments (fp64 for the reference), with a hook on alpha:
    h = X W^T + bW; e_ij = leaky_relu_0.2(a1 . h_j + a2 . h_i); -1e9 where A_ij = 0; alpha = softmax_j; out = relu(drop(alpha) h) + X.
    a1, a2: [d] or [1, d]."""
    B, n, _ = X.shape
    h = F.linear(X, W, bW)
    e = F.leaky_relu(F.linear(h, a1.reshape(1, -1)).view(B, 1, n) + F.linear(h, a2.reshape(1, -1)), 0.2)
    alpha = F.softmax(e.masked_fill(A == 0, O.MASK_FILL), dim=2)
    if drop is not None:
        alpha = drop(alpha)
    return F.relu(torch.bmm(alpha, h)) + X


def gat_drop(p_alpha, seed=GAT_SEED):
    """The hook that applies the kernels' keep bits: digat_dropout_fwd runs over the contiguous [B, n, n] alpha, the flat hash of
    oracle.hash_dropout is the same function."""
    return (lambda alpha: O.hash_dropout(alpha.contiguous(), p_alpha, seed)) if p_alpha > 0 else None


KINK_MARGIN = E.KINK_MARGIN     # of relu's argument, relative to the sum of the magnitudes of its terms
SCORE_MARGIN = E.SCORE_MARGIN   # of leaky_relu's argument, relative to the sum of the magnitudes of its terms
RES_MARGIN = 2.0 ** -22         # of relu's argument, relative to the residual: four times fp32's unit roundoff
NEGLIGIBLE = 1e-7               # a gradient term of this size is a twentieth of GRAD_TOL's atol


def _gat_off_the_kinks(X, dOut, A, w):
    """Moves bW and a1 (in place, by a few 1e-4) until, in fp64, no pre-activation that reaches a gradient lies at the kink of its
    activation — as eq8_fp64_common._keep_off_the_kinks does, and for its reason: a training case is a condition on its inputs; fp32
    rounding that flips one such derivative moves a gradient summed over a few hundred rows by percents, in the fp32 oracle as in
    a kernel.  Off the kinks the function is smooth and the tolerances measure arithmetic.
      * the scores a1 . h_j + a2 . h_i on the adjacency entries (leaky_relu): SCORE_MARGIN of the sum of |a_c h_c|;
      * Z = alpha' h with and without the attention dropout of GAT_P (relu): KINK_MARGIN of the sum of alpha'_j |h_j|.  A row whose
        every entry was dropped is exactly zero in any arithmetic;
      * digat_gat_bwd reads relu' off out - X > 0 (relu_res_mask_kernel), which a positive Z below half an ulp of X cannot show: Z < 0,
        or Z >= RES_MARGIN |X|.  A row whose kept weights sum to r ~ 1e-5 (a dense graph at gain 8 whose dominant entry was dropped)
        has Z ~ r h, and no bW lifts that above 2^-22 |X|.  Everything relu'(Z_ic) multiplies is dOut_ic times the row's weights:
        where r |dOut_ic| max(1, |h|) <= NEGLIGIBLE the element is left alone; at the few elements in between the COTANGENT is set
        to zero (in place), which takes the term out of both sides."""
    Xd, Ab = X.double(), A.bool()
    W = w["W"].double()
    h0 = Xd @ W.T                                                                                   # without bW
    a1_0 = w["a1"].clone()
    d = X.shape[2]
    for attempt in range(50):
        if attempt:                                                                                 # the scores were at a kink: another a1
            w["a1"].copy_(a1_0)
            w["a1"].view(-1)[(attempt - 1) % d] += 1e-3 * float(a1_0.abs().max()) * (1 + attempt // d)
        a1, a2 = w["a1"].double().view(-1), w["a2"].double().view(-1)

        def scores():
            h = h0 + w["bW"].double()
            s = (h @ a1).unsqueeze(1) + (h @ a2).unsqueeze(2)                                       # [B, i, j]: a1 over j, a2 over i
            mag = (h.abs() @ a1.abs()).unsqueeze(1) + (h.abs() @ a2.abs()).unsqueeze(2)
            return s, bool((s.abs() >= SCORE_MARGIN * mag).masked_fill(~Ab, True).all())
        s, ok = scores()
        if not ok:
            continue
        alpha = torch.softmax(F.leaky_relu(s, 0.2).masked_fill(~Ab, O.MASK_FILL), dim=2)
        alphas = [alpha if p == 0 else O.hash_dropout(alpha.contiguous(), p, GAT_SEED) for p in GAT_P]
        Z0 = torch.stack([al @ h0 for al in alphas])                                                # [P, B, n, d]
        M0 = torch.stack([al @ h0.abs() for al in alphas])
        r = torch.stack([al.sum(dim=2) for al in alphas]).unsqueeze(3)                              # [P, B, n, 1]
        dead = r == 0
        small = r * dOut.double().abs() * max(1.0, float(h0.abs().max()) + 1.0) <= NEGLIGIBLE

        def conditions(cand):
            Z = Z0 + cand * r
            return (Z.abs() >= KINK_MARGIN * (M0 + cand.abs() * r)) | dead, (Z < 0) | (Z >= RES_MARGIN * Xd.abs()) | dead | small
        per_channel = lambda m: m.all(dim=0).all(dim=0).all(dim=0)
        b0 = w["bW"].double().clone()
        for both in (True, False):                              # False: the second condition is left to the cotangent
            cand, todo = b0.clone(), torch.ones(d, dtype=torch.bool)
            for t in range(200):
                step = ((t + 1) // 2 * (1 if t % 2 else -1)) * 37 * KINK_MARGIN
                cand[todo] = (b0[todo] + step).float().double()
                sign_ok, seen_ok = conditions(cand)
                todo = ~per_channel(sign_ok & seen_ok if both else sign_ok)
                if not bool(todo.any()):
                    break
            if not bool(todo.any()):
                break
        else:
            raise AssertionError("no bW keeps alpha h off zero")
        w["bW"].copy_(cand.float())
        if not scores()[1]:                                                                         # bW moves h, and with it the scores
            continue
        unseen = ~conditions(cand)[1].all(dim=0)                                                    # [B, n, d]
        assert int(unseen.sum()) <= 1e-3 * unseen.numel(), (int(unseen.sum()), unseen.numel())
        dOut[unseen] = 0.0
        return
    raise AssertionError("no (a1, bW) keeps the scores and alpha h off their kinks")


@functools.lru_cache(maxsize=4)
def gat_inputs(case):
    """fp32 (X [B, n, d], cotangent, A bool [B, n, n], weights {W, bW, a1 [1, d], a2 [1, d]}) of a Case, drawn as
    tests/test_hip_training.py draws them, a1 and a2 times gat_gain(case).  Cached: callers leave them unchanged."""
    n, d, B, kind = case
    g = _gen("gat", *case)
    X, dOut = torch.randn(B, n, d, generator=g), torch.randn(B, n, d, generator=g)
    w = {k: torch.randn(*shape, generator=g) * scale for k, shape, scale in
         [("W", (d, d), d ** -0.5), ("bW", (d,), 0.1), ("a1", (1, d), d ** -0.5 * gat_gain(case)), ("a2", (1, d), d ** -0.5 * gat_gain(case))]}
    A = torch.from_numpy(adjacency(kind, n, B))
    _gat_off_the_kinks(X, dOut, A, w)
    return X, dOut, A, w


GAT_GRADS = ("X", "W", "bW", "a1", "a2")


def gat_eval(case, dtype, p_alpha, stock=False):
    """(output, {X, W, bW, a1, a2: gradient}) of the layer in ``dtype`` under torch autograd with the cotangent of gat_inputs.
    ``stock`` (fp32, p_alpha = 0): oracle.gat_layer itself on its parameter dictionary."""
    X, dOut, A, w = gat_inputs(case)
    Xo = X.detach().to(dtype).clone().requires_grad_(True)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    if stock:
        assert p_alpha == 0
        out = O.gat_layer({"user_graph_attention_W.0.weight": p["W"], "user_graph_attention_W.0.bias": p["bW"],
                           "user_graph_attention_a1.0.weight": p["a1"], "user_graph_attention_a2.0.weight": p["a2"]}, "user", 0, Xo, A)
    else:
        out = gat_fp64(Xo, A, p["W"], p["bW"], p["a1"], p["a2"], drop=gat_drop(p_alpha))
    assert out.dtype == dtype
    (out * dOut.to(dtype)).sum().backward()
    return out.detach(), {"X": Xo.grad, **{k: p[k].grad for k in w}}


@functools.lru_cache(maxsize=4)
def gat_reference(case, p_alpha):
    """gat_eval in fp64, and the condition of the case: every gradient's largest element is above 1e-3 of the scale of the tensor it
    belongs to (the 5 % floor of the comparison is then a floor under real signal) — except a1 and a2 where nothing reaches the
    scores: a single node attends to itself with weight one, a centre without an entry attends uniformly, and those gradients are
    exactly zero.  (A centre with a single entry attends to it with weight one: inert as well.)"""
    out, grads = gat_eval(case, torch.float64, p_alpha)
    X, _, A, w = gat_inputs(case)
    scale = {"X": X, **w}
    inert = int(A.sum(dim=2).max()) <= 1
    for k, g in grads.items():
        if inert and k in ("a1", "a2"):
            assert float(g.abs().max()) == 0.0, (case, k)
        elif case.n >= 10 or k not in ("a1", "a2"):             # (two nodes: the softmax gradients of a centre sum to zero, and so can a2's)
            assert float(g.abs().max()) > 1e-3 * float(scale[k].abs().max()), (case, k, float(g.abs().max()))
    return out, grads


# ==== B: the table gradients ========================================================================================================
EMB_CHUNK = 64                  # csrc/digat_news_train.inc:265 `constexpr int EMB_CHUNK = 64;` — positions per workgroup of both paths
U24 = 2.0 ** -24                # the unit roundoff of fp32


def sorted_levels(M):
    """Launches of embedding_bwd_kernel for M rows (digat_embedding_bwd's loop: a level leaves two partial rows per chunk)."""
    levels, n = 1, M
    while (n + EMB_CHUNK - 1) // EMB_CHUNK > 1:
        n, levels = 2 * ((n + EMB_CHUNK - 1) // EMB_CHUNK), levels + 1
    return levels


def unsorted_U(dm):
    """float4 pieces per lane of embedding_bwd_chunk_kernel<U> / embedding_bwd_merge_kernel<U> (digat_embedding_bwd_unsorted)."""
    return 1 if dm <= 256 else 2 if dm <= 512 else 4


# M: 1; 63 | 64 | 65 one | two chunks (one | two levels); 128 | 129; 2048 | 2049 two | three levels; 4161 = 65 chunks + 1 row (66 chunks, three levels,
# and room for a run over more than 32 whole chunks that fills a whole chunk of the SECOND level); 20000
SORTED_M = (1, 63, 64, 65, 128, 129, 2048, 2049, 4161, 20000)
# dm: 4; 7 (odd: the kernel takes any width); 256 | 260 one | two steps of the channel loop; 300
SORTED_DM = (4, 7, 256, 260, 300)
SORTED_DM_ALL_M, SORTED_M_ALL_DM = (7, 260), (65, 2049, 4161)
SORTED_SHAPES = sorted({(M, dm) for M in SORTED_M for dm in SORTED_DM_ALL_M} | {(M, dm) for M in SORTED_M_ALL_DM for dm in SORTED_DM})
SORTED_LD_PAD = (0, 5)          # ld_row_grad = dm, and dm + 5 with NaN in the unused columns
SORTED_LAYOUTS = ("same", "distinct", "chunk64", "long", "border", "tail", "drawn")


def _runs(runs, M):
    """Sorted tokens [M] from (token, length) runs with ascending tokens, cut at M; what is left over is distinct tokens."""
    out = np.empty(M, dtype=np.int64)
    pos, last = 0, -1
    for tok, length in runs:
        assert tok > last
        last = tok
        k = min(length, M - pos)
        out[pos:pos + k] = tok
        pos += k
    out[pos:] = last + 2 + 2 * np.arange(M - pos)
    return out


def sorted_tokens(layout, M):
    """The SORTED token sequence [M] of a layout, built by hand:
      same      every position the same token
      distinct  every position a distinct token (odd ones: every second row of the table stays zero)
      chunk64   5 + 59 positions, then a run of exactly 64 that coincides with chunk 1, then runs of 3
      long      ten distinct tokens, then ONE token up to three positions before the end: a run that covers whole chunks and goes on
                in the next (the open-head-and-tail chunk, whose second slot carries a zero row); from M = 4161 on it covers more
                than 32 whole chunks and fills a whole chunk of the second level, where the case recurs
      border    runs of 64, 32, 32, 64, 128, 64 ...: every run ends exactly on a chunk border with another token behind it
      tail      drawn tokens below 50, and one token that occupies the last, partial chunk alone (the last 17 positions when M is a
                multiple of 64)
      drawn     half of the positions the padding token 0, the others drawn from 1 .. 199"""
    rng = _rng("sorted", layout, M)
    if layout == "same":
        return np.full(M, 3, dtype=np.int64)
    if layout == "distinct":
        return 1 + 2 * np.arange(M, dtype=np.int64)
    if layout == "chunk64":
        return _runs([(1, 5), (4, 59), (6, 64)] + [(10 + 2 * k, 3) for k in range((max(M - 128, 0) + 2) // 3)], M)
    if layout == "long":
        return _runs([(k, 1) for k in range(10)] + [(20, max(M - 13, 1))], M)
    if layout == "border":
        lens = [64, 32, 32, 64, 128, 64]
        return _runs([(2 * k + 1, lens[k % 6]) for k in range(M // 32 + 1)], M)
    if layout == "tail":
        last = M % EMB_CHUNK or min(17, M)
        return np.concatenate([np.sort(rng.integers(0, 50, size=M - last)), np.full(last, 77)]).astype(np.int64)
    if layout == "drawn":
        return np.sort(np.where(rng.random(M) < 0.5, 0, rng.integers(1, 200, size=M))).astype(np.int64)
    raise ValueError(layout)


def sorted_case(layout, M):
    """(tokens [M] by position, order int32 [M], sorted_tokens int32 [M], V): the layout's sorted sequence spread over the positions
    by a drawn permutation; ``order`` is the STABLE sort digat_embedding_bwd asks for (ascending position within a token)."""
    stok = sorted_tokens(layout, M)
    tokens = np.empty(M, dtype=np.int64)
    tokens[_rng("perm", layout, M).permutation(M)] = stok
    order = np.argsort(tokens, kind="stable")
    assert np.array_equal(tokens[order], stok)
    return tokens, order.astype(np.int32), stok.astype(np.int32), int(stok.max()) + 3


def open_chunks_per_level(stok):
    """Per level of digat_embedding_bwd, the number of chunks that are ONE run open at both ends (the zero-row case of
    embedding_bwd_kernel), from the token sequence alone — the kernel's bookkeeping restated for the CPU file's coverage check."""
    counts, tok = [], [int(t) for t in stok]
    while True:
        chunks = (len(tok) + EMB_CHUNK - 1) // EMB_CHUNK
        nxt, both = [], 0
        for k in range(chunks):
            c = tok[k * EMB_CHUNK:(k + 1) * EMB_CHUNK]
            before = tok[k * EMB_CHUNK - 1] if k else -2
            after = tok[(k + 1) * EMB_CHUNK] if (k + 1) * EMB_CHUNK < len(tok) else -2
            head, tail = c[0] == before and c[0] >= 0, c[-1] == after and c[-1] >= 0
            one_run = all(t == c[0] for t in c)
            if head and tail and one_run:
                both += 1
                nxt += [c[0], c[0]]
            else:
                nxt += [c[0] if head else -1, c[-1] if tail else -1]
        counts.append(both)
        if chunks == 1:
            return counts
        tok = nxt


# dm: 4; 252 | 256 | 260 U = 1 | 2; 512 | 516 U = 2 | 4; 1024 the limit
UNSORTED_DM = (4, 252, 256, 260, 512, 516, 1024)
# (M0, M1): one list alone; the first list NULL; a few ids; a list boundary inside chunk 0 (37) and on a chunk border (64), M = 101 not a
# multiple of 4; 513 = 8 chunks + 1; 6437: 101 chunks, the boundary inside chunk 50; (1, 1100)
UNSORTED_M = ((1, 0), (0, 5), (3, 2), (37, 64), (64, 37), (100, 413), (3200, 3237), (1, 1100))
UNSORTED_V = (1, 50, 70000)
UNSORTED_LD_PAD = (4, 8)        # ld0 = dm + 4, ld1 = dm + 8: both multiples of 4, both larger than dm, NaN in the unused columns
UNSORTED_DM_ALL_M, UNSORTED_M_ALL_DM = (4, 260, 516), ((37, 64), (100, 413), (3200, 3237))
UNSORTED_CASES = sorted({(dm, M, 50) for dm in UNSORTED_DM_ALL_M for M in UNSORTED_M} | {(dm, M, 50) for dm in UNSORTED_DM for M in UNSORTED_M_ALL_DM}
                        | {(dm, M, V) for dm in (256, 516) for M in ((3, 2), (64, 37), (1, 1100), (3200, 3237)) for V in (1, 70000)})
PAD_ID, MANY_ID, FAR_ID, LAST_ID, SECOND_ID = 0, 1, 2, 3, 4


def unsorted_ids(M0, M1, V):
    """(ids int64 [M0 + M1] — the two lists one behind the other — and the set of patterns the case holds).  Built by hand over
    drawn ids from 5 .. min(V, 40) - 1 (V <= 5: the padding id alone), as far as the case has room:
      out     ids outside [0, V): -1, V, V + 5 and 2^40 — they receive nothing and disturb nothing
      pad     id 0 fills chunks 2 and 3 whole, and lies here and there elsewhere
      many    id 1 once in every chunk but 2, 3 and the last (M >= 12 chunks: present in more than 8)
      far     id 2 in chunk 0 and next only in chunks 9, 12, 15 ...: the merge's first step of eight chunks finds one partial row, its
              second step the rest
      last    id 3 only in the last, partial chunk
      second  id 4 only in the second list
      top     the id V - 1"""
    rng = _rng("unsorted", M0, M1, V)
    M, C = M0 + M1, EMB_CHUNK
    has = set()
    ids = rng.integers(5, min(V, 40), size=M) if V > 5 else np.zeros(M, dtype=np.int64)
    ids = ids.astype(np.int64)
    chunks = (M + C - 1) // C
    # the positions of `out` and `top` are set aside first: no other pattern is written there
    out_at = [] if M < 5 else [1, M // 2, M - 2, M - 1] if M < 100 else [1, 70, M // 2 + 1, M - 2]
    top_at = [q for q in (2, 0) if q not in out_at][:1] if M >= 3 and V > 1 else []
    taken = set(out_at + top_at)

    def free(positions):                                                               # ... and each pattern keeps what it takes
        got = np.array([q for q in positions if q not in taken], dtype=np.int64)
        taken.update(int(q) for q in got)
        return got
    if V > 5:
        ids[rng.random(M) < 0.1] = PAD_ID
        if M >= 4 * C and not taken & set(range(2 * C, 4 * C)):
            ids[2 * C:4 * C] = PAD_ID
            has.add("pad")
        many = free(k * C + 9 for k in range(chunks - 1) if k not in (2, 3))
        if len(many) > 8:
            ids[many] = MANY_ID
            has.add("many")
        far = free(k * C + 11 for k in range(9, chunks - 1, 3))
        if len(far) >= 1:
            ids[ids == FAR_ID] = 5                                                     # (drawn ids start at 5; none is FAR_ID)
            ids[3], ids[far] = FAR_ID, FAR_ID
            taken.add(3)
            has.add("far")
        if M % C and M > C:
            last = free(sorted(set((M - 1) // C * C + rng.integers(0, M % C, size=min(3, M % C)))))
            if len(last):
                ids[last] = LAST_ID
                has.add("last")
        second = free(M0 + q for q in (0, M1 // 2, M1 - 1) if M0 >= 1 and M1 >= 2)
        if len(second):
            ids[second] = SECOND_ID
            has.add("second")
    if out_at:
        ids[np.array(out_at)] = np.array([-1, V, V + 5, 1 << 40])
        has.add("out")
    if top_at:
        ids[top_at[0]] = V - 1
        has.add("top")
    # every pattern the case claims is there, and only where it is meant to be
    if "pad" in has:
        assert (ids[2 * C:4 * C] == PAD_ID).all()
    if "many" in has:
        assert len(set(np.nonzero(ids == MANY_ID)[0] // C)) > 8
    if "far" in has:
        at = np.nonzero(ids == FAR_ID)[0] // C
        assert at[0] == 0 and len(at) >= 2 and at[1] >= 9
    if "second" in has:
        assert (ids[M0:] == SECOND_ID).any() and not (ids[:M0] == SECOND_ID).any()
    if "last" in has:
        assert (ids == LAST_ID).any() and not (ids[:(M - 1) // C * C] == LAST_ID).any()
    if "out" in has:
        assert sorted(ids[(ids < 0) | (ids >= V)]) == sorted([-1, V, V + 5, 1 << 40])
    if "top" in has:
        assert (ids == V - 1).any()
    return ids, has


def table_rows(M, dm, exact, *key):
    """fp32 row gradients [M, dm]: integers in [-8, 8] (``exact``: with at most 2^20 rows per id every partial sum stays below 2^24 in
    magnitude, so every summation order gives the same fp32 value) or standard normal draws rounded to bf16.  The rounding is a
    condition on the inputs: sequential fp32 summation of three to five arbitrary floats can by itself reach (count - 1) / count of
    the bound — F.embedding's backward stood at 0.51 - 0.63 of it on plain normal rows, always at ids with a handful of rows — while
    a few eight-bit significands add exactly; ids with many rows round as any (from some sixteen rows on, and the padding id has
    thousands), and the CPU file holds F.embedding's backward to half of the bound on every case."""
    g = _gen("rows", M, dm, exact, *key)
    return torch.randint(-8, 9, (M, dm), generator=g).float() if exact else torch.randn(M, dm, generator=g).bfloat16().float()


def padded(rows, pad):
    """rows [M, dm] inside a NaN-filled [M, dm + pad] buffer: (buffer, ld)."""
    buf = torch.full((rows.shape[0], rows.shape[1] + pad), NAN)
    buf[:, :rows.shape[1]] = rows
    return buf, rows.shape[1] + pad


def table_check(got, ids, rows, V, exact, what):
    """Holds a table gradient [V, dm] to the sum of ``rows`` per id of ``ids`` (ids outside [0, V) dropped).  Exact inputs: equal to an
    int64 index_add_, bit for bit.  Normal inputs: |err[t, c]| <= count[t] 2^-24 sum|rows[t, c]| of an fp64 index_add_ — the
    recursive-summation bound, valid for any order (adding the zero rows of the open chunks is exact) — with no table-wide scale;
    rows of ids that do not occur must be exactly 0.  Returns the worst err / bound."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    dm = rows.shape[1]
    assert got.shape == (V, dm) and got.dtype == torch.float32, (what, got.shape)
    ok = (ids >= 0) & (ids < V)
    uniq, inv = torch.unique(ids[ok], return_inverse=True)             # the ids that occur, ascending; only their rows leave the device
    r, T = rows[ok], uniq.numel()
    occurs = torch.zeros(V, dtype=torch.bool)
    occurs[uniq] = True
    untouched = (got.detach() == 0).all(dim=1).cpu()
    assert bool(untouched[~occurs].all()), f"{what}: a row of an id that does not occur is not exactly 0"
    got = got.detach()[uniq.to(got.device)].cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
    count = torch.zeros(T, dtype=torch.int64).index_add_(0, inv, torch.ones_like(inv))
    if exact:
        want = torch.zeros(T, dm, dtype=torch.int64).index_add_(0, inv, r.long())
        assert int(want.abs().max()) < 2 ** 24 if T else True
        if not torch.equal(got, want.float()):
            bad = torch.nonzero((got != want.float()).any(dim=1)).flatten()
            raise AssertionError(f"{what}: {bad.numel()} rows differ from the integer sum, first id {int(uniq[bad[0]])} (count {int(count[bad[0]])})")
        return 0.0
    want = torch.zeros(T, dm, dtype=torch.float64).index_add_(0, inv, r.double())
    bound = count.double().unsqueeze(1) * U24 * torch.zeros(T, dm, dtype=torch.float64).index_add_(0, inv, r.double().abs())
    err = (got.double() - want).abs()
    if bool((err > bound).any()):
        t, c = np.unravel_index(int(torch.argmax(err - bound)), err.shape)
        raise AssertionError(f"{what}: id {int(uniq[t])} (count {int(count[t])}) column {c}: got {float(got[t, c]):.9g} want {float(want[t, c]):.9g}, "
                             f"err {float(err[t, c]):.3e} > bound {float(bound[t, c]):.3e}")
    return float((err / bound.clamp_min(1e-300)).max()) if T else 0.0


# ==== C: the step's head and tail ===================================================================================================
# tests/test_hip_training.py:test_step_head_and_tail_match_torch_autograd's figures, with that file's 5 % floor
LOGIT_TOL = dict(rtol=1e-5, atol=1e-5, floor=0.05)
LOSS_TOL = dict(rtol=1e-6, atol=1e-6, floor=0.05)
HEAD_GRAD_TOL = dict(rtol=2e-5, atol=1e-8, floor=0.05)         # d news_ctx, d user_ctx there; d logits here
# ... and test_clip_adam_matches_clip_grad_norm_and_torch_adam's
ADAM_TOL = dict(rtol=2e-5, atol=1e-6, floor=0.05)

# B: 1; 3; 257 = 64 workgroups of four rows + 1; 4099.  d: 4; 36; 256 | 260 four | five steps of a lane; 1028
LOGITS_B, LOGITS_D = (1, 3, 257, 4099), (4, 36, 256, 260, 1028)


@functools.lru_cache(maxsize=4)
def logits_inputs(B, d):
    """fp32 (news_ctx [B, d], user_ctx [B, d] at 0.3, d logits [B]) as tests/test_hip_training.py draws the contexts."""
    g = _gen("logits", B, d)
    return torch.randn(B, d, generator=g), 0.3 * torch.randn(B, d, generator=g), torch.randn(B, generator=g)


def logits_eval(nc, uc, dl, dtype=torch.float64):
    """(logits, d news_ctx, d user_ctx) of model.py:75 in ``dtype``."""
    nc, uc, dl = nc.to(dtype), uc.to(dtype), dl.to(dtype)
    return (uc * nc).sum(dim=1), dl.unsqueeze(1) * uc, dl.unsqueeze(1) * nc


# B: 1; 2; 255 | 256 | 257 one | two steps of click_loss_kernel's impression loop; 1000.  K: 1 (the loss is exactly 0); 2; 5; 300
LOSS_B, LOSS_K = (1, 2, 255, 256, 257, 1000), (1, 2, 5, 300)
# normal: N(0, 1); equal: every logit 0.75; x30: 30 N(0, 1), where only the max-subtraction keeps exp finite (exp(88.8) overflows fp32)
# — row 0's two first logits are both set to the row's maximum: d logits then has the scale 1 / (2 B) whatever the draw.  Without it
# a batch of one or two rows can consist of rows like p0 = 1 - 4e-4 alone, whose p0 - 1 carries fp32's absolute resolution of p0
# (6e-8) while nothing but itself sets the scale (torch.log_softmax in fp32 stood at 1.59 of the tolerance at B = K = 2);
# first: the clicked column 0 by far the largest (the others N(0, 1) - 30: the loss is ~ K e^-30, below fp32's resolution of 1 + x);
# last: by far the smallest (the others N(0, 1) + 30: the loss is ~ 30 + log(K - 1))
LOSS_KINDS = ("normal", "equal", "x30", "first", "last")
LOSS_DLOSS = 1.7                # the incoming gradient of the training.ClickLoss run


def loss_inputs(B, K, kind):
    g = _gen("loss", B, K, kind)
    x = torch.randn(B, K, generator=g)
    if kind == "equal":
        x = torch.full((B, K), 0.75)
    elif kind == "x30":
        x = 30.0 * x
        if K >= 2:
            x[0, :2] = x[0].max()
    elif kind in ("first", "last"):
        x[:, 1:] += -30.0 if kind == "first" else 30.0
    return x.contiguous()


def loss_eval(logits, dtype=torch.float64):
    """(loss, d loss / d logits) of trainer.py:100 — mean(-log_softmax(logits, dim=1)[:, 0]) — in ``dtype`` under autograd."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = (-torch.log_softmax(x, dim=1).select(1, 0)).mean()
    loss.backward()
    return loss.detach(), x.grad


# ---- clipping + Adam ---------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_BETAS, ADAM_EPS, ADAM_WD = 1e-2, (0.9, 0.999), 1e-8, 0.01
# sizes: 1; 3; 16383 | 16384 | 16385 one chunk less one | one chunk | one chunk + 1; 32771 = two chunks + 3; 70001 (five chunks); and
# 4099 as a contiguous view ONE FLOAT past a 16-byte boundary (parameter and gradient): clip_adam_kernel and grad_sq_chunks_kernel take
# their scalar paths there while the aligned tensors take the vector paths
ADAM_SIZES = (1, 3, 16383, 16384, 16385, 32771, 70001)
ADAM_UNALIGNED = 4099
ADAM_WD_GROUP = (1, 4, 7)       # indices (ADAM_SIZES + the unaligned one) of the weight-decay group; the others decay by 0
ADAM_MAX_NORMS = (0.0, 1.0, 0.05)
ADAM_STEPS = 4
ADAM_GRAD_SCALES = (3.0, 0.01)  # alternating large and small gradients
ADAM_MIN_RATIO = 1e3            # no element's |coef g + wd p| within this factor of eps


def adam_fp64_step(p, g, m, v, wds, max_norm, step, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS):
    """One step of clip_grad_norm_(all, max_norm) + torch.optim.Adam (coupled weight decay, bias correction) on lists of fp64
    tensors, in place on p, m, v; the gradients stay.  Returns (coef, the smallest |coef g + wd p| of the step)."""
    b1, b2 = betas
    coef = 1.0
    if max_norm > 0:
        total = float(torch.sqrt(sum((x * x).sum() for x in g)))
        coef = min(1.0, max_norm / (total + 1e-6))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    smallest = float("inf")
    for pk, gk, mk, vk, wd in zip(p, g, m, v, wds):
        ge = coef * gk + wd * pk
        smallest = min(smallest, float(ge.abs().min()))
        mk.mul_(b1).add_(ge, alpha=1 - b1)
        vk.mul_(b2).addcmul_(ge, ge, value=1 - b2)
        pk.sub_((lr / bc1) * mk / (vk.sqrt() / bc2 ** 0.5 + eps))
    return coef, smallest


def adam_grad(p64, scale, g):
    """An fp32 gradient for the fp64 parameter p64: scale x (0.5 + |N(0, 1)|) with the SIGN OF THE PARAMETER.  The condition of every
    Adam case: no element has |coef g + wd p| within a factor 1e3 of eps — the update m / (sqrt(v) + eps) would then measure its own
    conditioning, not the kernel.  With the parameter's sign the decay term wd p never cancels coef g, and |g| >= scale / 2 keeps
    coef g itself away from eps under every clipping coefficient of the cases (asserted on the fp64 side by adam_case)."""
    mag = scale * (0.5 + torch.randn(p64.shape, generator=g).abs())
    return torch.where(p64 < 0, -mag, mag).float()


@functools.lru_cache(maxsize=4)
def adam_case(max_norm, preset_step=0):
    """(fp32 parameters, weight decays, [fp32 gradients per step], [fp64 parameters after each step], fp32 (m, v) to preset or None).
    Tensors: ADAM_SIZES and the unaligned ADAM_UNALIGNED; ``preset_step``: the state holds that step count and drawn moments before
    the first call."""
    g = _gen("adam", max_norm, preset_step)
    sizes = ADAM_SIZES + (ADAM_UNALIGNED,)
    wds = [ADAM_WD if k in ADAM_WD_GROUP else 0.0 for k in range(len(sizes))]
    p0 = [torch.randn(s, generator=g) for s in sizes]
    preset = None
    if preset_step:
        preset = ([0.1 * torch.randn(s, generator=g) for s in sizes], [(0.1 * torch.randn(s, generator=g)) ** 2 + 1e-4 for s in sizes])
    p = [x.double() for x in p0]
    m = [x.double() for x in preset[0]] if preset else [torch.zeros_like(x) for x in p]
    v = [x.double() for x in preset[1]] if preset else [torch.zeros_like(x) for x in p]
    grads, after = [], []
    for s in range(ADAM_STEPS):
        gs = [adam_grad(x, ADAM_GRAD_SCALES[s % 2], g) for x in p]
        _, smallest = adam_fp64_step(p, [x.double() for x in gs], m, v, wds, max_norm, preset_step + s + 1)
        assert smallest >= ADAM_MIN_RATIO * ADAM_EPS, (max_norm, s, smallest)
        grads.append(gs)
        after.append([x.clone() for x in p])
    return p0, wds, grads, after, preset


ADAM_PRESET_STEP = 9999


def adam_big_numel(chunk):
    """The smallest single tensor whose squared-norm partials exceed grad_sq_total_kernel's 1024 threads: 1024 chunks + 1 element."""
    return 1024 * chunk + 1


# The case is ONE step, and one step from zero moments is p - lr g' / (|g'| + eps): the clipping coefficient cancels but for eps / |g'|,
# and the squared norm could be anything.  So the moments are preset (as in the ADAM_PRESET_STEP case), which makes the update
# m / sqrt(v) with m = b1 m0 + (1 - b1) coef g: linear in coef.  And the one element behind the 1024th chunk, which is all that
# grad_sq_total_kernel's second pass over the partials adds, carries a large gradient: about two fifths of the squared norm.
ADAM_BIG_MAX_NORM, ADAM_BIG_PRESET_STEP, ADAM_BIG_LAST = 1000.0, 9, 5000.0


@functools.lru_cache(maxsize=1)
def adam_big_case(chunk):
    """fp32 (p0, gradient, exp_avg, exp_avg_sq) of the 1024 chunks + 1 case, on the CPU: adam_grad at scale 1 with ADAM_BIG_LAST on
    the last element, moments 0.1 N(0, 1) and its square + 1e-4."""
    n, g = adam_big_numel(chunk), _gen("adam-big")
    p0 = torch.randn(n, generator=g)
    grad = adam_grad(p0, 1.0, g)
    grad[-1] = ADAM_BIG_LAST if p0[-1] >= 0 else -ADAM_BIG_LAST
    m0 = 0.1 * torch.randn(n, generator=g)
    return p0, grad, m0, m0.square() + 1e-4


def adam_big_reference(p0, grad, m0, v0, norm_of=None):
    """(fp64 parameters after the step, coef, the smallest |coef g|) on the device of the inputs.  ``norm_of``: the squared norm is
    taken over the first norm_of elements only — what a total that stops after 1024 partials would give."""
    b1, b2 = ADAM_BETAS
    step = ADAM_BIG_PRESET_STEP + 1
    g = grad.double()
    coef = min(1.0, ADAM_BIG_MAX_NORM / (float(g[:norm_of].square().sum().sqrt()) + 1e-6))
    g *= coef
    smallest = float(g.abs().min())
    m = b1 * m0.double() + (1 - b1) * g
    v = (b2 * v0.double()).addcmul_(g, g, value=1 - b2)
    del g
    return p0.double() - (ADAM_LR / (1 - b1 ** step)) * m / (v.sqrt_() / (1 - b2 ** step) ** 0.5 + ADAM_EPS), coef, smallest


def adam_ratio(got, want):
    """close()'s rule under ADAM_TOL where the tensors are (16.7 M elements stay on the device): err / tol per element."""
    tol = ADAM_TOL["atol"] + ADAM_TOL["rtol"] * torch.maximum(want.abs(), ADAM_TOL["floor"] * want.abs().max())
    return (got.double() - want).abs() / tol


def adam_big_check(p0, grad, m0, v0, chunk):
    """The reference of the case and its conditions, asserted on the fp64 side: clipping is on, no |coef g| within 1e3 of eps, and a
    squared norm that misses what lies behind the first 1024 partials moves MOST parameters by more than the tolerance (so does, a
    fortiori, no clipping at all)."""
    want, coef, smallest = adam_big_reference(p0, grad, m0, v0)
    assert coef < 0.5 and smallest >= ADAM_MIN_RATIO * ADAM_EPS, (coef, smallest)
    short, coef_short, _ = adam_big_reference(p0, grad, m0, v0, norm_of=1024 * chunk)
    miss = adam_ratio(short, want)
    del short
    assert coef_short < 1.0 and float((miss > 2.0).double().mean()) > 0.5, (coef, coef_short, float(miss.median()))
    return want
