"""Shared by tests/test_eq8_fp64_cpu.py and tests/test_hip_eq8_fp64.py: the fp64 references of Eq. 8 (the dual-interaction attention
layer), the adjacency kinds, the case lists both files run, the inputs of a case and the comparison.  The CPU file pins the references
to the golden fixtures and holds the stock fp32 oracle to a quarter (inference) / half (training) of the tolerance on every case listed
here; the GPU file holds the HIP kernels to the whole of it.

References, all in fp64:
  (a) the layer: oracle.cross_graph_attention / oracle.encoder_inference on double parameters and inputs (the oracle is dtype-agnostic).
      ``layer_fp64`` / ``encoder_fp64`` restate them graph by graph, so that [B, n, n, d] never exists; the CPU file holds the
      restatement to the oracle.
  (b) the pairwise stage alone on given fp32 Pr, Q, h, X, a, A: ``pairwise_fp64``.
Both run on the GPU (torch fp64) when there is one, as tests/test_hip_nrms.py does, and hand their result back on the CPU."""
import functools
import types
import zlib
from typing import NamedTuple

import numpy as np
import torch

from oracle import digat_oracle as O

OUT_TOL = dict(rtol=1e-5, atol=1e-5)            # tests/test_hip_parity.py's figures for the layer's output ...
ALPHA_TOL = dict(rtol=1e-5, atol=1e-6)          # ... and for alpha (atol 2e-6 there, 1e-6 here)
TRAIN_OUT_TOL = dict(rtol=2e-5, atol=2e-5, floor=0.05)      # tests/test_hip_training.py: the training forward ...
GRAD_TOL = dict(rtol=2e-4, atol=2e-6, floor=0.05)           # ... and every gradient, relative to max(|want|, 5 % of the tensor's scale)
FULL_GAIN = 8.0                                 # the largest gain on `a` of the dense training cases (see train_gain)


def close(got, want, what, rtol, atol, floor=0.0):
    """|got - want| <= atol + rtol max(|want|, floor * scale); returns the worst err / tol (floor 0: tests/test_hip_parity.py:close,
    floor 0.05: tests/test_hip_training.py:close)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    scale = max(float(np.abs(want).max()), 1e-12) if want.size else 1.0
    err = np.abs(got.astype(np.float64) - want)
    tol = atol + rtol * np.maximum(np.abs(want), floor * scale)
    ratio = float((err / tol).max()) if want.size else 0.0
    if (err > tol).any():
        idx = np.unravel_index(np.argmax(err / tol), err.shape)
        raise AssertionError(f"{what}: max|diff| {err.max():.3e} (scale {scale:.3e}), worst err/tol {ratio:.3f} at {idx}: "
                             f"got {got[idx]:.9g} want {want[idx]:.9g}")
    return ratio


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    n: int
    d: int
    B: int
    kind: str


KINDS = ("mind", "full", "identity", "none", "twins", "mixed")
# n: 1; 2; 4 | 5 and 8 | 9 the 4-node tiles; 15 | 16 | 17 the small-graph kernels' limit; 20 | 21, 32 | 33; 44 | 45 the last graph size with
# several graphs per workgroup of the tile kernel; 64 | 65 one adjacency word | two; 67 the user graph; 90; 112 | 113 the backward's
# chunk size; 127 | 128 the limit
N_LIST = (1, 2, 4, 5, 8, 9, 15, 16, 17, 20, 21, 32, 33, 44, 45, 64, 65, 67, 90, 112, 113, 127, 128)
# d: 4; 20, 36 (d / 4 odd); 64; 252 | 256 | 260 one | two float4 pieces per lane (U = 1 | 2); 400; 512 | 516 (U = 2 | 4, and the
# limit of the multi-centre kernels); 800; 1024 the wave-per-centre limit | 1028 beyond it (dense entries only)
D_LIST = (4, 20, 36, 64, 252, 256, 260, 400, 512, 516, 800, 1024)
D_DENSE_ONLY = (1028,)
N_ALL_D = (10, 16, 17, 44, 67, 128)
D_ALL_N = (36, 400)
CORNERS = ((8, 1024), (9, 1024), (15, 516), (16, 516), (16, 512), (128, 1024), (128, 4), (1, 4),
           (112, 4))       # with (128, 4): n n + 32 adjacency bytes beyond the 12 KiB ring of d = 4, staged in the score area (xattn_tile_plan)


def _shapes(with_dense_only):
    s = {(n, d) for n in N_LIST for d in D_ALL_N} | {(n, d) for n in N_ALL_D for d in D_LIST} | set(CORNERS)
    if with_dense_only:
        s |= {(n, d) for n in N_ALL_D for d in D_DENSE_ONLY}
    return sorted(s)


def _batch(n, d):
    return 1 + (7 * n + d // 4) % 3                                   # 1 .. 3 graphs, fixed per shape


SHAPES = _shapes(True)
# B = 1 and a partial last workgroup of the tile kernel with several graphs per workgroup (RB = 256 / tiles: 10 at n = 17, 2 at n = 44)
RB_EXTRA = [(17, 36, 1), (17, 36, 11), (17, 400, 11), (44, 36, 1), (44, 36, 3), (44, 400, 3)]
PAIR_CASES = [Case(n, d, _batch(n, d), k) for n, d in SHAPES for k in KINDS] + [Case(n, d, B, k) for n, d, B in RB_EXTRA for k in ("mind", "mixed")]
# the layer through DIGAT._xattn: every shape, four kinds (identity and none are rows of `mixed`; block A runs them whole)
LAYER_KINDS = ("mind", "full", "twins", "mixed")
LAYER_CASES = [Case(n, d, _batch(n, d), k) for n, d in SHAPES for k in LAYER_KINDS] + [Case(n, d, B, "mixed") for n, d, B in RB_EXTRA]
# ... and at B n >= 2048 with d % 80 == 0
LAYER_BIG = [Case(n, d, -(-2048 // n), "mixed") for n in (17, 67, 128) for d in (80, 240, 480, 800)]
PAIR_NS = sorted({c.n for c in PAIR_CASES})

# the encoder (block C): U = H + C user nodes, C = 17 topics, N = 10 news nodes, 4 groups x 8 rows, depth 3
ENC_U = (64, 65, 128)
ENC_D_LISTS = (80, 240, 320, 480)               # 4 G <= B, B U >= 2048, d % 80 == 0: the live-row lists; U = 1 (80, 240) and 2 (320, 480)
ENC_D_PLAIN = (64, 256, 516)                    # no row list; 516 is beyond the multi-centre kernels (d <= 512)
ENC_CASES = [(U, d) for U in ENC_U for d in ENC_D_LISTS + ENC_D_PLAIN]
ENC_C, ENC_N, ENC_G, ENC_ROWS, ENC_DEPTH = 17, 10, 4, 8, 3

# training (block D)
TRAIN_N = (1, 10, 16, 17, 33, 44, 45, 64, 65, 112, 113, 128)
TRAIN_D_ALL_N = (36, 256)
TRAIN_D = (4, 64, 260, 512, 516, 1024)
TRAIN_N_ALL_D = (10, 67)
TRAIN_SHAPES = sorted({(n, d) for n in TRAIN_N for d in TRAIN_D_ALL_N} | {(n, d) for n in TRAIN_N_ALL_D for d in TRAIN_D})
TRAIN_KINDS = ("mixed", "twins", "full")
TRAIN_P = (0.0, 0.3)
TRAIN_B = 2
TRAIN_CASES = [Case(n, d, TRAIN_B, k) for n, d in TRAIN_SHAPES for k in TRAIN_KINDS]
TRAIN_NONE = [Case(10, 36, 2, "none"), Case(67, 64, 2, "none"), Case(128, 36, 1, "none")]       # no centre has an entry


def train_gain(case):
    """The gain on `a` of the dense kinds (`full`, and `twins`: a history in one category is a clique): 8 up to d = 64, 64 / sqrt(d)
    beyond, so that attention over a hundred entries is far from uniform and the scores stay within what fp32 can resolve.  The
    scores are d-term sums of magnitude ~ gain: a plain fp32 chain over the channels rounds them by ~ sqrt(d) ulp(gain), the softmax
    turns that absolute error into a relative one of alpha, and at gain 8 such a chain alone spends 0.65 (d = 256) to 1.09
    (d = 1024) of the output's tolerance — while the blocked sums of the stock oracle's BLAS stay below 0.35.  tests/test_eq8_fp64_cpu.py
    holds both fp32 evaluations to half of the tolerance on every case.  The MIND-like `mixed` takes no gain."""
    return min(FULL_GAIN, 64.0 / case.d ** 0.5) if case.kind in ("full", "twins") else 1.0


# ---- adjacency -------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def twin_users(H, C):
    """(history categories [5, H], history lengths [5]) of the users of tests/test_hip_parity.py's twin-centre test: a whole history in
    one category, in another, two big categories, a one-item history — and an empty one."""
    cats = np.stack([np.zeros(H, dtype=np.int64), np.full(H, 3 % C, dtype=np.int64),
                     np.r_[np.zeros(H // 2, dtype=np.int64), np.full(H - H // 2, 1 % C, dtype=np.int64)],
                     np.full(H, 2 % C, dtype=np.int64), np.full(H, 1 % C, dtype=np.int64)])
    return cats, np.array([H, H, H, min(1, H), 0])


def _twins(n, B, rng):
    from digat_amd import synthetic
    C = max(1, min(17, n // 3))
    H = n - C
    cats, hl = twin_users(H, C)
    pick = (np.arange(B) * 2 + int(rng.integers(5))) % 5               # B <= 3 distinct users
    return synthetic.build_user_graphs(cats[pick], hl[pick], C)[0]


def _mind(n, B, rng):
    return (rng.random((B, n, n)) < min(0.6, 6.0 / n)) | np.eye(n, dtype=bool)[None]          # about 6 entries per node


def _plant(A, rng):
    """Rows of graph 0 replaced, from the last row down (so that centres beyond the first adjacency word get them): no entry; the self
    loop only; node n - 1 only; for n > 64 entries only at j >= 64 and only at j < 64; degrees 2, 3, 5, 6, 7."""
    n = A.shape[1]
    rows = []

    def put(cols):
        i = n - 1 - len(rows)
        if i < 0 or any(c < 0 or c >= n for c in cols) or len(set(cols)) != len(cols):
            return
        A[0, i] = False
        A[0, i, list(cols)] = True
        rows.append(i)
    put([])
    if n > 1:
        put([n - 2])                                                    # the centre's own column: row n - 2 is planted second
        put([n - 1])
    if n > 64:
        put(list(64 + rng.choice(n - 64, size=min(3, n - 64), replace=False)))
        put(list(rng.choice(64, size=5, replace=False)))
    for deg in (2, 3, 5, 6, 7):
        if deg <= n:
            put(list(rng.choice(n, size=deg, replace=False)))
    return A


def adjacency(kind, n, B, seed=0):
    """bool [B, n, n] of a kind of KINDS, a function of (kind, n, B, seed) alone.  Asymmetric wherever the kind allows (user graphs,
    `twins`, are symmetric by construction), so that an implementation that swaps centre and neighbour cannot pass."""
    rng = _rng("adj", kind, n, B, seed)
    if kind == "mind":
        return _mind(n, B, rng)
    if kind == "full":
        return np.ones((B, n, n), dtype=bool)
    if kind == "identity":                                              # degree 1: graph b links centre i to node (i + b + 1) % n alone
        A = np.zeros((B, n, n), dtype=bool)
        for b in range(B):
            A[b, np.arange(n), (np.arange(n) + b + 1) % n] = True
        return A
    if kind == "none":
        return np.zeros((B, n, n), dtype=bool)
    if kind == "twins":
        return _twins(n, B, rng)
    if kind == "mixed":
        return _plant(_mind(n, B, rng), rng)
    raise ValueError(kind)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def pair_inputs(case):
    """fp32 (Pr, Q, h, X, a [d], A uint8) of a Case for the pairwise stage: no GEMM is involved."""
    n, d, B, kind = case
    rng = _rng("pair", *case)
    f = lambda *s: torch.from_numpy((0.5 * rng.standard_normal(s)).astype(np.float32))
    Pr, Q, h, X = f(B, n, d), f(B, n, d), f(B, n, d), f(B, n, d)
    a = torch.from_numpy((rng.standard_normal(d) * d ** -0.5).astype(np.float32))
    return Pr, Q, h, X, a, torch.from_numpy(adjacency(kind, n, B).astype(np.uint8))


@functools.lru_cache(maxsize=2)
def layer_state(d):
    """DIGAT parameters at width d (one layer, three topics): a function of d, shared by every case of that width."""
    from digat_amd import synthetic
    return synthetic.make_state_dict(d, 3, 1, seed=1000 + d, bias_std=0.05)


def layer_inputs(case):
    """fp32 (X [B, n, d], ctx [B, d], A bool [B, n, n]) of a Case for the layer (graph "user", layer 0 of layer_state(d))."""
    n, d, B, kind = case
    rng = _rng("layer", *case)
    X = torch.from_numpy((0.5 * rng.standard_normal((B, n, d))).astype(np.float32))
    ctx = torch.from_numpy((0.5 * rng.standard_normal((B, d))).astype(np.float32))
    return X, ctx, torch.from_numpy(adjacency(kind, n, B))


def layer_encoder(d, device):
    from digat_amd.graphEncoders import DIGAT
    cfg = types.SimpleNamespace(news_graph_size=10, max_history_num=7, category_num=3, graph_depth=1, dropout_rate=0.2)
    enc = DIGAT(cfg, d)
    res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in layer_state(d).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return enc.to(device).eval()


TRAIN_NAMES = {"W": "W.0.weight", "bW": "W.0.bias", "F1": "ffn1.0.weight", "F2": "ffn2.0.weight", "F3": "ffn3.0.weight", "b3": "ffn3.0.bias",
               "a": "a.0.weight"}


# Cases whose first draw missed the fp32 oracle's half of the tolerance (tests/test_eq8_fp64_cpu.py) and took another seed, as that
# condition asks
TRAIN_RESEED = {Case(10, 4, 2, "full"): 3, Case(67, 4, 2, "full"): 5}    # d = 4: F2 / F3 / b3 gradients of four-term sums at 0.5 - 1.14 of the tolerance


@functools.lru_cache(maxsize=4)
def train_inputs(case):
    """fp32 (X, ctx, cotangent, A bool, weights {W, bW, F1, F2, F3, b3, a}) of a training Case, as tests/test_hip_training.py draws them,
    `a` times train_gain(case).  Cached: callers leave them unchanged."""
    n, d, B, kind = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(("train",) + tuple(case) + ((TRAIN_RESEED[case],) if case in TRAIN_RESEED else ())).encode()))
    X, ctx, dOut = torch.randn(B, n, d, generator=g), torch.randn(B, d, generator=g), torch.randn(B, n, d, generator=g)
    w = {k: torch.randn(*shape, generator=g) * scale for k, shape, scale in
         [("W", (d, d), d ** -0.5), ("bW", (d,), 0.1), ("F1", (d, d), d ** -0.5), ("F2", (d, d), d ** -0.5), ("F3", (d, d), d ** -0.5),
          ("b3", (d,), 0.1), ("a", (1, d), d ** -0.5 * train_gain(case))]}
    A = torch.from_numpy(adjacency(kind, n, B))
    _keep_off_the_kinks(X, ctx, A, w, train_gain(case))
    return X, ctx, dOut, A, w


KINK_MARGIN = 1e-5      # of O(1) pre-activations: some thirty times what fp32 rounding moves a d = 1024 dot product of O(1) by
SCORE_MARGIN = 2e-6     # of the sum of |a_c| relu(.): ten times what the rounding of the addends (2e-6 each, random signs) and of the sum moves it by
DROP_SEED = 4242        # the attention dropout's seed of every training case


def _keep_off_the_kinks(X, ctx, A, w, gain):
    """Moves b3, a and bW (in place, by a few 1e-4) until, in fp64, no pre-activation that reaches a gradient lies within KINK_MARGIN of
    the kink of its relu / leaky_relu: K3 + K1 + K2 on the adjacency entries, the scores on them and alpha @ h with and without the
    attention dropout of TRAIN_P (these two relative to the sum of the magnitudes of their terms).  A training case is a condition on its inputs: fp32 rounding that
    flips one such derivative changes a weight gradient that sums a few hundred rows by percents — in the fp32 oracle as in a kernel,
    each at the elements its own summation order picks — and the up to 9 M pre-activations of a dense case always hold a few within
    1e-6 of zero.  Off the kinks the function is smooth and the tolerances measure arithmetic."""
    Xd, cd, Ab = X.double(), ctx.double(), A.bool()
    wd = {k: v.double() for k, v in w.items()}
    K1, K2, K3 = Xd @ wd["F1"].T, Xd @ wd["F2"].T, cd @ wd["F3"].T                                  # K3 without b3
    inf = float("inf")

    def z_channel(c, b3c):                                                                          # [B, i, j]
        return (K3[:, c] + b3c).view(-1, 1, 1) + K1[:, :, c].unsqueeze(1) + K2[:, :, c].unsqueeze(2)

    def z_all():
        return (K3 + w["b3"].double()).view(K3.shape[0], 1, 1, -1) + K1.unsqueeze(1) + K2.unsqueeze(2)

    near = z_all().abs().masked_fill(~Ab.unsqueeze(3), inf).amin(dim=(0, 1, 2)) < KINK_MARGIN
    for c in torch.nonzero(near).flatten().tolist():
        for t in range(1, 200):
            cand = float(np.float32(float(w["b3"][c]) + (t if t % 2 else -t) * 37 * KINK_MARGIN))
            if float(z_channel(c, cand).abs().masked_fill(~Ab, inf).min()) >= KINK_MARGIN:
                w["b3"][c] = cand
                break
        else:
            raise AssertionError("no b3 keeps K3 + K1 + K2 off zero")
    relu_z = torch.relu(z_all())
    a0 = w["a"].clone()
    for t in range(200):
        if t:
            w["a"].copy_(a0)
            w["a"][0, (t - 1) % a0.shape[1]] += 1e-3 * gain * a0.shape[1] ** -0.5 * (1 + t // a0.shape[1])
        s, mag = relu_z @ w["a"].double().view(-1), relu_z @ w["a"].double().abs().view(-1)
        # relative to the sum of magnitudes: what rounding moves a sum by (a score of closed relus alone is exactly zero, and inert)
        if bool((s.abs() >= SCORE_MARGIN * mag).masked_fill(~Ab, True).all()):
            break
    else:
        raise AssertionError("no `a` keeps the scores off zero")
    alpha = torch.softmax(torch.nn.functional.leaky_relu(s, 0.2).masked_fill(~Ab, O.MASK_FILL), dim=2)
    alphas = [alpha if p == 0 else O.hash_dropout(alpha.contiguous(), p, DROP_SEED) for p in TRAIN_P]
    h = Xd @ wd["W"].T                                                                              # without bW
    rows = [al.sum(dim=2) for al in alphas]
    for c in range(h.shape[2]):
        ys = [(al @ h[:, :, c].unsqueeze(2)).squeeze(2) for al in alphas]                           # [B, n] each
        mags = [(al @ h[:, :, c].abs().unsqueeze(2)).squeeze(2) for al in alphas]
        for t in range(200):
            cand = float(np.float32(float(w["bW"][c]) + ((t + 1) // 2 * (1 if t % 2 else -1)) * 37 * KINK_MARGIN))
            # relative to the sum of magnitudes (a row whose every entry was dropped is exactly zero in any arithmetic)
            if all(bool(((y + cand * r).abs() >= KINK_MARGIN * (m + abs(cand) * r)).all()) for y, m, r in zip(ys, mags, rows)):
                w["bW"][c] = cand
                break
        else:
            raise AssertionError("no bW keeps alpha @ h off zero")


def sequential_forward_fp32(case, p_alpha):
    """The training forward in fp32 with the score a . relu(K3 + K1 + K2) summed as one chain over the channels — the plain loop, and
    the order a kernel with a running sum takes — where the stock oracle's F.linear sums in blocks."""
    F = torch.nn.functional
    X, ctx, _, A, w = train_inputs(case)
    with torch.no_grad():
        K1, K2 = F.linear(X, w["F1"]).unsqueeze(1), F.linear(X, w["F2"]).unsqueeze(2)
        t = F.relu(F.linear(ctx, w["F3"], w["b3"]).view(-1, 1, 1, X.shape[2]) + K1 + K2) * w["a"].view(-1)
        s = torch.zeros(t.shape[:3])
        for c in range(t.shape[3]):
            s = s + t[..., c]
        alpha = F.softmax(F.leaky_relu(s, 0.2).masked_fill(A == 0, O.MASK_FILL), dim=2)
        if p_alpha > 0:
            alpha = O.hash_dropout(alpha.contiguous(), p_alpha, DROP_SEED)
        return F.relu(torch.bmm(alpha, F.linear(X, w["W"], w["bW"]))) + X


def train_params(w, dtype):
    """The oracle's parameter dictionary of train_inputs' weights as leaves of ``dtype`` that require a gradient."""
    return {"user_graph_attention_" + TRAIN_NAMES[k]: v.detach().to(dtype).clone().requires_grad_(True) for k, v in w.items()}


def train_reference(case, dtype, p_alpha, seed=DROP_SEED):
    """(output, {X, ctx, W, bW, F1, F2, F3, b3, a: gradient}) of oracle.cross_graph_attention in ``dtype`` under autograd, the
    attention dropout drawn from the kernels' hash (oracle.hash_dropout)."""
    X, ctx, dOut, A, w = train_inputs(case)
    p = train_params(w, dtype)
    Xo, co = X.detach().to(dtype).clone().requires_grad_(True), ctx.detach().to(dtype).clone().requires_grad_(True)
    drop = (lambda x, frac: x if frac == 0.5 else O.hash_dropout(x.contiguous(), p_alpha, seed)) if p_alpha > 0 else None
    out = O.cross_graph_attention(p, "user", 0, Xo, A, co, drop=drop)
    (out * dOut.to(dtype)).sum().backward()
    grads = {"X": Xo.grad, "ctx": co.grad, **{k: p["user_graph_attention_" + TRAIN_NAMES[k]].grad for k in w}}
    return out.detach(), grads


SCORE_PATH = ("ctx", "F1", "F2", "F3", "b3", "a")       # the gradients that pass through the scores


def assert_well_conditioned(case, grads):
    """Every reference gradient's largest element is above 1e-3 of the scale of the tensor it belongs to: the 5 % floor of the
    comparison is then a floor under real signal.  A single node attends to itself with weight one whatever its score, and a centre
    without an entry attends uniformly: nothing reaches the scores there, and those gradients are exactly zero."""
    X, ctx, _, A, w = train_inputs(case)
    scale = {"X": X, "ctx": ctx, **w}
    inert = case.n == 1 or not bool(A.any())
    for k, g in grads.items():
        if inert and k in SCORE_PATH:
            assert float(g.abs().max()) == 0.0, (case, k)
        else:
            assert float(g.abs().max()) > 1e-3 * float(scale[k].abs().max()), (case, k, float(g.abs().max()), float(scale[k].abs().max()))


def encoder_inputs(U, d):
    """(state, batch) of a block C case: ENC_G groups of `twins` users (a history in one category, two big categories, a one-item
    history, an empty history), ENC_ROWS candidate rows each; the four user tensors once per group, ``row_group`` [B]."""
    from digat_amd import synthetic
    H, C, G = U - ENC_C, ENC_C, ENC_G
    B = G * ENC_ROWS
    seed = zlib.crc32(repr(("enc", U, d)).encode()) % (1 << 30)
    state = synthetic.make_state_dict(d, C, ENC_DEPTH, seed=seed, bias_std=0.05)
    batch = synthetic.make_encoder_batch(B, ENC_N, H, C, d, seed=seed + 1)
    cats, hl = twin_users(H, C)
    pick = [0, 2, 3, 4]
    g, cm, ci = synthetic.build_user_graphs(cats[pick], hl[pick], C)
    rng = np.random.default_rng(seed + 2)
    batch.update(user_graph=g, user_category_mask=cm, user_category_indices=ci,
                 user_news_embedding=(0.5 * rng.standard_normal((G, H, d))).astype(np.float32),
                 row_group=np.repeat(np.arange(G, dtype=np.int32), ENC_ROWS))
    return state, batch


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_device():
    return torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")


def pairwise(Pr, Q, h, X, a, A, dtype=torch.float64):
    """Reference (b) in ``dtype``: s_ij = a . relu(Pr_j + Q_i) (i the centre, j the neighbour), leaky_relu(0.2), -1e9 where A_ij = 0,
    softmax over j, out = relu(alpha @ h) + X.  One graph at a time; returns (out, alpha) on the CPU."""
    dev = ref_device()
    Pr, Q, h, X, a = (t.to(dev, dtype) for t in (Pr, Q, h, X, a.reshape(-1)))
    A = A.to(dev)
    out, alpha = torch.empty_like(X), torch.empty(A.shape, dtype=dtype, device=dev)
    for b in range(X.shape[0]):
        s = torch.relu(Pr[b].unsqueeze(0) + Q[b].unsqueeze(1)) @ a                       # [i, j]
        e = torch.nn.functional.leaky_relu(s, 0.2).masked_fill(A[b] == 0, O.MASK_FILL)
        alpha[b] = torch.softmax(e, dim=1)
        out[b] = torch.relu(alpha[b] @ h[b]) + X[b]
    return out.cpu(), alpha.cpu()


def pairwise_fp64(Pr, Q, h, X, a, A):
    return pairwise(Pr, Q, h, X, a, A, torch.float64)


def _f64(p):
    return {k: torch.as_tensor(v).double() for k, v in p.items()}


def layer_fp64(state, graph, layer, X, A, ctx):
    """Reference (a) for one layer: the projections in fp64 (K3 + K1 summed first, as oracle.cross_graph_attention evaluates it), then
    reference (b).  Returns (out, alpha) in fp64."""
    p, pre = _f64(state), f"{graph}_graph_attention_"
    lin = lambda x, name: torch.nn.functional.linear(x, p[f"{pre}{name}.{layer}.weight"], p.get(f"{pre}{name}.{layer}.bias"))
    X, ctx = X.double().cpu(), ctx.double().cpu()
    Pr = lin(ctx, "ffn3").unsqueeze(1) + lin(X, "ffn1")
    return pairwise_fp64(Pr, lin(X, "ffn2"), lin(X, "W"), X, p[f"{pre}a.{layer}.weight"], torch.as_tensor(A))


def encoder_fp64(state, depth, Xn, An, Mn, ue, Au, cm, ci, c_n):
    """oracle.encoder_inference in fp64 with its two Eq. 8 calls per layer through layer_fp64 (the contexts are the oracle's own
    functions on double parameters)."""
    p = _f64(state)
    Xn, ue, c_n = (torch.as_tensor(t).double() for t in (Xn, ue, c_n))
    An, Mn, Au, cm, ci = (torch.as_tensor(t) for t in (An, Mn, Au, cm, ci))
    H = ue.shape[1]
    Xu = O.user_nodes(p, ue)
    c_u = O.user_graph_context(p, Xu, cm, ci, c_n, H)
    for i in range(depth):
        Xn, Xu = layer_fp64(p, "news", i, Xn, An, c_u)[0], layer_fp64(p, "user", i, Xu, Au, c_n)[0]
        c_n = c_n + O.news_graph_context(p, Xn, Mn)
        c_u = c_u + O.user_graph_context(p, Xu, cm, ci, c_n, H)
    return c_n, c_u
