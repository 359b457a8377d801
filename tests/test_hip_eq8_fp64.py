"""GPU suite: Eq. 8, the dual-interaction attention layer (csrc/digat_xattn.inc and the Eq. 8 part of csrc/digat_train.inc), against fp64
references over every kernel variant, graph size and width at which the code changes its path (the case lists and what each is chosen
for: tests/eq8_fp64_common.py).  tests/test_eq8_fp64_cpu.py pins the references to the golden fixtures and holds fp32 arithmetic alone
(the stock oracle) to a quarter (inference) / half (training) of the tolerances used here.

  A  the pairwise kernels alone (digat_xattn_pairwise_fwd on random fp32 Pr, Q, h, X, a: no GEMM), every shape with every adjacency kind
  B  the layer through DIGAT._xattn: with alpha (score kernels + aggregation), without (the fused small-graph kernel up to 16 nodes)
     and in sparse mode (digat_xattn_fwd_mode, xattn_sparse_kernel<U, 0, false>), each against the reference on its own
  C  the variants only the encoder reaches (K3 added in the kernel, the layer-0 chunk kernel, the twin kernel, group indirection):
     inference_grouped in sparse mode on `twins` users, in both operand formats
  D  training.XattnFused, entry-wise and all-pairs, with and without attention dropout, against fp64 autograd

Tolerances are the project's: out rtol 1e-5 / atol 1e-5, alpha 1e-5 / 1e-6 (tests/test_hip_parity.py), the training forward 2e-5 / 2e-5 and
every gradient 2e-4 / 2e-6 relative to max(|want|, 5 % of the tensor's scale) (tests/test_hip_training.py).  Workspaces are filled with
0xFF bytes — NaN as floats — before every call, outputs handed to the C ABI directly (block A) are NaN-filled, and every result must
be finite.  The training pair runs through both bindings: the torch extension allocates `save` and its scratch in C++, so the ctypes
twin, which takes them from digat_amd._lib, is the run whose `save` and scratch arrive filled with 0xFF (asserted in _train).

Worst err / tol per block, measured on an MI355X (every figure is to stay below 1; nothing is tuned to them):
    A  pairwise kernels      out 0.043 (n = 10), alpha 0.060 (n = 44)
    B  layer entries         out 0.207 (n = 128), alpha 0.313 (n = 44); 0.201 / 0.288 from 2 048 rows; permutation and 0xFF workspace bit-identical
    C  encoder variants      0.242 in both formats (U = 128, d = 516); on the row lists 0.191 (bf16x6) / 0.166 (fp16x3); live_rows=False bit-identical
    D  training              output 0.285, gradients 0.276 (n = 64, d = 256); centres without an entry: exact zeros on the score path
The stock fp32 oracle on a CPU, held to 0.25 (A - C) and 0.5 (D) on the same cases by tests/test_eq8_fp64_cpu.py, reaches 0.016 / 0.021
(A, the pairwise stage in fp32), 0.112 / 0.104 (B), 0.224 (C) and 0.339 / 0.214 (D): the kernels are about as far from fp64 as fp32 is.
"""
import functools
import types

import numpy as np
import pytest
import torch

import eq8_fp64_common as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _poison(byte=0xFF):
    """Every cached workspace of the library calls (digat_amd._lib.workspace) filled with ``byte``."""
    from digat_amd import _lib
    for buf in _lib._workspaces.values():
        buf.fill_(byte)


def _report(block, what, cases, **worst):
    print(f"[{block}] {what}: worst err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" over {cases} cases")


# ---- A: the pairwise kernels alone ----------------------------------------------------------------------------------------------
def _pairwise(case):
    from digat_amd import _lib
    n, d, B, _ = case
    ins = C.pair_inputs(case)
    Pr, Q, h, X, a, A = (t.to(_dev()).contiguous() for t in ins)
    out, alpha = torch.full_like(X, float("nan")), torch.full((B, n, n), float("nan"), device=_dev())
    _poison()
    _lib.check(_lib.lib().digat_xattn_pairwise_fwd(Pr.data_ptr(), Q.data_ptr(), h.data_ptr(), X.data_ptr(), a.data_ptr(), A.data_ptr(),
                                                   out.data_ptr(), alpha.data_ptr(), B, n, d, _lib.stream_ptr()), f"digat_xattn_pairwise_fwd {case}")
    torch.cuda.synchronize()
    want, want_alpha = C.pairwise_fp64(*ins)
    o = C.close(out, want, f"pairwise {case} out", **C.OUT_TOL)
    al = C.close(alpha, want_alpha, f"pairwise {case} alpha", **C.ALPHA_TOL)
    got, adj = alpha.cpu().double(), ins[5].bool()
    has = adj.any(dim=2)
    assert bool((got[has.unsqueeze(2) & ~adj] == 0).all()), f"{case}: alpha off the adjacency"
    assert float((got.sum(dim=2) - 1).abs().max()) <= 1e-6, f"{case}: alpha rows sum to 1 +- {float((got.sum(dim=2) - 1).abs().max()):.2e}"
    if bool((~has).any()):
        assert float((got[~has] * n - 1).abs().max()) <= 1e-6, f"{case}: a row without an entry is not 1 / n"
    return o, al


@pytest.mark.parametrize("n", C.PAIR_NS)
def test_pairwise_kernels_against_fp64(n):
    cases = [c for c in C.PAIR_CASES if c.n == n]
    res = [_pairwise(c) for c in cases]
    _report("A", f"pairwise n={n}", len(cases), out=max(r[0] for r in res), alpha=max(r[1] for r in res))


# ---- B: the layer through the public entries -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _layer_encoder(d):
    return C.layer_encoder(d, _dev())


def _layer(case):
    """(worst err/tol of out over the entries, of alpha)"""
    n, d, B, _ = case
    enc = _layer_encoder(d)
    X, ctx, A = C.layer_inputs(case)
    want, want_alpha = C.layer_fp64(C.layer_state(d), "user", 0, X, A, ctx)
    Xd, cd, Ad = X.to(_dev()), ctx.to(_dev()), A.to(_dev())
    perm = torch.arange(B - 1, -1, -1, device=_dev())
    worst = 0.0

    def call(mode, Xc=Xd, cc=cd, Ac=Ad, fill=0xFF, **kw):
        enc.user_xattn_mode = mode
        _poison(fill)
        with torch.no_grad():
            return enc._xattn("user", 0, Xc, Ac, cc, **kw)
    out, alpha = call("dense", return_alpha=True)                     # digat_xattn_fwd: score kernels + aggregation
    worst = max(worst, C.close(out, want, f"layer {case} with alpha", **C.OUT_TOL))
    al = C.close(alpha, want_alpha, f"layer {case} alpha", **C.ALPHA_TOL)
    again = call("dense", fill=0x00, return_alpha=True)
    assert _same_bits(again[0], out) and _same_bits(again[1], alpha), f"{case} with alpha: the workspace's contents reach the output"
    if B > 1:
        moved = call("dense", Xd[perm].contiguous(), cd[perm].contiguous(), Ad[perm].contiguous(), return_alpha=True)
        assert _same_bits(moved[0], out[perm]) and _same_bits(moved[1], alpha[perm]), f"{case} with alpha: permuting the graphs does not permute the bits"
    modes = ["dense"] + (["sparse"] if n > 16 and d <= 1024 else [])   # without alpha: the fused small-graph kernel up to 16 nodes; sparse: digat_xattn_fwd_mode
    for mode in modes:
        got = call(mode)
        worst = max(worst, C.close(got, want, f"layer {case} {mode}", **C.OUT_TOL))
        assert _same_bits(call(mode, fill=0x00), got), f"{case} {mode}: the workspace's contents reach the output"
        if B > 1:
            assert _same_bits(call(mode, Xd[perm].contiguous(), cd[perm].contiguous(), Ad[perm].contiguous()), got[perm]), \
                f"{case} {mode}: permuting the graphs does not permute the output bits"
    torch.cuda.synchronize()
    return worst, al


@pytest.mark.parametrize("n", C.PAIR_NS)
def test_layer_entries_against_fp64(n):
    cases = sorted((c for c in C.LAYER_CASES if c.n == n), key=lambda c: c.d)
    res = [_layer(c) for c in cases]
    _report("B", f"layer n={n}", len(cases), out=max(r[0] for r in res), alpha=max(r[1] for r in res))


@pytest.mark.parametrize("case", C.LAYER_BIG, ids=lambda c: f"n{c.n}-d{c.d}-B{c.B}")
def test_layer_entries_from_2048_rows_against_fp64(case):
    """B n >= 2048 and d % 80 == 0: the projections' strip kernels."""
    o, al = _layer(case)
    _report("B", f"layer {case}", 1, out=o, alpha=al)


# ---- C: the variants only the encoder reaches ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _encoder_case(U, d):
    """(state, device inputs of inference_grouped, fp64 reference) of a block C case, shared by the two operand formats."""
    from oracle import digat_oracle as O
    state, b = C.encoder_inputs(U, d)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(b[k]))
    rg = t("row_group").long()
    keys = ("news_graph_embeddings", "news_graph", "news_graph_mask", "user_news_embedding", "user_graph", "user_category_mask", "user_category_indices")
    with torch.no_grad():
        c0 = O.news_graph_context({k: torch.from_numpy(v).double() for k, v in state.items()}, t(keys[0]).double(), t(keys[2])).float()
        want = C.encoder_fp64(state, C.ENC_DEPTH, *(t(k) for k in keys[:3]), *(t(k)[rg] for k in keys[3:]), c0)
    args = [t(k).to(_dev()) for k in keys] + [t("row_group").to(_dev()), c0.to(_dev())]
    return state, args, want


@pytest.mark.parametrize("pm", ["bf16x6", "fp16x3"])
@pytest.mark.parametrize("U,d", C.ENC_CASES)
def test_encoder_only_variants_against_fp64(U, d, pm):
    from digat_amd import _lib
    from digat_amd.graphEncoders import DIGAT
    state, args, want = _encoder_case(U, d)
    cfg = types.SimpleNamespace(news_graph_size=C.ENC_N, max_history_num=U - C.ENC_C, category_num=C.ENC_C, graph_depth=C.ENC_DEPTH, dropout_rate=0.2)
    enc = DIGAT(cfg, d)
    res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    enc = enc.to(_dev()).eval()
    enc.user_xattn_mode, enc.projection_mode = "sparse", pm
    with torch.no_grad():
        enc.inference_grouped(*args)                                   # allocates the workspace, builds the weight images
        _poison()
        _lib.profile_start()
        got = enc.inference_grouped(*args)
        torch.cuda.synchronize()
        parts = {k: v["launches"] for k, v in _lib.profile_stop()["xattn"]["parts"].items()}
        with enc.launch_options(live_rows=False):
            _poison()
            _lib.profile_start()
            every = enc.inference_grouped(*args)
            torch.cuda.synchronize()
            parts_off = {k: v["launches"] for k, v in _lib.profile_stop()["xattn"]["parts"].items()}
    worst = max(C.close(g, w, f"encoder U={U} d={d} {pm} {name}", **C.OUT_TOL) for g, w, name in zip(got, want, ("news", "user")))
    assert all(_same_bits(a, b) for a, b in zip(got, every)), "live_rows=False changes bits"
    print(f"[C] U={U} d={d} {pm}: Eq. 8 launches {parts}, without the live lists {parts_off}")
    # "l0" / "twin" count the Eq. 8 launches through the group index / on the live-row lists (digat_kernels.hip, XPART_*), whichever
    # kernel serves them: the chunk kernel or a wave per centre (beyond d = 512: xattn_sparse_kernel<4, 0, true>), the twin kernel or
    # a wave per live centre.  The counters name the route, not the kernel; which kernel a route takes is the plan's
    # (digat_encoder_plan.h: l0_chunked, twins).  Layer 0 of grouped rows always goes through the group index; layers 1 and 2 run
    # on the lists only where the projection takes a row list, d % 80 == 0; without live rows neither route exists.
    assert parts["l0"] == 1 and parts["twin"] == (2 if d in C.ENC_D_LISTS else 0) and parts["other"] == (0 if d in C.ENC_D_LISTS else 2), parts
    assert parts_off["l0"] == 0 and parts_off["twin"] == 0 and parts_off["other"] == 3, parts_off
    _report("C", f"encoder U={U} d={d} {pm}", 1, out=worst)


# ---- D: training -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _train_reference(case, p_alpha):
    out, grads = C.train_reference(case, torch.float64, p_alpha)
    C.assert_well_conditioned(case, grads)
    return out, grads


def _train(case, mode, p_alpha, monkeypatch, poisoned):
    """(worst err/tol of the output, of the gradients, the gradients).  ``poisoned``: through the ctypes twin of the binding, whose
    `save` and scratch are allocated in Python (_lib.save_buffer, _lib.workspace) and are handed over filled with 0xFF bytes at
    every request; else through the torch extension (the default binding), which allocates both in C++ out of this file's reach."""
    from digat_amd import _lib, training
    X, ctx, dOut, A, w = C.train_inputs(case)
    want, wgrads = _train_reference(case, p_alpha)
    filled = {"save": 0, "workspace": 0}
    with monkeypatch.context() as m:
        m.setattr(training, "_seed", lambda: C.DROP_SEED)
        m.setattr(_lib, "USE_TORCH_EXT", not poisoned)
        if poisoned:
            plain = _lib.workspace

            def save_buffer(nbytes, device):
                filled["save"] += 1
                return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=device)

            def workspace(nbytes, device, tag=""):
                filled["workspace"] += 1
                return plain(nbytes, device, tag).fill_(0xFF)
            m.setattr(_lib, "save_buffer", save_buffer)
            m.setattr(_lib, "workspace", workspace)
        else:
            assert _lib.ext() is not None, "the torch extension is not built"
        dv = {k: v.to(_dev()).requires_grad_(True) for k, v in w.items()}
        Ab = A.to(torch.uint8).to(_dev()).contiguous()
        Xd, cd = X.to(_dev()).requires_grad_(True), ctx.to(_dev()).requires_grad_(True)
        out = training.XattnFused.apply(Xd, Ab, cd, dv["W"], dv["bW"], dv["F1"], dv["F2"], dv["F3"], dv["b3"], dv["a"], p_alpha, None, 0.0, mode)
        (out * dOut.to(_dev())).sum().backward()
        torch.cuda.synchronize()
    if poisoned:                                                       # forward: `save` and the scratch; backward: the scratch again
        assert filled["save"] >= 1 and filled["workspace"] >= 2, filled
    what = f"training {case} mode {mode} p {p_alpha} {'ctypes, poisoned' if poisoned else 'extension'}"
    o = C.close(out, want, f"{what} out", **C.TRAIN_OUT_TOL)
    got = {"X": Xd.grad, "ctx": cd.grad, **{k: dv[k].grad for k in w}}
    g = max(C.close(got[k], wgrads[k], f"{what} grad {k}", **C.GRAD_TOL) for k in wgrads)
    return o, g, got


@pytest.mark.parametrize("n,d", C.TRAIN_SHAPES)
def test_training_pair_against_fp64_autograd(n, d, monkeypatch):
    """Entry-wise (1) and all-pairs (2) — beyond d = 512 the backward is all-pairs whatever the mode — with the attention dropout off
    and live under the oracle's hash masks, each through both bindings (see _train)."""
    cases = [c for c in C.TRAIN_CASES if (c.n, c.d) == (n, d)]
    res = [_train(c, mode, p, monkeypatch, poisoned)[:2] for c in cases for p in C.TRAIN_P for mode in (1, 2) for poisoned in (False, True)]
    _report("D", f"training n={n} d={d}", len(res), out=max(r[0] for r in res), gradients=max(r[1] for r in res))


@pytest.mark.parametrize("case", C.TRAIN_NONE, ids=lambda c: f"n{c.n}-d{c.d}")
def test_centres_without_an_entry_send_no_gradient_to_the_scores(case, monkeypatch):
    """-1e9 replaces every score of such a centre: its attention is uniform whatever the scores, so nothing reaches K1, K2, K3 or `a`,
    while the uniform aggregation still carries the gradient to W and X."""
    for p in C.TRAIN_P:
        for mode in (1, 2):
            for poisoned in (False, True):
                o, g, got = _train(case, mode, p, monkeypatch, poisoned)
                for k in C.SCORE_PATH:
                    assert float(got[k].abs().max()) == 0.0, (case, mode, p, poisoned, k)
                assert float(got["W"].abs().max()) > 0.0 and float(got["X"].abs().max()) > 0.0
    _report("D", f"training {case}", 8, out=o, gradients=g)
