"""CPU half of the training step's fp64 sweeps (tests/test_hip_step_fp64.py is the GPU half; the case lists, references and
tolerances: tests/step_fp64_common.py).  Three things are held here:
  * the fp64 restatements equal the functions they restate to 1e-12 on double inputs — gat_fp64 and oracle.gat_layer (and, in
    oracle.gat_layer's place, it reproduces the vectors minted from the reference's own ablation encoder,
    tests/golden/ablation_wo_interaction_*.npz), loss_eval and oracle.training_loss, adam_fp64_step and clip_grad_norm_ +
    torch.optim.Adam on double tensors;
  * on every case the GPU file runs, the stock fp32 formulation alone — oracle.gat_layer, F.embedding's backward, torch.log_softmax,
    clip_grad_norm_ + torch.optim.Adam — stays within HALF of the tolerance the kernels are granted: a condition on the inputs of
    a case, so that the tolerance is not already spent by the number format;
  * the coverage the case lists are chosen for, in code: the U each dm takes, the levels each M takes, the chunks that are one
    open run at the second level, the id patterns of the unsorted lists, the centres `mixed` keeps, more than 1024 chunks."""
import numpy as np
import pytest
import torch

import step_fp64_common as C
from conftest import load_golden
from oracle import digat_oracle as O

HALF = C.HALF
F = torch.nn.functional


# ---- the restatements against what they restate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [C.Case(10, 36, 3, "mixed"), C.Case(67, 64, 2, "mixed"), C.Case(128, 36, 2, "twins"), C.Case(17, 4, 2, "none"),
                                  C.Case(65, 260, 1, "full")], ids=lambda c: f"n{c.n}-d{c.d}-{c.kind}")
def test_gat_fp64_equals_the_oracle_on_double_inputs(case):
    X, _, A, w = C.gat_inputs(case)
    p = {"user_graph_attention_" + k: v.double() for k, v in (("W.0.weight", w["W"]), ("W.0.bias", w["bW"]), ("a1.0.weight", w["a1"]),
                                                              ("a2.0.weight", w["a2"]))}
    want = O.gat_layer(p, "user", 0, X.double(), A)
    got = C.gat_fp64(X.double(), A, w["W"].double(), w["bW"].double(), w["a1"].double(), w["a2"].double())
    assert want.dtype == got.dtype == torch.float64
    assert C.close(got, want, "gat_fp64", rtol=1e-12, atol=1e-12) <= 1.0
    # the hook: p = 0.3 under the kernels' keep bits equals the oracle's lines with hash_dropout between softmax and bmm
    h = F.linear(X.double(), p["user_graph_attention_W.0.weight"], p["user_graph_attention_W.0.bias"])
    e = F.leaky_relu(F.linear(h, p["user_graph_attention_a1.0.weight"]).view(case.B, 1, case.n) + F.linear(h, p["user_graph_attention_a2.0.weight"]), 0.2)
    alpha = O.hash_dropout(F.softmax(e.masked_fill(A == 0, O.MASK_FILL), dim=2).contiguous(), 0.3, C.GAT_SEED)
    got = C.gat_fp64(X.double(), A, w["W"].double(), w["bW"].double(), w["a1"].double(), w["a2"].double(), drop=C.gat_drop(0.3))
    assert C.close(got, F.relu(torch.bmm(alpha, h)) + X.double(), "gat_fp64 with dropout", rtol=1e-12, atol=1e-12) <= 1.0


@pytest.mark.parametrize("tag", ["tiny", "default"])
def test_gat_fp64_reproduces_reference_vectors(tag, monkeypatch):
    """oracle.ablation_encode("wo_interaction") with gat_fp64 on double parameters in oracle.gat_layer's place against the vectors minted
    from the reference's own class (tests/test_oracle_golden.py holds the fp32 oracle to them)."""
    from digat_amd import synthetic
    fx = load_golden(f"ablation_wo_interaction_{tag}.npz")
    B, N, H, Ct, d, L = (int(v) for v in fx["meta"])
    s_w, s_b = (int(v) for v in fx["seeds"])
    state = synthetic.make_ablation_state_dict("wo_interaction", d, Ct, L, seed=s_w)
    batch = synthetic.make_encoder_batch(B, N, H, Ct, d, seed=s_b, empty_history_rows=(1,), isolated_news_rows=(2,))
    tot = sum(float(np.asarray(v, dtype=np.float64).sum()) for v in list(batch.values()) + list(state.values()))
    assert abs(tot - float(fx["input_checksum"])) < 1e-6 * max(1.0, abs(tot)), "regenerated inputs differ from the minted ones"
    calls = []

    def layer(p, graph, i, X, adj):
        calls.append(graph)
        pre = f"{graph}_graph_attention_"
        return C.gat_fp64(X, adj, p[f"{pre}W.{i}.weight"], p[f"{pre}W.{i}.bias"], p[f"{pre}a1.{i}.weight"], p[f"{pre}a2.{i}.weight"])
    monkeypatch.setattr(O, "gat_layer", layer)
    p = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in state.items()}
    b = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    fn, fu = O.ablation_encode("wo_interaction", p, L, b["news_graph_embeddings"].double(), b["news_graph"], b["news_graph_mask"],
                               b["user_news_embedding"].double(), b["user_graph"], b["user_category_mask"], b["user_category_indices"])
    assert len(calls) == 2 * L and fn.dtype == fu.dtype == torch.float64
    np.testing.assert_allclose(fn.numpy(), fx["out_forward_news"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(fu.numpy(), fx["out_forward_user"], rtol=1e-5, atol=1e-5)


def test_loss_eval_equals_the_oracle_and_adam_fp64_equals_torch_on_double_tensors():
    x = C.loss_inputs(257, 5, "x30")
    loss, _ = C.loss_eval(x)
    assert abs(float(loss) - float(O.training_loss(x.double()))) <= 1e-12 * abs(float(loss))
    for max_norm, preset in ((0.05, 0), (1.0, C.ADAM_PRESET_STEP)):
        p0, wds, grads, after, state0 = C.adam_case(max_norm, preset)
        ref = _torch_adam(p0, wds, grads, max_norm, preset, state0, torch.float64)
        for s in range(C.ADAM_STEPS):
            for k, (got, want) in enumerate(zip(after[s], ref[s])):
                assert C.close(got, want, f"adam_fp64_step max_norm={max_norm} step {s} tensor {k}", rtol=1e-12, atol=1e-12) <= 1.0


# ---- the lists ---------------------------------------------------------------------------------------------------------------------
def test_gat_case_list_and_the_centres_mixed_keeps():
    shapes = {(c.n, c.d) for c in C.GAT_CASES}
    assert {(n, d) for n in (1, 2, 16, 17, 63, 64, 65, 67, 112, 113, 127, 128) for d in (36, 256)} <= shapes
    assert {(n, d) for n in (10, 67) for d in (4, 64, 252, 256, 260, 400, 512, 1024, 1028)} <= shapes
    assert {c.kind for c in C.GAT_CASES} == {"mixed", "full", "twins", "none"} and all(1 <= c.B <= 3 for c in C.GAT_CASES)
    assert len({c.B for c in C.GAT_CASES}) == 3 and C.GAT_REFUSED == {1028: C.ERR_SHAPE}
    assert [tuple(c[:3]) for c in C.GAT_X3] == [(67, 80, 32), (17, 240, 121)]
    # one | two steps of the score kernel's lane loop (d / 4 <= 64 | > 64) and of the score backward's channel loop (d <= 256 | > 256)
    live = {d for _, d in shapes if d not in C.GAT_REFUSED}
    assert {252, 256} <= live and any(d // 4 > 64 for d in live) and any(d > 256 for d in live)
    for n in sorted({c.n for c in C.GAT_CASES}):
        A = C.adjacency("mixed", n, 3)[0]
        assert not A[n - 1].any()                                                   # no entry at all: uniform attention over all n
        if n >= 3:
            assert A[n - 2].sum() == 1 and A[n - 2, n - 2]                          # the self loop alone
        if n > 64:
            assert any(A[i].any() and not A[i, :64].any() for i in range(n))        # entries only at columns >= 64


def test_table_gradient_lists_reach_every_route():
    assert C.EMB_CHUNK == 64
    # the sorted path: one, two and three or more launches of embedding_bwd_kernel
    levels = {M: C.sorted_levels(M) for M in C.SORTED_M}
    assert levels == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 2, 2048: 2, 2049: 3, 4161: 3, 20000: 3}, levels
    assert {M for M, _ in C.SORTED_SHAPES} == set(C.SORTED_M) and {dm for _, dm in C.SORTED_SHAPES} == {4, 7, 256, 260, 300}
    for M in C.SORTED_M:
        for layout in C.SORTED_LAYOUTS:
            tokens, order, stok, V = C.sorted_case(layout, M)
            assert (np.diff(stok) >= 0).all() and stok.min() >= 0 and stok.max() < V - 1 and len(order) == M
            same = stok[1:] == stok[:-1]
            assert (np.diff(order)[same] > 0).all(), "the sort is not stable"
        assert len(set(C.sorted_tokens("same", M))) == 1 and len(set(C.sorted_tokens("distinct", M))) == M
        if M >= 128:
            s = C.sorted_tokens("chunk64", M)
            assert (s[64:128] == s[64]).all() and s[63] != s[64] and (M == 128 or s[128] != s[64])
            b = C.sorted_tokens("border", M)
            ends = np.nonzero(np.diff(b))[0] + 1
            assert len(ends) >= 2 and (ends[ends <= M - 64] % 32 == 0).all() and (ends % 64 == 0).sum() >= 1
        t = C.sorted_tokens("tail", M)
        first = int(np.argmax(t == 77))
        assert (t[first:] == 77).all() and (M % 64 == 0 or first == M // 64 * 64)
        both = C.open_chunks_per_level(C.sorted_tokens("long", M))
        assert len(both) == levels[M]
        assert (both[0] >= 1) == (M >= 141), (M, both)                              # a run over whole chunks that goes on in the next
        if M >= 4161:
            assert both[0] > 32 and both[1] >= 1, (M, both)                         # ... and again at the second level
    # the unsorted path: U = 1 | 2 | 4 at their borders
    assert {dm: C.unsorted_U(dm) for dm in C.UNSORTED_DM} == {4: 1, 252: 1, 256: 1, 260: 2, 512: 2, 516: 4, 1024: 4}
    assert {dm for dm, _, _ in C.UNSORTED_CASES} == set(C.UNSORTED_DM) and {M for _, M, _ in C.UNSORTED_CASES} == set(C.UNSORTED_M)
    assert {V for _, _, V in C.UNSORTED_CASES} == set(C.UNSORTED_V)
    for U in (1, 2, 4):                                                             # every pattern at every U
        seen = set()
        for dm, (M0, M1), V in C.UNSORTED_CASES:
            if C.unsorted_U(dm) == U:
                ids, has = C.unsorted_ids(M0, M1, V)
                assert len(ids) == M0 + M1
                seen |= has
                if "many" in has:
                    assert len(set(np.nonzero(ids == C.MANY_ID)[0] // 64)) > 8
                if "far" in has:
                    at = np.nonzero(ids == C.FAR_ID)[0] // 64
                    assert at[0] == 0 and at[1] >= 9 and len(at) >= 2
                if "pad" in has:
                    assert (ids[128:256] == C.PAD_ID).all()
                if "top" in has:
                    assert (ids == V - 1).any()
        assert seen == {"out", "pad", "many", "far", "last", "second", "top"}, (U, seen)
    assert any(M0 % 64 and M1 for _, (M0, M1), _ in C.UNSORTED_CASES) and any((M0 + M1) % 4 for _, (M0, M1), _ in C.UNSORTED_CASES)


def test_the_largest_adam_case_has_more_than_1024_chunks():
    from digat_amd import _lib, build
    build.build(verbose=False)
    chunk = int(_lib.lib().digat_opt_chunk())
    assert chunk == 16384                                                           # ADAM_SIZES are written around it
    n = C.adam_big_numel(chunk)
    assert -(-n // chunk) == 1025 > 1024 and -(-(n - 1) // chunk) == 1024
    assert {-(-s // chunk) for s in C.ADAM_SIZES} == {1, 2, 3, 5} and C.ADAM_UNALIGNED % 4 and all(C.ADAM_SIZES[k] % 4 for k in (0, 1, 2, 4, 5, 6))


# ---- headroom: the stock fp32 formulations against fp64 -----------------------------------------------------------------------------
def _gat_headroom(cases):
    worst_o = worst_g = 0.0
    for case in cases:
        for p_alpha in C.GAT_P:
            want, wgrads = C.gat_reference(case, p_alpha)
            # p = 0: oracle.gat_layer itself; with dropout the oracle has no hook: its lines as gat_fp64 restates them, in fp32
            out, grads = C.gat_eval(case, torch.float32, p_alpha, stock=p_alpha == 0)
            o = C.close(out, want, f"fp32 {case} p={p_alpha} out", **(C.OUT_TOL if p_alpha == 0 else C.TRAIN_OUT_TOL))
            g = max(C.close(grads[k], wgrads[k], f"fp32 {case} p={p_alpha} grad {k}", **C.GRAD_TOL) for k in C.GAT_GRADS)
            assert o <= HALF and g <= HALF, f"{case} p={p_alpha}: the fp32 oracle alone uses {o:.3f} (out) / {g:.3f} (gradients) of the tolerance"
            worst_o, worst_g = max(worst_o, o), max(worst_g, g)
    print(f"[A] GAT: fp32 oracle against fp64, worst err/tol out {worst_o:.3f}, gradients {worst_g:.3f} over {len(cases)} x {len(C.GAT_P)} cases")


@pytest.mark.parametrize("n", C.GAT_N)
def test_fp32_headroom_gat_over_n(n):
    _gat_headroom([c for c in C.GAT_CASES if c.n == n and c.d in C.GAT_D_ALL_N])


@pytest.mark.parametrize("d", C.GAT_D)
def test_fp32_headroom_gat_over_d(d):
    _gat_headroom([c for c in C.GAT_CASES if c.d == d and c.n in C.GAT_N_ALL_D])


@pytest.mark.parametrize("case", C.GAT_X3, ids=lambda c: f"B{c.B}-n{c.n}-d{c.d}")
def test_fp32_headroom_gat_from_2048_rows(case):
    _gat_headroom([case])


def _embedding_backward(ids, rows, V):
    """F.embedding's backward in fp32 (ids outside [0, V) cannot be looked up: they are dropped first)."""
    ok = (ids >= 0) & (ids < V)
    table = torch.zeros(V, rows.shape[1], requires_grad=True)
    (F.embedding(ids[ok], table) * rows[ok]).sum().backward()
    return table.grad


@pytest.mark.parametrize("M", C.SORTED_M)
def test_fp32_headroom_sorted_table_gradient(M):
    worst = 0.0
    for dm in [dm for m, dm in C.SORTED_SHAPES if m == M]:
        for layout in C.SORTED_LAYOUTS:
            tokens, _, _, V = C.sorted_case(layout, M)
            ids = torch.from_numpy(tokens)
            for exact in (True, False):
                rows = C.table_rows(M, dm, exact, layout)
                r = C.table_check(_embedding_backward(ids, rows, V), ids, rows, V, exact, f"F.embedding M={M} dm={dm} {layout} exact={exact}")
                assert r <= HALF
                worst = max(worst, r)
    print(f"[B] sorted M={M}: F.embedding's backward in fp32, worst err/bound {worst:.3f}")


@pytest.mark.parametrize("dm", C.UNSORTED_DM)
def test_fp32_headroom_unsorted_table_gradient(dm):
    worst = 0.0
    for _, (M0, M1), V in [c for c in C.UNSORTED_CASES if c[0] == dm]:
        ids = torch.from_numpy(C.unsorted_ids(M0, M1, V)[0])
        for exact in (True, False):
            rows = C.table_rows(M0 + M1, dm, exact, V)
            r = C.table_check(_embedding_backward(ids, rows, V), ids, rows, V, exact, f"F.embedding dm={dm} M=({M0}, {M1}) V={V} exact={exact}")
            assert r <= HALF
            worst = max(worst, r)
    print(f"[B] unsorted dm={dm}: F.embedding's backward in fp32, worst err/bound {worst:.3f}")


def test_fp32_headroom_row_logits():
    worst = 0.0
    for B in C.LOGITS_B:
        for d in C.LOGITS_D:
            nc, uc, dl = C.logits_inputs(B, d)
            want, got = C.logits_eval(nc, uc, dl), C.logits_eval(nc, uc, dl, torch.float32)
            r = max(C.close(got[0], want[0], f"fp32 logits B={B} d={d}", **C.LOGIT_TOL),
                    C.close(got[1], want[1], f"fp32 d news_ctx B={B} d={d}", **C.HEAD_GRAD_TOL),
                    C.close(got[2], want[2], f"fp32 d user_ctx B={B} d={d}", **C.HEAD_GRAD_TOL))
            assert r <= HALF, (B, d, r)
            worst = max(worst, r)
    print(f"[C] row logits: fp32 against fp64, worst err/tol {worst:.3f}")


@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_fp32_headroom_click_loss(kind):
    worst = 0.0
    for B in C.LOSS_B:
        for K in C.LOSS_K:
            x = C.loss_inputs(B, K, kind)
            want, wgrad = C.loss_eval(x)
            got, grad = C.loss_eval(x, torch.float32)                               # torch.log_softmax on fp32
            r = max(C.close(got, want, f"fp32 loss B={B} K={K} {kind}", **C.LOSS_TOL), C.close(grad, wgrad, f"fp32 d logits B={B} K={K} {kind}", **C.HEAD_GRAD_TOL))
            assert r <= HALF, (B, K, kind, r)
            if K == 1:
                assert float(want) == 0.0 and float(wgrad.abs().max()) == 0.0
            worst = max(worst, r)
    print(f"[C] click loss {kind}: torch.log_softmax in fp32 against fp64, worst err/tol {worst:.3f}")


def _torch_adam(p0, wds, grads, max_norm, preset_step, state0, dtype):
    """clip_grad_norm_ + torch.optim.Adam in ``dtype``: the parameters after each step."""
    ps = [x.to(dtype).clone().requires_grad_(True) for x in p0]
    opt = torch.optim.Adam([{"params": [p], "weight_decay": wd} for p, wd in zip(ps, wds)], lr=C.ADAM_LR, betas=C.ADAM_BETAS, eps=C.ADAM_EPS)
    if preset_step:
        for p, m, v in zip(ps, *state0):
            opt.state[p] = {"step": torch.tensor(float(preset_step)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    after = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        after.append([p.detach().clone() for p in ps])
    return after


@pytest.mark.parametrize("max_norm,preset", [(m, 0) for m in C.ADAM_MAX_NORMS] + [(1.0, C.ADAM_PRESET_STEP)])
def test_fp32_headroom_clip_adam(max_norm, preset):
    p0, wds, grads, after, state0 = C.adam_case(max_norm, preset)
    got = _torch_adam(p0, wds, grads, max_norm, preset, state0, torch.float32)
    worst = max(C.close(got[s][k], after[s][k], f"fp32 Adam max_norm={max_norm} step {s} tensor {k}", **C.ADAM_TOL)
                for s in range(C.ADAM_STEPS) for k in range(len(p0)))
    assert worst <= HALF, worst
    print(f"[C] clip + Adam max_norm={max_norm} preset={preset}: torch in fp32 against fp64, worst err/tol {worst:.3f}")


def test_fp32_headroom_clip_adam_beyond_1024_chunks():
    """The one-tensor case of 1024 chunks + 1 element, one step with clipping on — the very inputs the GPU file runs
    (C.adam_big_case) — and, in C.adam_big_check, its conditions: a squared norm without the 1025th partial would be seen."""
    chunk = 16384
    p0, grad, m0, v0 = C.adam_big_case(chunk)
    want = C.adam_big_check(p0, grad, m0, v0, chunk)
    got = _torch_adam([p0], [0.0], [[grad]], C.ADAM_BIG_MAX_NORM, C.ADAM_BIG_PRESET_STEP, ([m0], [v0]), torch.float32)
    worst = float(C.adam_ratio(got[0][0], want).max())
    assert worst <= HALF, worst
    print(f"[C] clip + Adam, 1025 chunks: torch in fp32 against fp64, worst err/tol {worst:.3f}")
