"""CPU half of the Eq. 8 fp64 sweeps (tests/test_hip_eq8_fp64.py is the GPU half).  Three things are held here:
  * the fp64 references of tests/eq8_fp64_common.py reproduce the a1 / a2 vectors minted from the reference's own module
    (tests/golden/tiny.npz, edges.npz), equal oracle.cross_graph_attention / oracle.encoder_inference on double inputs, and the
    pairwise reference fed with fp64 projections equals the layer reference;
  * on every case the GPU file runs, fp32 arithmetic alone (the stock fp32 oracle; for the pairwise stage its fp32 evaluation) stays
    within a QUARTER of the tolerance of the fp64 reference for the inference cases and within HALF of it for the training cases
    (there also with the scores summed as one fp32 chain over the channels, the order a kernel takes): a condition on the inputs
    of a case, so that the tolerance the kernels are held to is not already spent by the number format;
  * the case lists name at least one case of every kernel class of the Eq. 8 dispatch (a membership check on (n, d, B)), and the
    launch plan (digat_amd/csrc/digat_xattn_plan.h) sends them to every kernel family at every width class."""
import numpy as np
import pytest
import torch

import eq8_fp64_common as C
import xattn_plan_common as XP
from conftest import load_golden, split_fixture
from oracle import digat_oracle as O

QUARTER, HALF = 0.25, 0.5


# ---- the references against the golden fixtures and the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny.npz", "edges.npz"])
def test_layer_fp64_reproduces_reference_vectors(name):
    ins, w, outs = split_fixture(load_golden(name))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    Xn, ue = t(ins["news_graph_embeddings"]), t(ins["user_news_embedding"])
    Xu = torch.cat([ue, t(w["topic_node_embedding"]).unsqueeze(0).expand(Xn.shape[0], -1, -1)], dim=1)
    got_n, _ = C.layer_fp64(w, "news", 0, Xn, t(ins["news_graph"]), t(outs["a4_user_ctx"]))
    got_u, _ = C.layer_fp64(w, "user", 0, Xu, t(ins["user_graph"]), t(outs["a3_news_ctx"]))
    assert got_n.dtype == got_u.dtype == torch.float64
    np.testing.assert_allclose(got_n.numpy(), outs["a1_news_emb_l0"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got_u.numpy(), outs["a2_user_emb_l0"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", [C.Case(10, 36, 3, "mixed"), C.Case(67, 64, 2, "mixed"), C.Case(128, 20, 2, "twins"), C.Case(17, 4, 2, "none")],
                         ids=lambda c: f"n{c.n}-d{c.d}-{c.kind}")
def test_layer_fp64_equals_the_oracle_on_double_inputs(case):
    """oracle.cross_graph_attention runs in fp64 when its inputs are double; the graph-by-graph restatement (projections, then the
    pairwise reference (b)) is the same function."""
    state = C.layer_state(case.d)
    X, ctx, A = C.layer_inputs(case)
    p = {k: torch.from_numpy(v).double() for k, v in state.items()}
    want, want_alpha = O.cross_graph_attention(p, "user", 0, X.double(), A, ctx.double(), return_alpha=True)
    assert want.dtype == want_alpha.dtype == torch.float64
    got, alpha = C.layer_fp64(state, "user", 0, X, A, ctx)
    assert C.close(got, want, "layer_fp64", rtol=1e-12, atol=1e-12) <= 1.0 and C.close(alpha, want_alpha, "alpha", rtol=1e-12, atol=1e-13) <= 1.0


def test_encoder_fp64_equals_the_oracle_on_double_inputs():
    U, d = 64, 64
    state, b = C.encoder_inputs(U, d)
    p = {k: torch.from_numpy(v).double() for k, v in state.items()}
    t = lambda k: torch.from_numpy(np.ascontiguousarray(b[k]))
    rg = t("row_group").long()
    args = [t("news_graph_embeddings"), t("news_graph"), t("news_graph_mask"), t("user_news_embedding")[rg], t("user_graph")[rg],
            t("user_category_mask")[rg], t("user_category_indices")[rg]]
    c0 = O.news_graph_context(p, args[0].double(), args[2])
    want = O.encoder_inference(p, C.ENC_DEPTH, args[0].double(), args[1], args[2], args[3].double(), *args[4:], c0)
    got = C.encoder_fp64(state, C.ENC_DEPTH, *args, c0)
    for g, w_, name in zip(got, want, ("news", "user")):
        assert w_.dtype == torch.float64 and C.close(g, w_, f"encoder_fp64 {name}", rtol=1e-12, atol=1e-12) <= 1.0


# ---- the lists -------------------------------------------------------------------------------------------------------------------
def test_adjacency_kinds_are_what_they_are_named_for():
    for n in C.N_LIST:
        for kind in C.KINDS:
            A = C.adjacency(kind, n, 3)
            assert A.shape == (3, n, n) and A.dtype == bool and np.array_equal(A, C.adjacency(kind, n, 3)), (kind, n)
            if kind not in ("twins", "full", "none") and n >= 8:                        # centre and neighbour cannot be swapped, in any graph
                assert all(not np.array_equal(A[b], A[b].T) for b in range(3)), (kind, n)
        deg = C.adjacency("mixed", n, 2)[0].sum(axis=1)
        A = C.adjacency("mixed", n, 2)[0]
        assert (C.adjacency("full", n, 1).sum(axis=2) == n).all() and (C.adjacency("identity", n, 3).sum(axis=2) == 1).all()
        assert not C.adjacency("none", n, 2).any()
        assert deg[n - 1] == 0
        if n >= 3:
            assert A[n - 2].sum() == 1 and A[n - 2, n - 2] and A[n - 3].sum() == 1 and A[n - 3, n - 1]
        if n > 64:
            assert any(A[i, :64].sum() == 0 and A[i, 64:].any() for i in range(n)) and any(A[i, 64:].sum() == 0 and A[i, :64].any() for i in range(n))
        if n >= 17:
            assert {2, 3, 5, 6, 7} <= set(int(v) for v in deg)
    g = C.adjacency("twins", 67, 3)
    assert np.array_equal(g, g.transpose(0, 2, 1)) and g.sum(axis=2).max() >= 50                   # a clique of a whole history


def test_case_lists_name_every_kernel_class():
    """At least one case of each class of the Eq. 8 dispatch: membership on (n, d, B), not a restatement of the launch plan; then the plan's own answer."""
    pair = {(c.n, c.d, c.B) for c in C.PAIR_CASES}
    layer = {(c.n, c.d) for c in C.LAYER_CASES}
    has = lambda s, f: any(f(*c) for c in s)
    for V, lo, hi in ((1, 1, 256), (2, 257, 512), (4, 513, 1024)):                                  # pieces of a row per lane
        # small-graph kernels: the graph-in-LDS one (n d / 4 <= 2048, no alpha: the layer entry) and score + aggregation
        assert has(layer, lambda n, d: n <= 16 and lo <= d <= hi and n * d / 4 <= 2048), V
        assert has(pair, lambda n, d, B: n <= 16 and lo <= d <= hi), V
        # the wave-per-centre sparse kernel on user-sized graphs, inference and training
        assert has(layer, lambda n, d: n > 16 and lo <= d <= hi) and has(layer, lambda n, d: n in (64, 65, 67, 128) and lo <= d <= hi), V
    assert (15, 516) in layer and (16, 516) in layer and (16, 512) in layer                        # both sides of n d / 4 = 2048
    assert has(layer, lambda n, d: n <= 16 and d > 1024) and has(pair, lambda n, d, B: n <= 16 and d > 1024)   # tile kernel on a small graph
    # tile kernel: several graphs per workgroup (17 <= n <= 44) with B = 1, a full and a partial last workgroup; one graph from n = 45
    for n, per_wg in ((17, 10), (44, 2)):
        assert has(pair, lambda m, d, B: m == n and B == 1) and has(pair, lambda m, d, B: m == n and B > per_wg and B % per_wg)
    assert {17, 20, 21, 32, 33, 44} <= {n for n, _, _ in pair} and {45, 64, 65, 127, 128} <= {n for n, _, _ in pair}
    assert has(pair, lambda n, d, B: n == 128 and d == 1024) and has(pair, lambda n, d, B: n == 128 and d == 4)     # the largest LDS plan, the smallest
    assert len({d for n, d, _ in pair if n == 128}) >= 12 and len({d for n, d, _ in pair if n == 67}) >= 12         # > 64 KiB plans at every width
    # the encoder's variants: layer-0 chunk and twin kernels at one and two pieces per lane, with and without the row lists
    assert {d for _, d in C.ENC_CASES if d <= 256 and d % 80 == 0} and {d for _, d in C.ENC_CASES if 256 < d <= 512 and d % 80 == 0}
    assert {U for U, _ in C.ENC_CASES} == {64, 65, 128} and any(d > 512 for _, d in C.ENC_CASES) and any(d % 80 for _, d in C.ENC_CASES)
    assert all(4 * C.ENC_G <= C.ENC_G * C.ENC_ROWS and C.ENC_G * C.ENC_ROWS * U >= 2048 for U, _ in C.ENC_CASES)
    assert all(c.B * c.n >= 2048 and c.d % 80 == 0 and c.n > 16 for c in C.LAYER_BIG)
    # training: centre / node backward at one and two pieces (d <= 256 | 512), the all-pairs backward on both sides of n = 113
    train = {(c.n, c.d) for c in C.TRAIN_CASES}
    assert has(train, lambda n, d: n > 16 and d <= 256) and has(train, lambda n, d: n > 16 and 256 < d <= 512) and has(train, lambda n, d: d > 512)
    assert {(112, 36), (113, 36), (128, 256), (1, 36), (16, 36), (17, 36)} <= train
    assert all(c.B <= 3 for c in C.PAIR_CASES if (c.n, c.d, c.B) not in C.RB_EXTRA) and all(c.B <= 3 for c in C.TRAIN_CASES)

    # ... and what the launch plan itself says (digat_amd/csrc/digat_xattn_plan.h, asked through its test harness): the kernel
    # instantiations the cases of each list take, as the GPU file calls the entries
    def kernels(requests, *fields):
        return {XP.kernel_name(w[f]) for w in map(XP.parse, XP.run(requests)) for f in fields} - {"NONE"}
    shapes = lambda cases: sorted({(c.B, c.n, c.d) for c in cases})
    widths = lambda fmt: {fmt.format(U) for U in (1, 2, 4)}
    # block A: digat_xattn_pairwise_fwd, alpha wanted
    pair_k = kernels([("pair", dict(B=B, n=n, d=d, alpha_wanted=1)) for B, n, d in shapes(C.PAIR_CASES)], "score", "agg")
    assert pair_k == widths("SMALL<{}>") | {"TILE", "AGG<512>", "AGG<1024>"}, pair_k
    # block B, dense: the layer without alpha; sparse (n > 16, d <= 1024): the wave-per-centre kernel
    dense_k = kernels([("pair", dict(B=B, n=n, d=d, alpha_wanted=0)) for B, n, d in shapes(C.LAYER_CASES)], "score", "agg")
    # (16 nodes of up to two pieces per lane always fit the graph-in-LDS kernel: the fused form reaches the other one at four only)
    assert dense_k == widths("SMALL_LDS<{}>") | {"SMALL<4>", "TILE", "AGG<512>", "AGG<1024>"}, dense_k
    sparse_k = kernels([("sparse", dict(B=B, n=n, d4=d // 4)) for B, n, d in shapes(C.LAYER_CASES) if n > 16 and d <= 1024], "launch")
    assert sparse_k == widths("SPARSE<{},0,0,0>"), sparse_k
    # block C: layer 0 of grouped rows (the chunk kernel, or the sparse kernel adding K3 beyond two pieces per lane), then the
    # layers on the live lists with their twins
    B = C.ENC_G * C.ENC_ROWS
    l0_on = dict(group=1, xgroup=1, radd=1, rowidx=1, nrows_dev=1, live=1)
    enc_k = kernels([("l0", dict(B=B, n=U, d4=d // 4, G=C.ENC_G, **l0_on)) for U, d in C.ENC_CASES], "launch")
    enc_k |= kernels([("sparse", dict(B=B, n=U, d4=d // 4, **l0_on)) for U, d in C.ENC_CASES if d > 512], "launch")
    enc_k |= kernels([("sparse", dict(B=B, n=U, d4=d // 4, twin=1, rowidx=1, nrows_dev=1, live=1)) for U, d in C.ENC_CASES], "launch")
    assert enc_k == {"L0<1,4>", "L0<2,4>", "TWIN<1,2>", "TWIN<2,2>", "SPARSE<4,0,1,0>", "SPARSE<4,0,0,0>"}, enc_k
    # block D: the layer's training entries always pass the device flag and ask for K3's gradient; modes 1 and 2
    tr = [(r, dict(B=B, n=n, d=d, mode=m, flag=1, dr=1)) for B, n, d in shapes(C.TRAIN_CASES) for m in (1, 2) for r in ("train_fwd", "train_bwd")]
    fwd_k = kernels([q for q in tr if q[0] == "train_fwd"], "sparse", "score", "agg")
    bwd_k = kernels([q for q in tr if q[0] == "train_bwd"], "sparse", "pair")
    assert fwd_k == widths("SPARSE<{},0,0,1>") | widths("SMALL<{}>") | {"TILE", "AGG<512>", "AGG<1024>"}, fwd_k
    assert bwd_k == {"SPARSE_BWD<1>", "SPARSE_BWD<2>", "PAIR_BWD<64>", "PAIR_BWD<32>"}, bwd_k


# ---- headroom: fp32 against fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PAIR_NS)
def test_fp32_headroom_pairwise(n):
    worst_o = worst_a = 0.0
    cases = [c for c in C.PAIR_CASES if c.n == n]
    for case in cases:
        ins = C.pair_inputs(case)
        out, alpha = C.pairwise(*ins, dtype=torch.float32)
        want, want_alpha = C.pairwise_fp64(*ins)
        o, a = C.close(out, want, f"fp32 {case} out", **C.OUT_TOL), C.close(alpha, want_alpha, f"fp32 {case} alpha", **C.ALPHA_TOL)
        assert o <= QUARTER and a <= QUARTER, f"{case}: fp32 alone uses {o:.3f} (out) / {a:.3f} (alpha) of the tolerance"
        worst_o, worst_a = max(worst_o, o), max(worst_a, a)
    print(f"pairwise n={n}: fp32 against fp64, worst err/tol out {worst_o:.3f}, alpha {worst_a:.3f} over {len(cases)} cases")


def _layer_headroom(cases):
    worst_o = worst_a = 0.0
    for case in cases:
        state = C.layer_state(case.d)
        X, ctx, A = C.layer_inputs(case)
        with torch.no_grad():
            out, alpha = O.cross_graph_attention(O.as_params(state), "user", 0, X, A, ctx, return_alpha=True)
        want, want_alpha = C.layer_fp64(state, "user", 0, X, A, ctx)
        o, a = C.close(out, want, f"fp32 {case} out", **C.OUT_TOL), C.close(alpha, want_alpha, f"fp32 {case} alpha", **C.ALPHA_TOL)
        assert o <= QUARTER and a <= QUARTER, f"{case}: the fp32 oracle alone uses {o:.3f} (out) / {a:.3f} (alpha) of the tolerance"
        worst_o, worst_a = max(worst_o, o), max(worst_a, a)
    print(f"layer: fp32 oracle against fp64, worst err/tol out {worst_o:.3f}, alpha {worst_a:.3f} over {len(cases)} cases")


@pytest.mark.parametrize("d", sorted({c.d for c in C.LAYER_CASES}))
def test_fp32_headroom_layer(d):
    _layer_headroom([c for c in C.LAYER_CASES if c.d == d])


@pytest.mark.parametrize("d", sorted({c.d for c in C.LAYER_BIG}))
def test_fp32_headroom_layer_from_2048_rows(d):
    _layer_headroom([c for c in C.LAYER_BIG if c.d == d])


@pytest.mark.parametrize("U,d", C.ENC_CASES)
def test_fp32_headroom_encoder(U, d):
    state, b = C.encoder_inputs(U, d)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(b[k]))
    rg = t("row_group").long()
    args = [t("news_graph_embeddings"), t("news_graph"), t("news_graph_mask"), t("user_news_embedding")[rg], t("user_graph")[rg],
            t("user_category_mask")[rg], t("user_category_indices")[rg]]
    c0 = O.news_graph_context({k: torch.from_numpy(v).double() for k, v in state.items()}, args[0].double(), args[2]).float()
    want = C.encoder_fp64(state, C.ENC_DEPTH, *args, c0)
    with torch.no_grad():                                      # one group's rows at a time: [8, U, U, d] fp32
        got = [O.encoder_inference(O.as_params(state), C.ENC_DEPTH, *(a[s:s + C.ENC_ROWS] for a in args), c0[s:s + C.ENC_ROWS])
               for s in range(0, rg.shape[0], C.ENC_ROWS)]
    worst = max(C.close(torch.cat([g[i] for g in got]), want[i], f"fp32 encoder U={U} d={d} {name}", **C.OUT_TOL) for i, name in enumerate(("news", "user")))
    assert worst <= QUARTER, f"U={U} d={d}: the fp32 oracle alone uses {worst:.3f} of the tolerance"
    print(f"encoder U={U} d={d}: fp32 oracle against fp64, worst err/tol {worst:.3f}")


def _train_headroom(cases):
    worst_o = worst_g = 0.0
    for case in cases:
        for p_alpha in C.TRAIN_P:
            out, grads = C.train_reference(case, torch.float32, p_alpha)
            want, wgrads = C.train_reference(case, torch.float64, p_alpha)
            C.assert_well_conditioned(case, wgrads)
            o = max(C.close(out, want, f"fp32 {case} p={p_alpha} out", **C.TRAIN_OUT_TOL),
                    C.close(C.sequential_forward_fp32(case, p_alpha), want, f"fp32, scores summed as a chain, {case} p={p_alpha} out", **C.TRAIN_OUT_TOL))
            g = max(C.close(grads[k], wgrads[k], f"fp32 {case} p={p_alpha} grad {k}", **C.GRAD_TOL) for k in wgrads)
            assert o <= HALF and g <= HALF, f"{case} p={p_alpha}: the fp32 oracle alone uses {o:.3f} (out) / {g:.3f} (gradients) of the tolerance"
            worst_o, worst_g = max(worst_o, o), max(worst_g, g)
    print(f"training: fp32 oracle against fp64, worst err/tol out {worst_o:.3f}, gradients {worst_g:.3f} over {len(cases)} x {len(C.TRAIN_P)} cases")


@pytest.mark.parametrize("n", sorted({c.n for c in C.TRAIN_CASES}))
def test_fp32_headroom_training(n):
    _train_headroom([c for c in C.TRAIN_CASES + C.TRAIN_NONE if c.n == n])
