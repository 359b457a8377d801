"""CPU half of the context stage's fp64 sweeps (tests/test_hip_ctx_fp64.py is the GPU half).  Held here:
  * the fp64 references of tests/ctx_fp64_common.py reproduce the a3 / a4 / a6 vectors minted from the reference's own module
    (tests/golden/tiny.npz, edges.npz) and equal the oracle's functions on double inputs;
  * on every case the GPU file runs, fp32 arithmetic alone stays within a QUARTER of the tolerance of the fp64 reference when its
    sums are torch's (BLAS), and on the kernel-alone cases of blocks A and B within HALF of it when the scores are summed as one
    fp32 chain over the channels, the plain loop: a condition on the inputs of a case, so that the tolerance the kernels are held
    to is not already spent by the number format;
  * the case lists reach every kernel the launchers choose between (route_pool / route_topic restate their conditions), and the
    planted rows are what they are named for."""
import math

import numpy as np
import pytest
import torch

import ctx_fp64_common as C
from conftest import load_golden, split_fixture
from oracle import digat_oracle as O

QUARTER, HALF = 0.25, 0.5
t = lambda v: torch.from_numpy(np.ascontiguousarray(v))


def _folded(p, name, c):
    """K^T (Q c + b) in the dtype of p."""
    sep = "_" if name == "user_news" else "."
    return (c @ p[f"{name}{sep}Q.weight"].T + p[f"{name}{sep}Q.bias"]) @ p[f"{name}{sep}K.weight"]


# ---- the references against the golden fixtures and the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny.npz", "edges.npz"])
def test_references_reproduce_the_reference_vectors(name):
    ins, w, outs = split_fixture(load_golden(name))
    p = C.f64_params(w)
    Xn, Mn, ue = t(ins["news_graph_embeddings"]).double(), t(ins["news_graph_mask"]), t(ins["user_news_embedding"]).double()
    tol = dict(rtol=1e-5, atol=1e-5)
    # a6: candidate_attention over the news graph, query = node 0, through pool_eval on the folded query
    a6, _ = C.pool_eval(Xn, _folded(p, "candidate_attention", Xn[:, 0]), Mn)
    assert a6.dtype == torch.float64
    np.testing.assert_allclose(a6.numpy(), outs["a6_sdpa_candidate"], **tol)
    # a3: block C's news reference is the oracle on double inputs
    a3 = O.news_graph_context(p, Xn, Mn)
    np.testing.assert_allclose(a3.numpy(), outs["a3_news_ctx"], **tol)
    # a4: block C's user reference, and block D's evaluation from the two folded queries
    H = ue.shape[1]
    Xu = O.user_nodes(p, ue)
    cm, ci = t(ins["user_category_mask"]), t(ins["user_category_indices"])
    a4 = C.user_context(p, Xu, cm, ci, a3, H)
    np.testing.assert_allclose(a4.numpy(), outs["a4_user_ctx"], **tol)
    c = dict(x=Xu[:, :H], kq_t=_folded(p, "user_news", a3), kq_u=_folded(p, "userAttention", a3), idx=ci, mask=cm.bool(),
             Fa=p["featureAffine.weight"], bFa=p["featureAffine.bias"])
    np.testing.assert_allclose(C.fused_eval(c, cm.shape[1]).numpy(), outs["a4_user_ctx"], **tol)


@pytest.mark.parametrize("H,C1,d", [(5, 6, 64), (50, 18, 36), (65, 29, 64)])
def test_references_equal_the_oracle_on_double_inputs(H, C1, d):
    """Where every index is valid: user_context is oracle.user_graph_context, topic_eval is oracle.topic_pooling on the folded query,
    and fused_eval on the two folded queries is the same function again."""
    p = C.f64_params(C.ctx_state(d, C1 - 1))
    Xu, mask, idx, c_n, _ = C.user_inputs(H, C1, d)
    ok = ((idx >= 0) & (idx < C1)).all(dim=1)
    Xu, mask, idx, c_n = Xu[ok].double(), mask[ok], idx[ok], c_n[ok].double()
    assert int(ok.sum()) >= 2
    want = O.user_graph_context(p, Xu, mask, idx, c_n, H)
    assert want.dtype == torch.float64
    assert C.close(C.user_context(p, Xu, mask, idx, c_n, H), want, "user_context", rtol=1e-12, atol=1e-12) <= 1.0
    kq_t, kq_u = _folded(p, "user_news", c_n), _folded(p, "userAttention", c_n)
    T, empty = C.topic_eval(Xu[:, :H], kq_t, idx, C1)
    assert C.close(T, O.topic_pooling(p, Xu, idx, c_n, H), "topic_eval", rtol=1e-10, atol=1e-10) <= 1.0
    assert bool((T[empty] == 0).all())
    c = dict(x=Xu[:, :H], kq_t=kq_t, kq_u=kq_u, idx=idx, mask=mask, Fa=p["featureAffine.weight"], bFa=p["featureAffine.bias"])
    assert C.close(C.fused_eval(c, C1), want, "fused_eval", rtol=1e-10, atol=1e-10) <= 1.0


def test_dead_slots_and_dropped_indices_in_the_topic_reference():
    """live: where(live, x, 0) — a dead slot keeps its place in its category's softmax with score 0; an index out of range does not."""
    x = torch.tensor([[[1.0, 2.0], [3.0, -1.0], [float("nan"), float("nan")], [5.0, 5.0]]])
    kq, idx = torch.tensor([[0.5, 0.25]]), torch.tensor([[0, 0, 0, 7]])
    live = torch.tensor([[1, 1, 0, 1]], dtype=torch.uint8)
    T, empty = C.topic_eval(x, kq, idx, 2, live=live)
    s = torch.tensor([1.0, 1.25, 0.0]).double() / math.sqrt(2)
    a = torch.softmax(s, 0)
    np.testing.assert_allclose(T[0, 0].numpy(), (a[0] * x[0, 0].double() + a[1] * x[0, 1].double()).numpy(), rtol=1e-14)
    assert bool((T[0, 1] == 0).all()) and empty.tolist() == [[False, True]]


# ---- the lists -------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_kernel():
    pool = [C.route_pool(n, d) for n, d in C.POOL_SHAPES]
    for kernel in [f"resident<{npw},{u}>" for npw in (3, 5, 7, 17) for u in (1, 2)] + ["attn_pool_kernel"]:
        assert pool.count(kernel) >= 2, kernel
    assert {C.route_pool(n, d) for n, d in C.POOL_LD} == {f"resident<{npw},{u}>" for npw in (3, 5, 7, 17) for u in (1, 2)}
    topic = {C.route_topic(*s) for s in C.TOPIC_SHAPES}
    assert topic >= {(k, ct) for k in ("resident<13>", "resident<16>", "topic_pool_kernel") for ct in (1, 2, 3, 4)}, topic
    # H = 53 .. 64 beyond eight channel groups must take topic_pool_kernel; both sides of each boundary are on the list
    assert C.route_topic(53, 18, 516)[0] == C.route_topic(64, 18, 1024)[0] == "topic_pool_kernel" and C.route_topic(64, 18, 512)[0] == "resident<16>"
    assert {(52, 18, 400), (53, 18, 400), (64, 18, 400), (65, 18, 400), (53, 18, 516), (64, 18, 516), (0, 18, 36)} <= set(C.TOPIC_SHAPES)
    assert all(n <= C.MAX_NODES for n, _ in C.POOL_SHAPES) and all(d % 4 == 0 for _, d in C.POOL_SHAPES)
    assert all(C1 <= C.MAX_NODES and {3, 5, 7, 17} == {int(C.route_pool(c, 400)[9:-3]) for c in C.USER_C1} for _, C1, _ in C.USER_SHAPES)
    # D: every case fits the kernel, every refusal does not; every batch size meets the overflow tile, and whole and partial workgroups occur
    assert all(C.fused_ok(H, C1, d) for H, C1, d, _ in C.FUSED_CASES) and not any(C.fused_ok(*s) for s in C.FUSED_REFUSED)
    assert {(d + 63) // 64 for d in C.FUSED_D} == {4, 5, 7}
    assert {B for H, C1, d, B in C.FUSED_CASES if H >= C1 >= 17} == set(C.FUSED_B) and {B % 4 for B in C.FUSED_B} == {0, 1, 2, 3}


def test_planted_rows_are_what_they_are_named_for():
    for n in C.POOL_N:
        m = C.pool_masks(n, C._gen("m", n))
        assert m[0].all() and m[1].any() and m[2].tolist() == [j == 0 for j in range(n)] and m[3].tolist() == [j == n - 1 for j in range(n)] and not m[4].any()
        assert m.shape[0] <= 8 and (n <= 64 or (m[5, 64:].any() and not m[5, :64].any()))
        feat, _, mask, _ = C.pool_inputs(n, 36, 1.0)
        assert torch.isnan(feat[mask.any(1)][~mask[mask.any(1)]]).all() and torch.isfinite(feat[~mask.any(1)]).all() and torch.isfinite(feat[mask]).all()
    for H, C1 in [(52, 18), (64, 64), (256, 49), (5, 2), (1, 1), (0, 18)]:
        idx = C.topic_rows(H, C1, C._gen("r", H, C1))
        assert idx.shape == (7, H) and idx.shape[0] <= 8
        if H >= C1:
            assert set(idx[2].tolist()) == set(range(C1)) and len(set(idx[1].tolist())) == 1
        if H >= 3:
            assert {-1, C1 + 1} <= set(idx[5].tolist()) and (idx[3][1:] >= idx[3][:-1]).all() and int(((idx[4] >= 0) & (idx[4] < C1)).sum()) == 1
        if H >= 2 and C1 >= 2:
            assert int((idx[6] == 1).sum()) == 1
    for H in C.TOPIC_H:
        hl = C.topic_hlasts(H)
        k4 = 4 * max(1, H // 8)
        assert {min(v, H) for v in (0, 1, k4 - 1, k4, k4 + 1, H)} <= set(hl) and all(0 <= v <= H for v in hl)
        Xu, _, _, flags, hlast = C.topic_list_inputs(H, 18, 36, 1.0)
        live = flags[:, :H].bool()
        assert (flags[:, H:] == 0xEE).all() and torch.isnan(Xu[:, :H][~live]).all() and torch.isfinite(Xu[:, :H][live]).all() and torch.isnan(Xu[:, H:]).all()
        for r in range(8):                                              # hlast = 1 + the last live slot
            assert (int(hlast[r]) == 0 and not live[r].any()) or (live[r, int(hlast[r]) - 1] and not live[r, int(hlast[r]):].any())
        if H >= 8:
            assert not live[6].all() and int(hlast[6]) == H              # a dead slot in the middle of live ones
    # D: at C + 1 = 17 .. 20 rows 0, 3 and 4 need more than 16 slots and share their workgroups with rows that need fewer
    for C1 in (17, 18, 20):
        idx, mask = C.fused_users(52, C1, C._gen("u", C1))
        slots = []
        for r in range(8):
            present = {int(v) for v in idx[r].tolist() if 0 <= v < C1}
            slots.append(len(present & ({c for c in range(C1) if mask[r, c]} if mask[r].any() else set(range(C1)))))
        assert slots[0] == C1 - 1 and slots[3] == C1 and slots[4] == C1 and max(slots[1], slots[2], slots[5], slots[6], slots[7]) <= 16, slots


# ---- headroom: fp32 against fp64 ---------------------------------------------------------------------------------------------
def _budget(what, got, want, tol, share, worst):
    r = C.close(got, want, what, **tol)
    assert r <= share, f"{what}: fp32 alone uses {r:.3f} of the tolerance (allowed: {share})"
    return max(worst, r)


@pytest.mark.parametrize("n", C.POOL_N)
def test_fp32_headroom_attention_pooling(n):
    blas = chain = 0.0
    shapes = [s for s in C.POOL_SHAPES if s[0] == n]
    for _, d in shapes:
        for gain in C.gains("pool", n, d):
            feat, kq, mask, _ = C.pool_inputs(n, d, gain)
            want, want_alpha = C.pool_eval(feat, kq, mask)
            for share, ch in ((QUARTER, False), (HALF, True)):
                out, alpha = C.pool_eval(feat, kq, mask, torch.float32, chain=ch)
                w = _budget(f"pool n={n} d={d} gain={gain} chain={ch} out", out, want, C.OUT_TOL, share, 0.0)
                w = _budget(f"pool n={n} d={d} gain={gain} chain={ch} alpha", alpha, want_alpha, C.ALPHA_TOL, share, w)
                blas, chain = (blas, max(chain, w)) if ch else (max(blas, w), chain)
    print(f"[A] pool n={n}: fp32 against fp64, worst err/tol BLAS {blas:.3f}, chain {chain:.3f} over {len(shapes)} shapes x {len(C.GAINS)} gains")


@pytest.mark.parametrize("H", C.TOPIC_H)
def test_fp32_headroom_topic_pooling(H):
    blas = chain = 0.0
    shapes = [s for s in C.TOPIC_SHAPES if s[0] == H]
    for _, C1, d in shapes:
        for gain in C.gains("topic", H, C1, d):
            Xu, kq, idx = C.topic_inputs(H, C1, d, gain)
            Xl, kql, idxl, flags, _ = C.topic_list_inputs(H, C1, d, gain)
            Xg, rg, kqg, idxg, flagsg, _ = C.topic_group_inputs(H, C1, d, gain)
            calls = [("plain", Xu[:, :H], kq, idx, None), ("lists", Xl[:, :H], kql, idxl, flags[:, :H]),
                     ("groups", Xg[rg.long()][:, :H], kqg, idxg, flagsg[:, :H])]
            for name, x, k, ix, live in calls:
                want, _ = C.topic_eval(x, k, ix, C1, live=live)
                for share, ch in ((QUARTER, False), (HALF, True)):
                    got, _ = C.topic_eval(x, k, ix, C1, torch.float32, live=live, chain=ch)
                    w = _budget(f"topic {name} H={H} C1={C1} d={d} gain={gain} chain={ch}", got, want, C.OUT_TOL, share, 0.0)
                    blas, chain = (blas, max(chain, w)) if ch else (max(blas, w), chain)
    print(f"[B] topic H={H}: fp32 against fp64, worst err/tol BLAS {blas:.3f}, chain {chain:.3f} over {len(shapes)} shapes x {len(C.GAINS)} gains x 3 calls")


@pytest.mark.parametrize("d", C.NEWS_D)
def test_fp32_headroom_news_context(d):
    worst = 0.0
    for N in C.NEWS_N:
        state = C.ctx_state(d, 17)
        X, mask, _ = C.news_inputs(N, d)
        with torch.no_grad():
            got, want = O.news_graph_context(O.as_params(state), X, mask), O.news_graph_context(C.f64_params(state), X.double(), mask)
        worst = _budget(f"news context N={N} d={d}", got, want, C.OUT_TOL, QUARTER, worst)
    print(f"[C] news context d={d}: fp32 oracle against fp64, worst err/tol {worst:.3f}")


@pytest.mark.parametrize("d", C.USER_D)
def test_fp32_headroom_user_context(d):
    worst = 0.0
    for H, C1, _ in [s for s in C.USER_SHAPES if s[2] == d]:
        state = C.ctx_state(d, C1 - 1)
        Xu, mask, idx, c_n, _ = C.user_inputs(H, C1, d)
        with torch.no_grad():
            got = C.user_context(O.as_params(state), Xu, mask, idx, c_n, H)
            want = C.user_context(C.f64_params(state), Xu.double(), mask, idx, c_n.double(), H)
        worst = _budget(f"user context H={H} C1={C1} d={d}", got, want, C.OUT_TOL, QUARTER, worst)
    print(f"[C] user context d={d}: fp32 oracle against fp64, worst err/tol {worst:.3f}")


@pytest.mark.parametrize("H", C.FUSED_H)
def test_fp32_headroom_fused_user_context(H):
    worst = 0.0
    cases = [c for c in C.FUSED_CASES if c[0] == H]
    for _, C1, d, B in cases:
        for gain in C.GAINS:
            for lists in (False, True):
                c = C.fused_inputs(H, C1, d, B, gain, lists)
                worst = _budget(f"fused H={H} C1={C1} d={d} B={B} gain={gain} lists={lists}", C.fused_eval(c, C1, torch.float32), C.fused_eval(c, C1),
                                C.OUT_TOL, QUARTER, worst)
    print(f"[D] fused H={H}: fp32 against fp64, worst err/tol {worst:.3f} over {len(cases)} cases x {len(C.GAINS)} gains x 2")
