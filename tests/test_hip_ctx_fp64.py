"""GPU suite: the context stage (compute_news_graph_context, compute_user_graph_context: csrc/digat_context.inc, csrc/digat_ctxfused.inc)
against fp64 references over every pooling kernel, size and width at which the code changes its path (the case lists and what each
is chosen for: tests/ctx_fp64_common.py).  tests/test_ctx_fp64_cpu.py pins the references to the golden fixtures and the oracle and
holds fp32 arithmetic alone to a quarter (BLAS sums) / half (scores as one fp32 chain) of the tolerances used here.

  A  attention pooling alone through digat_pool_fwd, the dispatch inference takes: the eight attn_pool_resident_kernel<NPW, U> and
     attn_pool_kernel; digat_attn_pool_fwd (always attn_pool_kernel) on the same inputs, its alpha held to the fp64 weights
  B  topic pooling alone through digat_topic_pool_fwd and, with the encoder's row_group / live / hlast lists, digat_topic_pool_lists_fwd:
     topic_pool_resident_kernel<13>, <16> and topic_pool_kernel at one to four category tiles
  C  digat_news_ctx_fwd and digat_user_ctx_fwd / _grouped whole against the oracle on double parameters, as three-row calls and from
     2 048 GEMM rows
  D  user_ctx_fused_kernel alone through digat_user_ctx_fused_fwd, against fp64 and against digat_user_ctx_fwd's three launches

Tolerances are the project's: context outputs rtol = atol = 2e-5 (tests/test_hip_user_ctx0.py, tests/test_hip_train_primitives.py),
attention weights 1e-5 / 1e-6 (eq8_fp64_common.ALPHA_TOL), the one launch against the three 2e-6 / 2e-6 (tests/test_hip_parity.py).
Outputs start as NaN, workspaces are filled with 0xFF bytes before every call, and every result must be finite.

Worst err / tol per block, measured on an MI355X (every figure is to stay below 1; nothing is tuned to them), with the CPU file's fp32
figures beside them:
    A  attention pooling      out 0.097 (n = 12), digat_attn_pool_fwd's alpha 0.123 (n = 20)           fp32 on a CPU: 0.144 with BLAS sums, 0.496 as a chain
    B  topic pooling          0.108 (H = 64); with the lists 0.469 (H = 256), 0.115 elsewhere          fp32 on a CPU: 0.163 / 0.493
    C  entries whole          news context 0.060 (N = 65), user context 0.167 (H = 65)                 the fp32 oracle on a CPU: 0.041 / 0.072
    D  the one launch         against fp64 0.118 (H = 51); against the three launches 0.631 (H = 4)    fp32 on a CPU: 0.228
The CPU figures are those tests/test_ctx_fp64_cpu.py prints and holds to 0.25 (BLAS sums, every block) and 0.5 (the chain, A and B) on
the same cases: the kernels are about as far from fp64 as fp32 arithmetic is.  The whole file takes about eight seconds.
"""
import functools

import pytest
import torch

import ctx_fp64_common as C
from oracle import digat_oracle as O

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_SHAPE = 0, 1, 2


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _L():
    from digat_amd import _lib
    return _lib.lib()


def _S():
    from digat_amd import _lib
    return _lib.stream_ptr()


def _nan(*shape):
    return torch.full(shape, C.NAN, device=_dev())


def _d(t):
    """On the device, contiguous; a tensor without elements (H = 0) becomes a 16-element buffer, so that its pointer is not NULL."""
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.to(_dev()).contiguous() if t.numel() else torch.zeros(16, dtype=t.dtype, device=_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes):
    """A workspace of its own, filled with 0xFF bytes (NaN as floats)."""
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=_dev())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(block, what, cases, **worst):
    print(f"[{block}] {what}: worst err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" over {cases} cases")


# ---- A: attention pooling alone --------------------------------------------------------------------------------------------------
def _pool_call(feat, ld_b, kq, mask, addend, B, n, d):
    out = _nan(B, d)
    assert _L().digat_pool_fwd(feat.data_ptr(), ld_b, kq.data_ptr(), mask.data_ptr(), _ptr(addend), out.data_ptr(), B, n, d, _S()) == OK
    return out


def _pool(n, d, gain):
    """(worst err/tol of the outputs, of digat_attn_pool_fwd's alpha)"""
    feat, kq, mask, addend = C.pool_inputs(n, d, gain)
    want, want_alpha = C.pool_eval(feat, kq, mask)
    B = feat.shape[0]
    assert B <= 8
    fd, kd, md, ad = _d(feat), _d(kq), _d(mask), _d(addend)
    what = f"pool n={n} d={d} gain={gain} {C.route_pool(n, d)}"
    got = _pool_call(fd, n * d, kd, md, None, B, n, d)
    got_add = _pool_call(fd, n * d, kd, md, ad, B, n, d)
    o = C.close(got, want, what, **C.OUT_TOL)
    o = max(o, C.close(got_add, want + addend.double(), what + " + addend", **C.OUT_TOL))
    assert _same_bits(got_add, ad + got), what + ": the addend joins after the sum"
    if (n, d) in C.POOL_LD:                                             # rows of stride n d + 8 with NaN in the gap
        wide = _nan(B, n * d + C.POOL_LD_PAD)
        wide[:, :n * d] = fd.view(B, n * d)
        assert _same_bits(_pool_call(wide, n * d + C.POOL_LD_PAD, kd, md, None, B, n, d), got), what + ": ld_b"
    # the two-pass kernel on the same inputs, and its alpha
    out2, alpha = _nan(B, d), _nan(B, n)
    assert _L().digat_attn_pool_fwd(fd.data_ptr(), n * d, kd.data_ptr(), md.data_ptr(), out2.data_ptr(), alpha.data_ptr(), B, n, d, _S()) == OK
    torch.cuda.synchronize()
    o = max(o, C.close(out2, want, what + ": digat_attn_pool_fwd", **C.OUT_TOL))
    o = max(o, C.close(got, out2.double().cpu(), what + " against digat_attn_pool_fwd", **C.OUT_TOL))
    al = C.close(alpha, want_alpha, what + ": alpha", **C.ALPHA_TOL)
    a, some = alpha.double().cpu(), mask.any(dim=1)
    assert bool((a[some][~mask[some]] == 0).all()), what + ": a masked node's weight is not exactly 0"
    assert float((a.sum(dim=1) - 1).abs().max()) <= 1e-6, what + f": alpha rows sum to 1 +- {float((a.sum(dim=1) - 1).abs().max()):.2e}"
    return o, al


@pytest.mark.parametrize("n", C.POOL_N)
def test_attention_pooling_kernels_against_fp64(n):
    res = [_pool(n, d, gain) for m, d in C.POOL_SHAPES if m == n for gain in C.gains("pool", n, d)]
    _report("A", f"pool n={n}", len(res), out=max(r[0] for r in res), alpha=max(r[1] for r in res))


# ---- B: topic pooling alone ------------------------------------------------------------------------------------------------------
def _topic_lists_call(Xu, ld_b, kq, idx, rg, live, live_ld, hlast, B, H, C1, d):
    out = _nan(B, C1, d)
    assert _L().digat_topic_pool_lists_fwd(Xu.data_ptr(), ld_b, kq.data_ptr(), idx.data_ptr(), _ptr(rg), _ptr(live), live_ld, _ptr(hlast),
                                           out.data_ptr(), B, H, C1, d, _S()) == OK
    return out


def _topic(H, C1, d, gain):
    """(worst err/tol without lists, with lists)"""
    U, ld_live = H + C.TOPIC_EXTRA_NODES, H + C.TOPIC_LIVE_PAD
    what = f"topic H={H} C1={C1} d={d} gain={gain} {C.route_topic(H, C1, d)[0]}"
    # digat_topic_pool_fwd
    Xu, kq, idx = C.topic_inputs(H, C1, d, gain)
    B = Xu.shape[0]
    assert B <= 8
    want, empty = C.topic_eval(Xu[:, :H], kq, idx, C1)
    Xd, kd, idd = _d(Xu), _d(kq), _d(idx)
    got = _nan(B, C1, d)
    assert _L().digat_topic_pool_fwd(Xd.data_ptr(), kd.data_ptr(), idd.data_ptr(), got.data_ptr(), B, U, H, C1, d, _S()) == OK
    plain = C.close(got, want, what, **C.OUT_TOL)
    assert bool((got.cpu()[empty] == 0).all()), what + ": an empty bucket is not exactly zero"
    # the lists entry without lists and with an all-live list: the same bits
    assert _same_bits(_topic_lists_call(Xd, U * d, kd, idd, None, None, 0, None, B, H, C1, d), got), what + ": lists entry, no list"
    ones, full = torch.ones(B, ld_live, dtype=torch.uint8, device=_dev()), torch.full((B,), H, dtype=torch.int32, device=_dev())
    assert _same_bits(_topic_lists_call(Xd, U * d, kd, idd, None, ones, ld_live, None, B, H, C1, d), got), what + ": all-live list"
    assert _same_bits(_topic_lists_call(Xd, U * d, kd, idd, None, ones, ld_live, full, B, H, C1, d), got), what + ": all-live list, hlast = H"
    # live and hlast, one graph per row
    Xl, kql, idxl, flags, hlast = C.topic_list_inputs(H, C1, d, gain)
    want_l, empty_l = C.topic_eval(Xl[:, :H], kql, idxl, C1, live=flags[:, :H])
    Xld, kld, ild, fld, hld = _d(Xl), _d(kql), _d(idxl), _d(flags), _d(hlast)
    Bl = Xl.shape[0]
    with_h = _topic_lists_call(Xld, U * d, kld, ild, None, fld, ld_live, hld, Bl, H, C1, d)
    without_h = _topic_lists_call(Xld, U * d, kld, ild, None, fld, ld_live, None, Bl, H, C1, d)
    lists = C.close(with_h, want_l, what + " live + hlast", **C.OUT_TOL)
    assert _same_bits(with_h, without_h), what + ": live without hlast gives other bits than with it"
    assert bool((with_h.cpu()[empty_l] == 0).all()), what + " live + hlast: an empty bucket is not exactly zero"
    # ... and through row_group: two groups, not in contiguous runs
    Xg, rg, kqg, idxg, flagsg, hlastg = C.topic_group_inputs(H, C1, d, gain)
    want_g, _ = C.topic_eval(Xg[rg.long()][:, :H], kqg, idxg, C1, live=flagsg[:, :H])
    grouped = _topic_lists_call(_d(Xg), U * d, _d(kqg), _d(idxg), _d(rg), _d(flagsg), ld_live, _d(hlastg), rg.shape[0], H, C1, d)
    torch.cuda.synchronize()
    lists = max(lists, C.close(grouped, want_g, what + " row_group + live + hlast", **C.OUT_TOL))
    return plain, lists


@pytest.mark.parametrize("H", C.TOPIC_H)
def test_topic_pooling_kernels_against_fp64(H):
    res = [_topic(H, C1, d, gain) for h, C1, d in C.TOPIC_SHAPES if h == H for gain in C.gains("topic", H, C1, d)]
    _report("B", f"topic H={H}", len(res), plain=max(r[0] for r in res), lists=max(r[1] for r in res))


def test_list_entries_refuse_what_the_kernels_would_ignore():
    L = _L()
    p = torch.zeros(64, device=_dev()).data_ptr()
    assert L.digat_topic_pool_lists_fwd(p, 72, p, p, None, None, 0, p, p, 1, 2, 18, 36, None) == ERR_ARG        # hlast without live
    assert L.digat_topic_pool_lists_fwd(p, 72, p, p, None, p, 1, None, p, 1, 2, 18, 36, None) == ERR_ARG        # live_ld < H
    assert L.digat_topic_pool_lists_fwd(p, 74, p, p, None, None, 0, None, p, 1, 2, 18, 36, None) == ERR_SHAPE   # ld_b % 4
    assert L.digat_topic_pool_lists_fwd(p, 72, p, p, None, None, 0, None, p, 1, 2, 65, 36, None) == ERR_SHAPE   # five category tiles
    assert L.digat_topic_pool_lists_fwd(p, 72, p, p, None, None, 0, None, p, 0, 2, 18, 36, None) == OK          # B == 0: no launch
    assert L.digat_pool_fwd(p, 36, p, None, None, p, 1, 1, 36, None) == ERR_ARG
    assert L.digat_pool_fwd(p, 36, p, p, None, p, 1, 129, 36, None) == ERR_SHAPE and L.digat_pool_fwd(p, 38, p, p, None, p, 1, 1, 36, None) == ERR_SHAPE
    assert L.digat_pool_fwd(p, 36, p, p, None, p, 0, 1, 36, None) == OK


# ---- C: the per-function entries whole -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _weights(d, Ctopics):
    """(fp64 parameters, device fp32 weights by name) of ctx_state(d, C)."""
    state = C.ctx_state(d, Ctopics)
    return C.f64_params(state), {k: torch.from_numpy(v).to(_dev()).contiguous() for k, v in state.items()}


def _news(N, d):
    p64, w = _weights(d, 17)
    X, mask, addend = C.news_inputs(N, d)
    with torch.no_grad():
        want = O.news_graph_context(p64, X.double(), mask)
    wp = [w[k].data_ptr() for k in ("candidate_attention.K.weight", "candidate_attention.Q.weight", "candidate_attention.Q.bias",
                                    "news_graph_W.weight", "news_graph_W.bias")]
    worst = 0.0
    for rep in (1, -(-C.BIG_ROWS // C.ROWS)):                           # three rows; from 2 048 rows the other GEMM family
        B = C.ROWS * rep
        Xd, md, ad = _d(X).repeat(rep, 1, 1), _d(mask).repeat(rep, 1), _d(addend).repeat(rep, 1)
        nb = _L().digat_news_ctx_workspace_bytes(B, N, d)
        for add in (None, ad):
            out, ws = _nan(B, d), _ws(nb)
            assert _L().digat_news_ctx_fwd(Xd.data_ptr(), md.data_ptr(), *wp, _ptr(add), out.data_ptr(), B, N, d, ws.data_ptr(), nb, _S()) == OK
            ref = (want if add is None else want + addend.double()).repeat(rep, 1)
            worst = max(worst, C.close(out, ref, f"news context N={N} d={d} B={B} addend={add is not None}", **C.OUT_TOL))
    return worst


@pytest.mark.parametrize("N", C.NEWS_N)
def test_news_context_entry_against_the_fp64_oracle(N):
    res = [_news(N, d) for n, d in C.NEWS_SHAPES if n == N]
    _report("C", f"news context N={N}", len(res), out=max(res))


USER_W = ("user_news_K.weight", "user_news_Q.weight", "user_news_Q.bias", "featureAffine.weight", "featureAffine.bias",
          "userAttention.K.weight", "userAttention.Q.weight", "userAttention.Q.bias")


def _user_call(wp, Xu, mask, idx, c_n, add, B, U, H, C1, d):
    nb = _L().digat_user_ctx_workspace_bytes(B, U, H, C1, d)
    out, ws = _nan(B, d), _ws(nb)
    assert _L().digat_user_ctx_fwd(Xu.data_ptr(), mask.data_ptr(), idx.data_ptr(), c_n.data_ptr(), *wp, _ptr(add), out.data_ptr(),
                                   B, U, H, C1, d, ws.data_ptr(), nb, _S()) == OK
    return out


def _user(H, C1, d):
    p64, w = _weights(d, C1 - 1)
    wp = [w[k].data_ptr() for k in USER_W]
    Xu, mask, idx, c_n, addend = C.user_inputs(H, C1, d)
    U = Xu.shape[1]
    with torch.no_grad():
        want = C.user_context(p64, Xu.double(), mask, idx, c_n.double(), H)
    Xd, md, idd, cd, ad = _d(Xu), _d(mask), _d(idx), _d(c_n), _d(addend)
    what = f"user context H={H} C1={C1} d={d}"
    worst = 0.0
    for lo in (0, 2):                                                   # three rows a call: users 0 .. 2 and 2 .. 4
        s = slice(lo, lo + C.ROWS)
        for add in (None, ad[s].contiguous()):
            out = _user_call(wp, Xd[s].contiguous(), md[s].contiguous(), idd[s].contiguous(), cd[s].contiguous(), add, C.ROWS, U, H, C1, d)
            ref = want[s] if add is None else want[s] + addend[s].double()
            worst = max(worst, C.close(out, ref, f"{what} rows {lo}..{lo + 2} addend={add is not None}", **C.OUT_TOL))
    rep = -(-C.BIG_ROWS // (5 * C1))                                    # B (C + 1) >= 2 048: featureAffine on the other GEMM family
    for add in (None, ad.repeat(rep, 1)):
        out = _user_call(wp, Xd.repeat(rep, 1, 1), md.repeat(rep, 1), idd.repeat(rep, 1), cd.repeat(rep, 1), add, 5 * rep, U, H, C1, d)
        ref = (want if add is None else want + addend.double()).repeat(rep, 1)
        worst = max(worst, C.close(out, ref, f"{what} B={5 * rep} addend={add is not None}", **C.OUT_TOL))
    # grouped and expanded calls: equal bits
    rg = torch.tensor(C.USER_GROUP_OF_ROW)
    c7, a7 = c_n[(rg + 1) % 5].contiguous(), addend[(rg + 2) % 5].contiguous()
    with torch.no_grad():
        want7 = C.user_context(p64, Xu[rg].double(), mask[rg], idx[rg], c7.double(), H) + a7.double()
    rgd, c7d, a7d = _d(rg.to(torch.int32)), _d(c7), _d(a7)
    expanded = _user_call(wp, Xd[rgd.long()].contiguous(), md[rgd.long()].contiguous(), idd[rgd.long()].contiguous(), c7d, a7d, 7, U, H, C1, d)
    nb = _L().digat_user_ctx_grouped_workspace_bytes(7, 5, U, H, C1, d)
    grouped, ws = _nan(7, d), _ws(nb)
    assert _L().digat_user_ctx_fwd_grouped(Xd.data_ptr(), md.data_ptr(), idd.data_ptr(), rgd.data_ptr(), c7d.data_ptr(), *wp, a7d.data_ptr(),
                                           grouped.data_ptr(), 7, 5, U, H, C1, d, ws.data_ptr(), nb, _S()) == OK
    torch.cuda.synchronize()
    worst = max(worst, C.close(grouped, want7, f"{what} grouped", **C.OUT_TOL))
    assert _same_bits(grouped, expanded), f"{what}: grouped and expanded calls give other bits"
    return worst


@pytest.mark.parametrize("H", C.USER_H)
def test_user_context_entries_against_the_fp64_oracle(H):
    res = [_user(H, C1, d) for h, C1, d in C.USER_SHAPES if h == H]
    _report("C", f"user context H={H}", len(res), out=max(res))


# ---- D: the one-launch user context alone ----------------------------------------------------------------------------------------
def _fused_call(c, image, add, flag, B, H, C1, d, lists):
    out = _nan(B, d)
    if lists:                                                           # row b reads group B - 1 - b; live_ld = H + 1
        Xu, rg, live, live_ld, hlast = c["x"].flip(0).contiguous(), torch.arange(B - 1, -1, -1, dtype=torch.int32, device=_dev()), c["live"], H + 1, c["hlast"]
    else:
        Xu, rg, live, live_ld, hlast = c["x"], None, None, 0, None
    assert _L().digat_user_ctx_fused_fwd(Xu.data_ptr(), H * d, _ptr(rg), _ptr(live), live_ld, _ptr(hlast), c["kq_t"].data_ptr(), c["kq_u"].data_ptr(),
                                         c["idx"].data_ptr(), c["mask"].data_ptr(), _ptr(add), out.data_ptr(), image.data_ptr(), c["bFa"].data_ptr(),
                                         flag.data_ptr(), B, H, C1, d, _S()) == OK
    return out


def _three_launches(c, B, H, C1, d):
    """digat_user_ctx_fwd on the same rows: identity K / Q hand it the topic query c_n = kq_t, a permutation the user query kq_u."""
    eye, zero = torch.eye(d, device=_dev()), torch.zeros(d, device=_dev())
    P = torch.zeros(d, d, device=_dev())
    P[torch.arange(d, device=_dev()), c["perm"]] = 1.0                  # (P c)[i] = c[perm[i]]
    wp = [eye.data_ptr(), eye.data_ptr(), zero.data_ptr(), c["Fa"].data_ptr(), c["bFa"].data_ptr(), eye.data_ptr(), P.data_ptr(), zero.data_ptr()]
    return _user_call(wp, c["x"], c["mask"], c["idx"], c["kq_t"], None, B, H, H, C1, d)


def _fused(H, C1, d, B, gain, lists):
    """(worst err/tol against fp64, against the three launches or None)"""
    host = C.fused_inputs(H, C1, d, B, gain, lists)
    want = C.fused_eval(host, C1)
    c = {k: _d(v) for k, v in host.items()}
    image = torch.full((int(_L().digat_split_ctx_fused_bytes(d)),), 0xFF, dtype=torch.uint8, device=_dev())
    assert _L().digat_split_ctx_fused_weights(c["Fa"].data_ptr(), d, image.data_ptr(), _S()) == OK
    flag = torch.zeros(1, dtype=torch.int32, device=_dev())
    what = f"fused H={H} C1={C1} d={d} B={B} gain={gain} lists={lists}"
    got = _fused_call(c, image, None, flag, B, H, C1, d, lists)
    got_add = _fused_call(c, image, c["addend"], flag, B, H, C1, d, lists)
    o = C.close(got, want, what, **C.OUT_TOL)
    assert _same_bits(got_add, c["addend"] + got), what + ": the addend joins after the sum"
    three = None
    if not lists and gain == C.FUSED_LAUNCHES_GAIN:
        old = _three_launches(c, B, H, C1, d)
        torch.cuda.synchronize()
        three = C.close(got, old.double().cpu(), what + " against digat_user_ctx_fwd", **C.FUSED_VS_LAUNCHES)
    assert int(flag.item()) == 0, what + ": the range flag is raised"
    return o, three


@pytest.mark.parametrize("H", C.FUSED_H)
def test_fused_user_context_kernel_against_fp64_and_the_three_launches(H):
    res = [_fused(H, C1, d, B, gain, lists) for h, C1, d, B in C.FUSED_CASES if h == H for gain in C.GAINS for lists in (False, True)]
    _report("D", f"fused H={H}", len(res), fp64=max(r[0] for r in res), three_launches=max(r[1] for r in res if r[1] is not None))


def test_fused_entry_refuses_what_the_kernel_cannot_take():
    L = _L()
    p = torch.zeros(64, device=_dev()).data_ptr()
    call = lambda H, C1, d, B=4, live=None, hlast=None, live_ld=0: L.digat_user_ctx_fused_fwd(p, H * d, None, live, live_ld, hlast, p, p, p, p, None, p, p, p,
                                                                                               None, B, H, C1, d, None)
    for H, C1, d in C.FUSED_REFUSED:                                    # H = 53, C + 1 = 21, d = 192, 456 and 244
        assert call(H, C1, d) == ERR_SHAPE, (H, C1, d)
    assert call(50, 18, 400, hlast=p) == ERR_ARG and call(50, 18, 400, live=p, live_ld=49) == ERR_ARG
    assert call(50, 18, 400, B=0) == OK                                 # B == 0: no launch
