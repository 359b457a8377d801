"""GPU suite: what is left of a training step once the attention side is held, every kernel alone against a high-precision
reference at the sizes where its code changes its path (the case lists and what each is chosen for: tests/step_fp64_common.py).
tests/test_step_fp64_cpu.py pins the references to the oracle and the golden fixtures and holds the stock fp32 formulations to half of
the tolerances used here.

  A  the GAT layer (csrc/digat_gat.inc: gat_node_scores_kernel, gat_alpha_kernel, gat_score_bwd_kernel) through digat_gat_fwd and the
     pair digat_gat_fwd_train / digat_gat_bwd at p_alpha = 0 and 0.3, against gat_fp64 under fp64 autograd with the kernels' keep bits
  B  the table gradients (csrc/digat_news_train.inc) through digat_embedding_bwd — embedding_bwd_kernel at one, two and three
     levels over hand-built token layouts — and digat_embedding_bwd_unsorted — the chunk and merge kernels at U = 1, 2 and 4 over
     hand-built id patterns: integer rows bit for bit, normal rows under count 2^-24 sum|rows| per element
  C  digat_row_logits / _bwd, digat_click_loss and training.ClickLoss, optim.ClipAdam (grad_sq_chunks_kernel, grad_sq_total_kernel with
     up to and beyond 1024 partials, clip_adam_kernel on its vector and scalar paths) against fp64

Every call goes through the ctypes table of digat_amd/_lib.py or the existing training.* Functions and optim.ClipAdam.  Outputs start
as NaN, workspaces and save buffers are filled with 0xFF bytes at exactly the size their query returns, and a second run on 0x00
bytes must give the same bits.  The one exception is the table gradient itself, which both entries ask the caller to zero-fill (rows
of ids that do not occur stay zero): it starts as zeros, and those rows are held to exactly 0.

Worst err / tol per block, measured on an MI355X (every figure is to stay below 1; nothing is tuned to them), with the CPU file's fp32
figures beside them:
    A  GAT layer              forward 0.344 (d = 1024; both entries), gradients 0.240 (n = 113)         the fp32 oracle on a CPU: 0.208 / 0.328
    B  normal rows            sorted 0.388 (M = 2049), unsorted 0.167 (dm = 256); integer rows equal    F.embedding's backward: 0.388 / 0.167
    C  head and tail          logits 0.116, loss 0.130, d logits 0.088, Adam 0.033 (step 10 000)       torch in fp32: 0.201, 0.136, 0.136, 0.028
The 1025-chunk Adam case stands at 0.005 (torch in fp32: 0.040).  The kernels are about as far from fp64 as fp32 arithmetic is.  This file takes
about ten seconds; with tests/test_step_fp64_cpu.py the whole suite went from 332 s to 346 s on the GPU machine.

NOT held by block A: digat_gat_bwd reads relu'(Z) off out - X > 0 (relu_res_mask_kernel), which is 0 where a positive Z lies below half an
ulp of X.  The case builder (step_fp64_common._gat_off_the_kinks) sets the cotangent to zero at exactly those elements, at most 0.1 %
of a case, so the sweep never compares that mask with relu' of Z there: it holds the arithmetic, not this design choice.

Found by this file: click_loss_kernel formed lse = m + log z and subtracted the clicked logit from it, which rounds at the size of the
largest logit — a loss of 1.1 under logits of +-100 came out 2.3e-6 off (1.10 of the tolerance, B = 1, K = 300, logits scaled by 30).
It now takes (x - m) - log z, as torch.log_softmax does; the case stays in LOSS_KINDS.
"""
import pytest
import torch

import step_fp64_common as C

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_SHAPE = C.OK, C.ERR_ARG, C.ERR_SHAPE


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
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.to(_dev()).contiguous()


def _bytes(nbytes, fill):
    """A buffer of exactly ``nbytes`` bytes, every one ``fill``."""
    assert nbytes > 0
    return torch.full((int(nbytes),), fill, dtype=torch.uint8, device=_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(block, what, cases, **worst):
    print(f"[{block}] {what}: worst err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" over {cases} cases")


# ---- A: the GAT layer --------------------------------------------------------------------------------------------------------------
def _gat_fwd(t, B, n, d, fill=0xFF):
    nb = _L().digat_gat_workspace_bytes(B, n, d)
    out, ws = _nan(B, n, d), _bytes(nb, fill)
    rc = _L().digat_gat_fwd(t["X"].data_ptr(), t["A"].data_ptr(), t["W"].data_ptr(), t["bW"].data_ptr(), t["a1"].data_ptr(), t["a2"].data_ptr(),
                            out.data_ptr(), B, n, d, ws.data_ptr(), nb, _S())
    return rc, out


def _gat_pair(t, B, n, d, p, fill=0xFF):
    """(rc, out, [dX, dW, dbW, da1, da2]) of digat_gat_fwd_train + digat_gat_bwd; the workspace is refilled between the two (one buffer
    serves both directions and carries nothing from one to the other)."""
    L = _L()
    nsave, nws = L.digat_gat_train_save_bytes(B, n, d), L.digat_gat_train_workspace_bytes(B, n, d)
    save, ws, out = _bytes(nsave, fill), _bytes(nws, fill), _nan(B, n, d)
    w = [t[k].data_ptr() for k in ("W", "bW", "a1", "a2")]
    rc = L.digat_gat_fwd_train(t["X"].data_ptr(), t["A"].data_ptr(), *w, out.data_ptr(), p, C.GAT_SEED, B, n, d, save.data_ptr(), nsave,
                               ws.data_ptr(), nws, _S())
    if rc != OK:
        return rc, out, None
    ws.fill_(fill)
    grads = [_nan(B, n, d), _nan(d, d), _nan(d), _nan(d), _nan(d)]
    rc = L.digat_gat_bwd(t["dOut"].data_ptr(), out.data_ptr(), t["X"].data_ptr(), t["A"].data_ptr(), t["W"].data_ptr(), t["a1"].data_ptr(),
                         t["a2"].data_ptr(), p, save.data_ptr(), nsave, *(g.data_ptr() for g in grads), B, n, d, ws.data_ptr(), nws, _S())
    return rc, out, grads


def _gat(case, x3=False):
    """(worst err/tol of the inference output, of the training outputs, of the gradients)"""
    n, d, B, kind = case
    X, dOut, A, w = C.gat_inputs(case)
    t = dict(X=_d(X), dOut=_d(dOut), A=_d(A), W=_d(w["W"]), bW=_d(w["bW"]), a1=_d(w["a1"]), a2=_d(w["a2"]))
    what = f"GAT {tuple(case)}"
    if d in C.GAT_REFUSED:                                              # refused before any launch: nothing is written
        rc, out = _gat_fwd(t, B, n, d)
        rc_t, out_t, _ = _gat_pair(t, B, n, d, 0.0)
        # ... and the backward on its own: buffers of the sizes the queries give, every gradient NaN before and after
        nsave, nws = _L().digat_gat_train_save_bytes(B, n, d), _L().digat_gat_train_workspace_bytes(B, n, d)
        save, ws, grads = _bytes(nsave, 0xFF), _bytes(nws, 0xFF), [_nan(B, n, d), _nan(d, d), _nan(d), _nan(d), _nan(d)]
        rc_b = _L().digat_gat_bwd(t["dOut"].data_ptr(), t["X"].data_ptr(), t["X"].data_ptr(), t["A"].data_ptr(), t["W"].data_ptr(), t["a1"].data_ptr(),
                                  t["a2"].data_ptr(), 0.0, save.data_ptr(), nsave, *(g.data_ptr() for g in grads), B, n, d, ws.data_ptr(), nws, _S())
        torch.cuda.synchronize()
        assert rc == rc_t == rc_b == C.GAT_REFUSED[d], (what, rc, rc_t, rc_b)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(out_t).all()), what + ": a refused call wrote its output"
        assert all(bool(torch.isnan(g).all()) for g in grads), what + ": the refused backward wrote a gradient"
        return None
    # inference
    want0, _ = C.gat_reference(case, 0.0)
    rc, out = _gat_fwd(t, B, n, d)
    assert rc == OK, (what, rc)
    o_inf = C.close(out, want0, what + " digat_gat_fwd", **C.OUT_TOL)
    assert _same_bits(_gat_fwd(t, B, n, d, fill=0x00)[1], out), what + ": 0x00 and 0xFF workspaces give other bits"
    if B > 1:                                                           # the graphs in another order: the same rows, bit for bit
        perm = torch.arange(B - 1, -1, -1, device=_dev())
        tp = dict(t, X=t["X"][perm].contiguous(), A=t["A"][perm].contiguous())
        assert _same_bits(_gat_fwd(tp, B, n, d)[1], out[perm]), what + ": permuting the graphs changes bits"
    # the training pair
    o_train = g_worst = 0.0
    for p in C.GAT_P:
        want, wgrads = C.gat_reference(case, p)
        rc, out_t, grads = _gat_pair(t, B, n, d, p)
        assert rc == OK, (what, p, rc)
        # (inference's OUT_TOL where the two forwards are the same function)
        o_train = max(o_train, C.close(out_t, want, f"{what} p={p} digat_gat_fwd_train", **(C.OUT_TOL if p == 0 else C.TRAIN_OUT_TOL)))
        for k, g in zip(C.GAT_GRADS, grads):
            g_worst = max(g_worst, C.close(g.view(wgrads[k].shape), wgrads[k], f"{what} p={p} grad {k}", **C.GRAD_TOL))
        if p == 0 and not x3:                                           # (from 2048 rows with d % 80 == 0 the two entries' GEMM routes differ)
            assert _same_bits(out_t, out), what + ": digat_gat_fwd and digat_gat_fwd_train at p = 0 give other bits"
        if kind == "none":
            assert float(grads[3].abs().max()) == 0.0 and float(grads[4].abs().max()) == 0.0, what + ": da1 / da2 are not exactly zero"
            assert float(grads[0].abs().max()) > 0.0
        rc, out_z, grads_z = _gat_pair(t, B, n, d, p, fill=0x00)
        assert rc == OK and _same_bits(out_z, out_t) and all(_same_bits(a, b) for a, b in zip(grads_z, grads)), \
            f"{what} p={p}: 0x00 and 0xFF buffers give other bits"
    torch.cuda.synchronize()
    return o_inf, o_train, g_worst


def _gat_sweep(what, cases, x3=False):
    res = [r for r in (_gat(c, x3) for c in cases) if r is not None]
    if res:
        _report("A", what, len(res), fwd=max(r[0] for r in res), fwd_train=max(r[1] for r in res), gradients=max(r[2] for r in res))
    else:
        print(f"[A] {what}: {len(cases)} cases refused with DIGAT_ERR_SHAPE")


@pytest.mark.parametrize("n", C.GAT_N)
def test_gat_layer_against_fp64_over_n(n):
    _gat_sweep(f"GAT n={n}", [c for c in C.GAT_CASES if c.n == n and c.d in C.GAT_D_ALL_N])


@pytest.mark.parametrize("d", C.GAT_D)
def test_gat_layer_against_fp64_over_d(d):
    _gat_sweep(f"GAT d={d}", [c for c in C.GAT_CASES if c.d == d and c.n in C.GAT_N_ALL_D])


@pytest.mark.parametrize("case", C.GAT_X3, ids=lambda c: f"B{c.B}-n{c.n}-d{c.d}")
def test_gat_layer_against_fp64_on_the_bf16x6_routes(case):
    from digat_amd import training
    assert training._x3_ok(case.B * case.n, case.d, case.d)
    _gat_sweep(f"GAT {tuple(case)}", [case], x3=True)


# ---- B: the table gradients --------------------------------------------------------------------------------------------------------
def _sorted_call(rows_dev, ld, order, stok, M, dm, V, fill):
    nb = _L().digat_embedding_bwd_workspace_bytes(M, dm)
    table, ws = torch.zeros(V, dm, device=_dev()), _bytes(nb, fill)
    assert _L().digat_embedding_bwd(rows_dev.data_ptr(), ld, order.data_ptr(), stok.data_ptr(), M, dm, table.data_ptr(), ws.data_ptr(), nb, _S()) == OK
    return table


def _sorted(M, dm):
    worst = 0.0
    for layout in C.SORTED_LAYOUTS:
        tokens, order, stok, V = C.sorted_case(layout, M)
        od, sd = _d(torch.from_numpy(order)), _d(torch.from_numpy(stok))
        for pad in C.SORTED_LD_PAD:
            for exact in (True, False):
                rows = C.table_rows(M, dm, exact, layout)
                buf, ld = C.padded(rows, pad)
                bd = _d(buf)
                what = f"digat_embedding_bwd M={M} dm={dm} ld={ld} {layout} exact={exact} ({C.sorted_levels(M)} levels)"
                got = _sorted_call(bd, ld, od, sd, M, dm, V, 0xFF)
                worst = max(worst, C.table_check(got, tokens, rows, V, exact, what))
                if pad:
                    assert _same_bits(_sorted_call(bd, ld, od, sd, M, dm, V, 0x00), got), what + ": 0x00 and 0xFF workspaces give other bits"
    return worst


@pytest.mark.parametrize("M", C.SORTED_M)
def test_sorted_table_gradient_alone(M):
    dms = [dm for m, dm in C.SORTED_SHAPES if m == M]
    worst = max(_sorted(M, dm) for dm in dms)
    torch.cuda.synchronize()
    _report("B", f"sorted M={M}", len(dms) * len(C.SORTED_LAYOUTS) * 4, normal_rows=worst)


def _unsorted_call(ids0, g0, ld0, M0, ids1, g1, ld1, M1, dm, V, fill):
    nb = _L().digat_embedding_bwd_unsorted_workspace_bytes(M0 + M1, dm, V)
    table, ws = torch.zeros(V, dm, device=_dev()), _bytes(nb, fill)
    assert _L().digat_embedding_bwd_unsorted(_ptr(ids0), _ptr(g0), ld0, M0, _ptr(ids1), _ptr(g1), ld1, M1, dm, V, table.data_ptr(), ws.data_ptr(), nb, _S()) == OK
    return table


def _unsorted(dm, M0, M1, V):
    ids, _ = C.unsorted_ids(M0, M1, V)
    idt = torch.from_numpy(ids)
    ids0, ids1 = (_d(idt[:M0]) if M0 else None), (_d(idt[M0:]) if M1 else None)             # an empty list is passed as NULL
    worst = 0.0
    for exact in (True, False):
        rows = C.table_rows(M0 + M1, dm, exact, V)
        (b0, ld0), (b1, ld1) = C.padded(rows[:M0], C.UNSORTED_LD_PAD[0]), C.padded(rows[M0:], C.UNSORTED_LD_PAD[1])
        g0, g1 = (_d(b0) if M0 else None), (_d(b1) if M1 else None)
        what = f"digat_embedding_bwd_unsorted dm={dm} (U={C.unsorted_U(dm)}) M=({M0}, {M1}) V={V} exact={exact}"
        got = _unsorted_call(ids0, g0, ld0, M0, ids1, g1, ld1, M1, dm, V, 0xFF)
        worst = max(worst, C.table_check(got, idt, rows, V, exact, what))
        again = _unsorted_call(ids0, g0, ld0, M0, ids1, g1, ld1, M1, dm, V, 0x00)
        assert _same_bits(again, got), what + ": a second call (on a 0x00 workspace) gives other bits"
    return worst


@pytest.mark.parametrize("dm", C.UNSORTED_DM)
def test_unsorted_table_gradient_alone(dm):
    cases = [c for c in C.UNSORTED_CASES if c[0] == dm]
    worst = max(_unsorted(dm, M0, M1, V) for _, (M0, M1), V in cases)
    torch.cuda.synchronize()
    _report("B", f"unsorted dm={dm}", 2 * len(cases), normal_rows=worst)


# ---- C: the step's head and tail ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", C.LOGITS_D)
def test_row_logits_and_their_backward_against_fp64(d):
    worst_l = worst_g = 0.0
    for B in C.LOGITS_B:
        nc, uc, dl = C.logits_inputs(B, d)
        want, want_dn, want_du = C.logits_eval(nc, uc, dl)
        ncd, ucd, dld = _d(nc), _d(uc), _d(dl)
        logits, dn, du = _nan(B), _nan(B, d), _nan(B, d)
        assert _L().digat_row_logits(ncd.data_ptr(), ucd.data_ptr(), logits.data_ptr(), B, d, _S()) == OK
        assert _L().digat_row_logits_bwd(dld.data_ptr(), ncd.data_ptr(), ucd.data_ptr(), dn.data_ptr(), du.data_ptr(), B, d, _S()) == OK
        torch.cuda.synchronize()
        worst_l = max(worst_l, C.close(logits, want, f"logits B={B} d={d}", **C.LOGIT_TOL))
        worst_g = max(worst_g, C.close(dn, want_dn, f"d news_ctx B={B} d={d}", **C.HEAD_GRAD_TOL), C.close(du, want_du, f"d user_ctx B={B} d={d}", **C.HEAD_GRAD_TOL))
    _report("C", f"row logits d={d}", len(C.LOGITS_B), logits=worst_l, gradients=worst_g)


@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_click_loss_against_fp64(kind):
    from digat_amd import training
    worst_l = worst_g = 0.0
    for B in C.LOSS_B:
        for K in C.LOSS_K:
            x = C.loss_inputs(B, K, kind)
            want, wgrad = C.loss_eval(x)
            xd = _d(x)
            loss, dlogits = _nan(1), _nan(B, K)
            assert _L().digat_click_loss(xd.data_ptr(), B, K, loss.data_ptr(), dlogits.data_ptr(), _S()) == OK
            what = f"click loss B={B} K={K} {kind}"
            worst_l = max(worst_l, C.close(loss.view(()), want, what, **C.LOSS_TOL))
            worst_g = max(worst_g, C.close(dlogits, wgrad, what + ": d logits", **C.HEAD_GRAD_TOL))
            # through training.ClickLoss with an incoming gradient other than 1
            xa = xd.clone().requires_grad_(True)
            la = training.ClickLoss.apply(xa)
            (la * C.LOSS_DLOSS).backward()
            torch.cuda.synchronize()
            assert _same_bits(la.detach().view(1), loss), what + ": training.ClickLoss and the entry give other bits"
            worst_g = max(worst_g, C.close(xa.grad, C.LOSS_DLOSS * wgrad, what + ": training.ClickLoss's gradient", **C.HEAD_GRAD_TOL))
            if K == 1:
                assert float(loss) == 0.0 and float(dlogits.abs().max()) == 0.0 and float(xa.grad.abs().max()) == 0.0, what + ": not exactly 0"
    _report("C", f"click loss {kind}", len(C.LOSS_B) * len(C.LOSS_K), loss=worst_l, gradients=worst_g)


def _unaligned(t):
    """t on the device as a contiguous view one float past a 16-byte boundary."""
    base = torch.zeros(t.numel() + 4, device=_dev())
    view = base[1:1 + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("max_norm,preset", [(m, 0) for m in C.ADAM_MAX_NORMS] + [(1.0, C.ADAM_PRESET_STEP)])
def test_clip_adam_against_fp64(max_norm, preset):
    from digat_amd.optim import ClipAdam
    p0, wds, grads, after, state0 = C.adam_case(max_norm, preset)
    last = len(p0) - 1                                                  # the unaligned tensor
    dev = [(_unaligned(x).detach() if k == last else _d(x).clone()).requires_grad_(True) for k, x in enumerate(p0)]
    assert dev[last].data_ptr() % 16 == 4 and all(q.data_ptr() % 16 == 0 for q in dev[:last])
    opt = ClipAdam([{"params": [q for q, wd in zip(dev, wds) if wd], "weight_decay": C.ADAM_WD},
                    {"params": [q for q, wd in zip(dev, wds) if not wd], "weight_decay": 0.0}], lr=C.ADAM_LR, betas=C.ADAM_BETAS, eps=C.ADAM_EPS)
    if preset:
        for q, m, v in zip(dev, *state0):
            opt.state[q] = {"step": preset, "exp_avg": _d(m).clone(), "exp_avg_sq": _d(v).clone()}
    worst = 0.0
    for s in range(C.ADAM_STEPS):
        for k, (q, g) in enumerate(zip(dev, grads[s])):
            q.grad = _unaligned(g) if k == last else _d(g).clone()
        opt.step(max_norm=max_norm)
        torch.cuda.synchronize()
        for k, q in enumerate(dev):
            worst = max(worst, C.close(q, after[s][k], f"ClipAdam max_norm={max_norm} preset={preset} step {s} tensor {k}", **C.ADAM_TOL))
            assert torch.equal(q.grad.cpu(), grads[s][k]), "the gradients are read, not rescaled"
    assert all(opt.state[q]["step"] == preset + C.ADAM_STEPS for q in dev)
    _report("C", f"ClipAdam max_norm={max_norm} preset={preset}", C.ADAM_STEPS * len(dev), parameters=worst)


def test_clip_adam_beyond_1024_chunks_against_fp64():
    """One tensor of 1024 chunks + 1 element, one step with clipping on: grad_sq_total_kernel's loop over the partials takes a second
    step.  The moments are preset, so that the update is linear in the clipping coefficient, and the last element carries two
    fifths of the squared norm: C.adam_big_check asserts that a total over the first 1024 partials alone would leave most
    parameters outside the tolerance.  The fp64 reference is built on the GPU, as tests/test_hip_nrms.py builds its references."""
    from digat_amd.optim import ClipAdam
    chunk = int(_L().digat_opt_chunk())
    p0, grad, m0, v0 = (_d(x) for x in C.adam_big_case(chunk))
    want = C.adam_big_check(p0, grad, m0, v0, chunk)
    q = p0.clone().requires_grad_(True)
    q.grad = grad.clone()
    opt = ClipAdam([q], lr=C.ADAM_LR, betas=C.ADAM_BETAS, eps=C.ADAM_EPS)
    opt.state[q] = {"step": C.ADAM_BIG_PRESET_STEP, "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    opt.step(max_norm=C.ADAM_BIG_MAX_NORM)
    torch.cuda.synchronize()
    assert torch.equal(q.grad, grad), "the gradients are read, not rescaled"
    assert bool(torch.isfinite(q).all()) and opt.state[q]["step"] == C.ADAM_BIG_PRESET_STEP + 1
    ratio = C.adam_ratio(q.detach(), want)
    worst = float(ratio.max())
    assert worst <= 1.0, f"ClipAdam, 1025 chunks: worst err/tol {worst:.3f} at element {int(ratio.argmax())}"
    _report("C", "ClipAdam 1025 chunks", 1, parameters=worst)
