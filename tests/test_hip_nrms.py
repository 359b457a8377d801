"""GPU suite for the NRMS / NRMS-SA baselines on the HIP kernels (csrc/digat_mhsa.inc through digat_amd/nrms.py and the C ABI):
the vectors minted from the reference's Appendix-B modules (tests/golden/nrms_*.npz), the key-masked attention stage alone against
an fp64 restatement and fp64 autograd, the oracle's hash dropout, and the properties of the entries (gather = dense, T = 0, no read of
uninitialised scratch).  Tolerances: rtol 1e-5 / atol 2e-6 forward and rtol 2e-4 for gradients, the MSA encoder's (tests/test_hip_news.py)."""
import math

import numpy as np
import pytest
import torch

import nrms_common as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _uses_fused(t, name="MhsaFused"):
    todo, seen = [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if name in type(fn).__name__:
            return True
        todo += [f for f, _ in fn.next_functions]
    return False


# ---- golden vectors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", list(C.MODELS))
@pytest.mark.parametrize("name", ["nrms_tiny.npz", "nrms_default.npz"])
def test_hip_inference_matches_reference_vectors(name, pre):
    from digat_amd import nrms
    fx = C.case(name)[0]
    m = C.model(name, pre, _dev()).eval()
    t = C.tensors(name, _dev())
    with torch.no_grad():
        plain, aug = nrms.news_caches(m, t["title_text"], t["title_mask"], t["augmented_title_text"], t["augmented_title_mask"], batch_size=5)
        C.close(plain, fx[f"{pre}_news_plain"], "plain news cache")
        C.close(aug, fx[f"{pre}_news_aug"], "augmented news cache")
        hist = plain[t["history_ids"]]
        user = m.user_encoder.encode(hist, t["history_mask"])                                     # dense rows
        C.close(user, fx[f"{pre}_user"], "user representations")
    dev = C.dev_set(name, _dev())
    grouped, ranks, _ = nrms.compute_scores(m, dev, batch_size=7, grouped=True)
    per_row, ranks_rows, _ = nrms.compute_scores(m, dev, batch_size=7, grouped=False)
    C.close(grouped, fx[f"{pre}_scores"], "scores")
    assert torch.equal(grouped, per_row), "one user per impression and one per row give the same scores"
    assert np.array_equal(ranks, fx[f"{pre}_ranks"]) and np.array_equal(ranks_rows, ranks)


@pytest.mark.parametrize("pre", list(C.MODELS))
@pytest.mark.parametrize("name", ["nrms_train_tiny.npz", "nrms_train_default.npz"])
def test_hip_training_step_matches_reference_autograd(name, pre):
    """Loss and every gradient (the word table's rows included) of one step of the whole Model, dropout 0, vs the reference's autograd."""
    fx = C.case(name)[0]
    m = C.model(name, pre, _dev()).train()
    logits, loss = C.training_step(m, C.tensors(name, _dev()))
    torch.cuda.synchronize()
    assert _uses_fused(logits) and (pre == "nrms" or _uses_fused(logits, "NewsCtxFused"))
    C.check_training_step(fx, pre, m, logits, loss)


def test_sa_gate_kernels_match_the_stock_gate():
    """The equivalence tests/test_nrms_cpu.py holds on the oracle, on the kernels: inference entry, training pair and its gradients."""
    m = C.model("nrms_default.npz", "sa", _dev()).eval()
    ne = m.news_encoder
    rng = np.random.default_rng(5)
    T, A, d = 37, ne.augmented_news_num, ne.news_embedding_dim
    orig = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32)).to(_dev())
    aug = torch.from_numpy(rng.standard_normal((T, A, d)).astype(np.float32)).to(_dev())
    with torch.no_grad():
        ref = C.model("nrms_default.npz", "sa").eval().news_encoder.sa_gate_stock(orig.cpu(), aug.cpu())
        C.close(ne.sa_gate(orig, aug), ref.numpy(), "gate, inference")
    o2, a2 = orig.clone().requires_grad_(True), aug.clone().requires_grad_(True)
    out = ne.sa_gate(o2, a2)
    assert _uses_fused(out, "NewsCtxFused")
    C.close(out, ref.numpy(), "gate, training pair")
    R = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32))
    (out * R.to(_dev())).sum().backward()
    cpu = C.model("nrms_default.npz", "sa").train().news_encoder
    o3, a3 = orig.cpu().requires_grad_(True), aug.cpu().requires_grad_(True)
    (cpu.sa_gate_stock(o3, a3) * R).sum().backward()
    C.close(o2.grad, o3.grad.numpy(), "d orig", rtol=2e-4)
    C.close(a2.grad, a3.grad.numpy(), "d aug", rtol=2e-4)
    for k in ("SA_attention.K.weight", "SA_attention.Q.weight", "SA_attention.Q.bias", "SA_transformation.weight", "SA_transformation.bias"):
        C.close(dict(ne.named_parameters())[k].grad, dict(cpu.named_parameters())[k].grad.numpy(), "d " + k, rtol=2e-4)


# ---- the attention stage alone -------------------------------------------------------------------------------------------------
MASKS = ("live", "prefix", "holes", "one", "none", "mixed")


def make_mask(kind, T, L, rng):
    m = np.ones((T, L), dtype=np.uint8)
    for t in range(T):
        k = MASKS[t % 5] if kind == "mixed" else kind
        if k == "prefix":
            m[t, int(rng.integers(1, L + 1)):] = 0
        elif k == "holes":
            m[t] = rng.integers(0, 2, size=L)
            m[t, int(rng.integers(0, L))] = 1
        elif k == "one":
            m[t] = 0
            m[t, int(rng.integers(0, L))] = 1
        elif k == "none":
            m[t] = 0
    return m


def attention_fp64(qkv, mask, T, L, heads, dk):
    """Appendix-B layers.py:84-94 in fp64 on [T L, 3 hd] rows: scores / sqrt(d_k), -1e9 over masked keys, softmax, alpha V."""
    hd = heads * dk
    q, k, v = (qkv[:, i * hd:(i + 1) * hd].reshape(T, L, heads, dk).transpose(1, 2) for i in range(3))
    a = q @ k.transpose(2, 3) / math.sqrt(float(dk))
    a = a.masked_fill(mask.view(T, 1, 1, L) == 0, -1e9)
    return (torch.softmax(a, dim=3) @ v).transpose(1, 2).reshape(T * L, hd)


def attention_hip(qkv, mask, T, L, heads, dk, p=0.0, seed=0):
    from digat_amd import _lib
    h = torch.full((T * L, heads * dk), float("nan"), dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.lib().digat_mhsa_attention_fwd(qkv.data_ptr(), mask.data_ptr(), h.data_ptr(), p, seed, T, L, heads, dk, _lib.stream_ptr()),
               "digat_mhsa_attention_fwd")
    return h


def attention_bwd_hip(qkv, mask, dh, T, L, heads, dk, p=0.0, seed=0):
    from digat_amd import _lib
    dqkv = torch.full_like(qkv, float("nan"))
    _lib.check(_lib.lib().digat_mhsa_attention_bwd(qkv.data_ptr(), mask.data_ptr(), dh.data_ptr(), dqkv.data_ptr(), p, seed, T, L, heads, dk,
                                                   _lib.stream_ptr()), "digat_mhsa_attention_bwd")
    return dqkv


# d_k: 4 and 32 are the ends of the matrix-core kernels, 20 the default, 25 no multiple of 4, 40 the plain kernel; heads: fewer and more
# than the waves of a workgroup; T: one workgroup, a few, more than one wave of workgroups; L: one position, one tile, one more, two
# tiles (the 2 x 2 kernel's limit), one more (the 4 x 4 kernel), the user encoder's 50, the limit.
@pytest.mark.parametrize("L", [1, 16, 17, 32, 33, 50, 64])
def test_attention_forward_sweep_against_fp64(L):
    rng = np.random.default_rng(100 + L)
    for dk in (4, 20, 25, 32, 40):
        for heads in (1, 5, 20):
            for T in (1, 3, 130):
                qkv = torch.from_numpy(rng.standard_normal((T * L, 3 * heads * dk)).astype(np.float32)).to(_dev())
                want_by_mask = {}
                for kind in MASKS:
                    mask = torch.from_numpy(make_mask(kind, T, L, rng)).to(_dev())
                    got = attention_hip(qkv, mask, T, L, heads, dk)
                    want = attention_fp64(qkv.double(), mask, T, L, heads, dk)
                    C.close(got, want.cpu().numpy(), f"attention L={L} dk={dk} heads={heads} T={T} mask={kind}")
                    want_by_mask[kind] = want
                # all keys masked: uniform over all L positions, padding included = the mean of V
                v = qkv.double()[:, 2 * heads * dk:].reshape(T, L, -1).mean(dim=1, keepdim=True).expand(T, L, -1).reshape(T * L, -1)
                assert torch.allclose(want_by_mask["none"], v, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("L", [1, 16, 17, 32, 33, 50, 64])
def test_attention_backward_sweep_against_fp64_autograd(L):
    rng = np.random.default_rng(200 + L)
    for dk in (4, 20, 25, 32, 40):
        for heads in (1, 5, 20):
            for T in (1, 3, 130):
                qkv = torch.from_numpy(rng.standard_normal((T * L, 3 * heads * dk)).astype(np.float32)).to(_dev())
                dh = torch.from_numpy(rng.standard_normal((T * L, heads * dk)).astype(np.float32)).to(_dev())
                for kind in MASKS:
                    mask = torch.from_numpy(make_mask(kind, T, L, rng)).to(_dev())
                    got = attention_bwd_hip(qkv, mask, dh, T, L, heads, dk)
                    x = qkv.double().requires_grad_(True)
                    (attention_fp64(x, mask, T, L, heads, dk) * dh.double()).sum().backward()
                    what = f"attention backward L={L} dk={dk} heads={heads} T={T} mask={kind}"
                    hd = heads * dk
                    for i, part in enumerate(("dQ", "dK", "dV")):
                        C.close(got[:, i * hd:(i + 1) * hd], x.grad[:, i * hd:(i + 1) * hd].cpu().numpy(), f"{part} {what}", rtol=2e-4, atol=2e-6)
                    if kind == "none":        # no gradient reaches a masked score, although alpha is uniform there
                        assert float(got[:, :2 * hd].abs().max()) == 0.0, what
                        assert float(got[:, 2 * hd:].abs().max()) > 0.0, what


def test_attention_dropout_site_draws_the_counter_hash():
    """Site 2 alone: the forward's output is the undropped output under the oracle's keep bits, the backward's dO likewise."""
    from oracle import digat_oracle as O
    rng = np.random.default_rng(9)
    T, L, heads, dk, p, seed = 5, 50, 20, 20, 0.2, 12345
    qkv = torch.from_numpy(rng.standard_normal((T * L, 3 * heads * dk)).astype(np.float32)).to(_dev())
    dh = torch.from_numpy(rng.standard_normal((T * L, heads * dk)).astype(np.float32)).to(_dev())
    mask = torch.from_numpy(make_mask("mixed", T, L, rng)).to(_dev())
    plain = attention_hip(qkv, mask, T, L, heads, dk)
    dropped = attention_hip(qkv, mask, T, L, heads, dk, p, seed)
    assert torch.equal(dropped.cpu(), O.hash_dropout(plain.cpu(), p, seed))
    assert torch.equal(attention_bwd_hip(qkv, mask, dh, T, L, heads, dk, p, seed),
                       attention_bwd_hip(qkv, mask, O.hash_dropout(dh.cpu(), p, seed).to(_dev()), T, L, heads, dk))


# ---- the whole encoder through the C ABI -----------------------------------------------------------------------------------------
class Raw:
    """digat_mhsa_* called directly: weights of a user-encoder-shaped block (or any), buffers filled as the test asks."""

    def __init__(self, in_dim, heads, dk, att, seed, flags=0, qk_gain=1.0):
        from digat_amd import _lib, synthetic
        self.lib, self.L = _lib, _lib.lib()
        st = synthetic.make_nrms_state(8, in_dim, heads, dk, att, sa=False, seed=seed)
        names = ("multiheadAttention.W_Q.weight", "multiheadAttention.W_Q.bias", "multiheadAttention.W_K.weight", "multiheadAttention.W_V.weight",
                 "multiheadAttention.W_V.bias", "attention.affine1.weight", "attention.affine1.bias", "attention.affine2.weight")
        self.w = [torch.from_numpy(st["news_encoder." + n]).to(_dev()).contiguous() for n in names]
        self.w[0], self.w[2] = self.w[0] * qk_gain, self.w[2] * qk_gain           # a peaked attention: well-conditioned pooling gradients
        self.dims = (in_dim, heads, dk, att)
        self.flags = flags

    def params(self, table):
        P = self.lib.MhsaParams(in_dim=self.dims[0], head_num=self.dims[1], head_dim=self.dims[2], attention_dim=self.dims[3], flags=self.flags)
        for k, w in zip(("W_Q", "b_Q", "W_K", "W_V", "b_V", "A1", "b1", "a2"), self.w):
            setattr(P, k, w.data_ptr())
        P.table = table.data_ptr()
        return P

    def split(self, P):
        in_dim, heads, dk, att = self.dims
        qkv = self.lib.split_buffer(self.L.digat_msa_split_bytes(in_dim, heads, dk), _dev())
        self.lib.check(self.L.digat_split_msa_weights(self.w[0].data_ptr(), self.w[2].data_ptr(), self.w[3].data_ptr(), in_dim, heads * dk,
                                                      qkv.data_ptr(), self.lib.stream_ptr()), "split")
        a1 = self.lib.split_buffer(self.L.digat_split_weights_bytes(att, heads * dk), _dev())
        self.lib.check(self.L.digat_split_weights(self.w[5].data_ptr(), att, heads * dk, a1.data_ptr(), self.lib.GEMM_BF16X6, self.lib.stream_ptr()), "split")
        P.qkv_wsplit, P.a1_wsplit = qkv.data_ptr(), a1.data_ptr()
        return qkv, a1

    def buf(self, nbytes, fill):
        b = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=_dev())
        if fill == "nan":
            b.view(torch.float32).fill_(float("nan"))
        else:
            b.zero_()
        return b

    def fwd(self, table, ids, mask, T, Ls, fill="zero", images=False):
        P = self.params(table)
        keep = self.split(P) if images else None
        nb = self.L.digat_mhsa_workspace_bytes(T, Ls, *self.dims)
        ws = self.buf(nb, fill)
        out = torch.full((max(T, 1), self.dims[1] * self.dims[2]), float("nan"), dtype=torch.float32, device=_dev())      # T = 0: still a pointer
        self.lib.check(self.L.digat_mhsa_fwd(P, self.lib.ptr(ids), mask.data_ptr(), out.data_ptr(), T, Ls, ws.data_ptr(), nb, self.lib.stream_ptr()),
                       "digat_mhsa_fwd")
        torch.cuda.synchronize()
        del keep
        return out[:T]

    def step(self, table, ids, mask, dout, T, Ls, p_in=0.0, p_ctx=0.0, seed=0, fill="zero"):
        """forward + backward -> (out, row_grad [T Ls, in_dim], [dW_Q, db_Q, dW_K, dW_V, db_V, dA1, db1, da2])"""
        in_dim, heads, dk, att = self.dims
        hd = heads * dk
        P = self.params(table)
        nsave, nws = self.L.digat_mhsa_train_save_bytes(T, Ls, *self.dims), self.L.digat_mhsa_train_workspace_bytes(T, Ls, *self.dims)
        save, ws = self.buf(nsave, fill), self.buf(nws, fill)
        f = dict(dtype=torch.float32, device=_dev())
        out = torch.full((max(T, 1), hd), float("nan"), **f)            # T = 0: an empty tensor's pointer is NULL, which the entries refuse
        S = self.lib.stream_ptr()
        self.lib.check(self.L.digat_mhsa_fwd_train(P, self.lib.ptr(ids), mask.data_ptr(), out.data_ptr(), p_in, p_ctx, seed, T, Ls, save.data_ptr(), nsave,
                                                   ws.data_ptr(), nws, S), "digat_mhsa_fwd_train")
        if fill == "nan":
            ws.view(torch.float32).fill_(float("nan"))
        ld = int(self.L.digat_msa_row_grad_ld(T, Ls, in_dim))
        row_grad = torch.full((max(T * Ls, 1), ld), float("nan"), **f)
        g = [torch.full(s, float("nan"), **f) for s in ((hd, in_dim), (hd,), (hd, in_dim), (hd, in_dim), (hd,), (att, hd), (att,), (att,))]
        self.lib.check(self.L.digat_mhsa_bwd(P, self.lib.ptr(ids), mask.data_ptr(), dout.data_ptr(), p_in, p_ctx, seed, save.data_ptr(), nsave,
                                             row_grad.data_ptr(), ld, *(t.data_ptr() for t in g), T, Ls, ws.data_ptr(), nws, S), "digat_mhsa_bwd")
        torch.cuda.synchronize()
        return out[:T], row_grad[:T * Ls, :in_dim], g


@pytest.mark.parametrize("T,Ls,in_dim,heads,dk,att,images", [(3, 50, 64, 2, 40, 12, False), (9, 33, 100, 5, 16, 24, True), (170, 64, 64, 20, 20, 200, True)])
def test_gather_input_and_dense_input_give_the_same_bits(T, Ls, in_dim, heads, dk, att, images):
    """table[ids] read through the projection's row list (170 x 64 rows: the strip-mined kernel, 128-row tiles either way), or gathered
    first (small shapes), against the same rows handed over densely; inference and the training pair."""
    rng = np.random.default_rng(T)
    r = Raw(in_dim, heads, dk, att, seed=T)
    V = 23
    table = torch.from_numpy(rng.standard_normal((V, in_dim)).astype(np.float32)).to(_dev())
    ids = torch.from_numpy(rng.integers(0, V, size=(T, Ls)).astype(np.int32)).to(_dev())
    mask = torch.from_numpy(make_mask("mixed", T, Ls, rng)).to(_dev())
    dense = table[ids.long().flatten()].contiguous()
    a, b = r.fwd(table, ids, mask, T, Ls, images=images), r.fwd(dense, None, mask, T, Ls, images=images)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    dout = torch.from_numpy(rng.standard_normal((T, heads * dk)).astype(np.float32)).to(_dev())
    (o1, rg1, g1), (o2, rg2, g2) = r.step(table, ids, mask, dout, T, Ls), r.step(dense, None, mask, dout, T, Ls)
    assert torch.equal(o1, o2) and torch.equal(rg1, rg2) and all(torch.equal(x, y) for x, y in zip(g1, g2))


@pytest.mark.parametrize("T,Ls,in_dim,heads,dk,att,flags", [(7, 50, 80, 20, 20, 200, 1), (70, 32, 300, 20, 20, 200, 0), (4, 9, 16, 2, 40, 8, 0)])
def test_nan_filled_workspace_and_save_change_no_bit(T, Ls, in_dim, heads, dk, att, flags):
    rng = np.random.default_rng(T + 1)
    r = Raw(in_dim, heads, dk, att, seed=T, flags=flags)
    x = torch.from_numpy(rng.standard_normal((T * Ls, in_dim)).astype(np.float32)).to(_dev())
    mask = torch.from_numpy(make_mask("mixed", T, Ls, rng)).to(_dev())
    dout = torch.from_numpy(rng.standard_normal((T, heads * dk)).astype(np.float32)).to(_dev())
    assert torch.equal(r.fwd(x, None, mask, T, Ls, "zero"), r.fwd(x, None, mask, T, Ls, "nan"))
    for p in (0.0, 0.2):
        (o1, rg1, g1), (o2, rg2, g2) = r.step(x, None, mask, dout, T, Ls, p, p, 7, "zero"), r.step(x, None, mask, dout, T, Ls, p, p, 7, "nan")
        assert torch.isfinite(o1).all() and torch.isfinite(rg1).all() and all(torch.isfinite(t).all() for t in g1)
        assert torch.equal(o1, o2) and torch.equal(rg1, rg2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def encoder_fp64(x, mask, w, T, Ls, heads, dk, unmasked_pooling, p_in, p_ctx, seed):
    """The whole encoder in fp64 on dense rows x [T Ls, in_dim] (Appendix-B layers.py:79-122), dropout under the oracle's hash masks."""
    from oracle import digat_oracle as O
    WQ, bQ, WK, WV, bV, A1, b1, a2 = (t.double() for t in w)
    xd = O.hash_dropout(x.cpu(), p_in, seed).to(x.device) if p_in > 0 else x
    qkv = torch.cat([xd @ WQ.T + bQ, xd @ WK.T, xd @ WV.T + bV], dim=1)
    c = attention_fp64(qkv, mask, T, Ls, heads, dk)
    hd = heads * dk
    q, k = (qkv.detach()[:, i * hd:(i + 1) * hd].reshape(T, Ls, heads, dk).transpose(1, 2) for i in range(2))
    encoder_fp64.score_max = float((q @ k.transpose(2, 3)).abs().max()) / math.sqrt(float(dk))       # the largest |score| of the case
    if p_ctx > 0:
        c = O.hash_dropout(c.cpu(), p_ctx, seed + 1).to(x.device)
    c = c.view(T, Ls, heads * dk)
    a = (torch.tanh(c @ A1.T + b1) @ a2.T).squeeze(2)
    if not unmasked_pooling:
        a = a.masked_fill(mask == 0, -1e9)
    return (torch.softmax(a, dim=1).unsqueeze(1) @ c).squeeze(1)


# dense rows through digat_mhsa_fwd_train / digat_mhsa_bwd: the user encoder's call (pooling unmasked) and the masked one, below and
# above the 2 048 rows where the projections take the matrix-core path, without and with both dropouts on the dense input
@pytest.mark.parametrize("T,Ls,in_dim,heads,dk,att,flags,p", [(7, 50, 80, 20, 20, 200, 1, 0.0), (45, 50, 400, 20, 20, 200, 1, 0.0),
                                                           (45, 50, 400, 20, 20, 200, 1, 0.2), (9, 33, 64, 5, 16, 24, 1, 0.2),
                                                           (70, 32, 300, 20, 20, 200, 0, 0.2)])
def test_training_pair_on_dense_rows_against_fp64_autograd(T, Ls, in_dim, heads, dk, att, flags, p):
    """Output, row_grad (= dX) and all eight weight gradients against fp64 autograd at the training tolerance.  Rows of unit variance
    and a gain on W_Q, W_K make the attention peaked, so the pooling sees rows that differ and its gradients are of ordinary size."""
    rng = np.random.default_rng(T + Ls)
    r = Raw(in_dim, heads, dk, att, seed=T, flags=flags, qk_gain=4.0)
    x = torch.from_numpy(rng.standard_normal((T * Ls, in_dim)).astype(np.float32)).to(_dev())
    mask = torch.from_numpy(make_mask("mixed", T, Ls, rng)).to(_dev())
    dout = torch.from_numpy(rng.standard_normal((T, heads * dk)).astype(np.float32)).to(_dev())
    seed = 4321
    out, row_grad, grads = r.step(x, None, mask, dout, T, Ls, p, p, seed)
    x64 = x.double().requires_grad_(True)
    w64 = [t.double().requires_grad_(True) for t in r.w]
    want = encoder_fp64(x64, mask, w64, T, Ls, heads, dk, bool(flags & 1), p, p, seed)
    (want * dout.double()).sum().backward()
    # Forward bound, from the number format: a score S carries an absolute rounding error of a few eps32 |S| (rows, projection, dot
    # product, scale: 8 roundings allowed), which the softmax turns into the same RELATIVE error of a weight; an output element is a
    # weighted sum of rows of the tensor's scale, so its absolute error is that fraction of the scale.  With the gain on W_Q, W_K the
    # scores reach a few tens (measured on the fp64 reference, not on the code under test).  1e-5 of the scale for everything else.
    want_np = want.detach().cpu().numpy()
    bound = (1e-5 + 8 * 2.0 ** -24 * encoder_fp64.score_max) * float(np.abs(want_np).max())
    err = float(np.abs(out.cpu().numpy() - want_np).max())
    assert np.isfinite(out.cpu().numpy()).all() and err <= bound, f"encoder output: max|diff| {err:.3e}, bound {bound:.3e} (|S| <= {encoder_fp64.score_max:.1f})"
    C.close(row_grad, x64.grad.cpu().numpy(), "row_grad", rtol=2e-4, atol=0.0)
    for name, got, ref in zip(("dW_Q", "db_Q", "dW_K", "dW_V", "db_V", "dA1", "db1", "da2"), grads, w64):
        assert float(ref.grad.abs().max()) > 1e-3, name + ": the case is meant to be well conditioned"
        C.close(got, ref.grad.reshape(got.shape).cpu().numpy(), name, rtol=2e-4, atol=0.0)


def test_no_sequence_forward_and_backward():
    r = Raw(64, 5, 16, 24, seed=1)
    x = torch.zeros((1, 64), dtype=torch.float32, device=_dev())
    mask = torch.zeros((1, 50), dtype=torch.uint8, device=_dev())
    assert r.fwd(x, None, mask, 0, 50).shape == (0, 80)
    out, rg, g = r.step(x, None, mask, torch.zeros((1, 80), device=_dev()), 0, 50)
    assert out.shape == (0, 80) and rg.shape[0] == 0 and all(float(t.abs().max()) == 0.0 for t in g)
    m = C.model("nrms_tiny.npz", "sa", _dev()).train()
    t = C.tensors("nrms_tiny.npz", _dev())
    empty = m.news_encoder(t["title_text"][:0].unsqueeze(0), t["title_mask"][:0].unsqueeze(0))
    assert empty.shape == (1, 0, m.news_embedding_dim)


# ---- dropout -------------------------------------------------------------------------------------------------------------------
def _titles(name):
    """The augmented titles of a fixture as one batch [N A, Lw] (120 x 32 rows at the default shape: the matrix-core GEMM path)."""
    t = C.tensors(name)
    Lw = t["augmented_title_text"].shape[-1]
    return t["augmented_title_text"].reshape(-1, Lw), t["augmented_title_mask"].reshape(-1, Lw)


@pytest.mark.parametrize("name", ["nrms_train_tiny.npz", "nrms_train_default.npz"])
def test_training_with_both_dropouts_live_matches_stock_under_the_same_masks(name):
    """p = 0.2 at both sites: site 1's keep bits are the counter hash of `seed` over the [T Lw, dm] embedded tokens, site 2's of
    `seed + 1` over the [T Lw, hd] attention output.  The stock encoder on the CPU with its dropout replaced by the oracle's restatement
    of that hash, and autograd: output and every gradient."""
    from oracle import digat_oracle as O
    text, mask = _titles(name)
    enc = C.model(name, "nrms", _dev(), dropout=0.2).train().news_encoder
    ref = C.model(name, "nrms", dropout=0.2).train().news_encoder
    R = torch.from_numpy(np.random.default_rng(4).standard_normal((text.shape[0], enc.news_embedding_dim)).astype(np.float32))
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())           # what MhsaFused.forward will draw
    torch.manual_seed(77)
    out = enc.encode_titles(text.to(_dev()), mask.to(_dev()))
    assert _uses_fused(out)
    (out * R.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    site = iter((seed, seed + 1))
    del ref.dropout
    ref.dropout = lambda x: O.hash_dropout(x.contiguous(), 0.2, next(site))
    want = ref._titles_stock(text, mask)
    (want * R).sum().backward()
    C.close(out, want.detach().numpy(), "news representation under dropout")
    ref.dropout = lambda x: x
    assert float((want.detach() - ref._titles_stock(text, mask).detach()).abs().max()) > 1e-3      # the dropout is live
    grads = dict(ref.named_parameters())
    for k, q in enc.named_parameters():
        C.close(q.grad, grads[k].grad.numpy(), "grad " + k + " under dropout", rtol=2e-4)


def test_training_with_dropout_is_reproducible():
    text, mask = _titles("nrms_train_default.npz")

    def once():
        torch.manual_seed(11)
        enc = C.model("nrms_train_default.npz", "nrms", _dev(), dropout=0.2).train().news_encoder
        out = enc.encode_titles(text.to(_dev()), mask.to(_dev()))
        out.square().sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), [p.grad.clone() for p in enc.parameters()]
    o1, g1 = once()
    o2, g2 = once()
    assert torch.isfinite(o1).all() and all(torch.isfinite(g).all() for g in g1)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
