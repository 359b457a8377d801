"""CPU suite for the NRMS / NRMS-SA baselines (digat_amd/nrms.py; the reference's Appendix-B): the stock PyTorch path against the
vectors minted from the reference's own modules (tools/make_golden_nrms.py), the state_dict keys, the identity the SA gate's HIP path
rests on (the gate is the news-graph context on [orig ; aug] with node 0 masked out), and the digat_mhsa_* C ABI without a device."""
import ctypes

import numpy as np
import pytest
import torch

import nrms_common as C

INFERENCE = ["nrms_tiny.npz", "nrms_default.npz"]
TRAIN = ["nrms_train_tiny.npz", "nrms_train_default.npz"]


@pytest.mark.parametrize("pre", list(C.MODELS))
@pytest.mark.parametrize("name", INFERENCE)
def test_stock_forward_matches_reference_vectors(name, pre):
    from digat_amd import nrms
    fx, cfg, inp, _ = C.case(name)
    m = C.model(name, pre).eval()
    t = C.tensors(name)
    ne, ue = m.news_encoder, m.user_encoder
    K = inp["candidate_ids"].shape[1]
    with torch.no_grad():
        w = ne.word_embedding(t["title_text"])
        c = ne.multiheadAttention(w, w, w, t["title_mask"])
        C.close(c[1:3], fx[f"{pre}_c_head"], "attention output of the title with holes and the all-padding title")
        assert torch.allclose(c[2], c[2].mean(dim=0, keepdim=True).expand_as(c[2]), rtol=1e-5, atol=1e-6), "all-masked keys attend uniformly"
        plain, aug = nrms.news_caches(m, t["title_text"], t["title_mask"], t["augmented_title_text"], t["augmented_title_mask"], batch_size=5)
        C.close(plain, fx[f"{pre}_news_plain"], "plain news cache")
        C.close(aug, fx[f"{pre}_news_aug"], "augmented news cache")
        if pre == "sa":
            N, A, Lw = t["augmented_title_text"].shape
            augt = ne._titles_stock(t["augmented_title_text"].reshape(N * A, Lw), t["augmented_title_mask"].reshape(N * A, Lw)).view(N, A, -1)
            C.close(augt, fx["sa_aug_titles"], "augmented titles")
            g = nrms._stock_sdpa(ne.SA_attention, augt, plain)
            C.close(g, fx["sa_g"], "attention of the original over its augmented titles")
            C.close(ne.SA_transformation(torch.cat([plain, g], dim=1)), fx["sa_gate_pre"], "gate before the sigmoid")
        hist = plain[t["history_ids"]]
        h = ue.multiheadAttention(hist, hist, hist, t["history_mask"])
        C.close(h[1:2], fx[f"{pre}_user_h_head"], "user attention output of the empty history")
        C.close(ue.encode(hist, t["history_mask"]), fx[f"{pre}_user"], "user representations")
        for grouped in (True, False):
            scores, ranks, metrics = nrms.compute_scores(m, C.dev_set(name), batch_size=7, grouped=grouped)
            C.close(scores, fx[f"{pre}_scores"], "scores")
            assert np.array_equal(ranks, fx[f"{pre}_ranks"]) and metrics is None
    assert fx[f"{pre}_scores"].shape == (4 * K,)


@pytest.mark.parametrize("pre", list(C.MODELS))
@pytest.mark.parametrize("name", TRAIN)
def test_stock_training_step_matches_reference_autograd(name, pre):
    fx = C.case(name)[0]
    m = C.model(name, pre).train()
    logits, loss = C.training_step(m, C.tensors(name))
    C.check_training_step(fx, pre, m, logits, loss)
    # the fixture is well conditioned: the reference's own fp32 run has every gradient to half the tolerance or better
    errs = C.reference_fp32_errors(fx, pre)
    assert set(errs) == {k for k, _ in m.named_parameters()} and max(errs.values()) <= 1e-4, errs


@pytest.mark.parametrize("pre", list(C.MODELS))
def test_state_dict_keys_are_the_references(pre):
    fx = C.case("nrms_tiny.npz")[0]
    m = C.model("nrms_tiny.npz", pre)
    assert sorted(m.state_dict().keys()) == [str(k) for k in fx[f"{pre}_state_keys"]]
    m.initialize()
    assert float(m.news_encoder.multiheadAttention.W_Q.bias.detach().abs().sum()) == 0.0


def test_sa_gate_is_the_news_graph_context_with_node_0_masked_out():
    """Appendix-B newsEncoders.py:100-102 = graphEncoders.py:109-114 on X = [orig ; aug], node mask [0, 1, ..., 1]: the query is
    node 0, the attention runs over the augmented titles only, the gate mixes node 0 with the attended context.  The HIP path of the
    gate is digat_news_ctx_* on exactly this input (tests/test_hip_nrms.py holds the kernels to it)."""
    from oracle import digat_oracle
    m = C.model("nrms_tiny.npz", "sa").eval()
    ne = m.news_encoder
    rng = np.random.default_rng(3)
    T, A, d = 9, ne.augmented_news_num, ne.news_embedding_dim
    orig = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32))
    aug = torch.from_numpy(rng.standard_normal((T, A, d)).astype(np.float32))
    p = {"candidate_attention.K.weight": ne.SA_attention.K.weight, "candidate_attention.Q.weight": ne.SA_attention.Q.weight,
         "candidate_attention.Q.bias": ne.SA_attention.Q.bias, "news_graph_W.weight": ne.SA_transformation.weight,
         "news_graph_W.bias": ne.SA_transformation.bias}
    mask = torch.ones((T, 1 + A), dtype=torch.int64)
    mask[:, 0] = 0
    with torch.no_grad():
        want = ne.sa_gate_stock(orig, aug)
        got = digat_oracle.news_graph_context(p, torch.cat([orig.unsqueeze(1), aug], dim=1), mask)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-6)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------
# (T, L, in_dim, heads, dk, att) -> (workspace, train_save, train_workspace).  The byte counts are ABI.  The encoder shares stages A
# and C with digat_msa_*: its buffers are that family's plus T * L bytes of an all-ones pooling mask (rounded up to 256) in both
# workspaces; the save buffer is the same.
MHSA_SIZES = {
    (6400, 32, 300, 20, 20, 200): (1753292800, 1815347200, 1612420352),
    (4096, 50, 400, 20, 20, 200): (1835212800, 1917747200, 1602602496),
    (300, 32, 300, 20, 20, 200): (82185728, 85094400, 133032704),
    (140, 20, 64, 5, 16, 100): (6095616, 6283264, 6553856),
    (3, 50, 64, 2, 40, 12): (279040, 289280, 892160),
    (1, 1, 16, 1, 4, 4): (1536, 1792, 65280),
    (0, 16, 32, 2, 8, 12): (0, 0, 89600),
}
SYMBOLS = ("digat_mhsa_workspace_bytes", "digat_mhsa_fwd", "digat_mhsa_train_save_bytes", "digat_mhsa_train_workspace_bytes",
           "digat_mhsa_fwd_train", "digat_mhsa_bwd", "digat_mhsa_attention_fwd", "digat_mhsa_attention_bwd")


def _lib_built():
    from digat_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


@pytest.mark.parametrize("shape", list(MHSA_SIZES))
def test_mhsa_size_queries_are_pinned(shape):
    _, L = _lib_built()
    got = (L.digat_mhsa_workspace_bytes(*shape), L.digat_mhsa_train_save_bytes(*shape), L.digat_mhsa_train_workspace_bytes(*shape))
    assert got == MHSA_SIZES[shape], shape
    ones = (shape[0] * shape[1] + 255) // 256 * 256
    assert got == (L.digat_msa_workspace_bytes(*shape) + ones, L.digat_msa_train_save_bytes(*shape), L.digat_msa_train_workspace_bytes(*shape) + ones)


OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
BIG = 1 << 30


def mhsa_status_cases(_lib, L):
    """[(what, returned status)] of the digat_mhsa_* entries on calls that end before any launch (tests/test_news_abi_cpu.py's manner)."""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)                                      # a non-null HOST address: every check below fails before it is read

    def params(dm=300, heads=20, dk=20, att=200, table=a):
        P = _lib.MhsaParams(in_dim=dm, head_num=heads, head_dim=dk, attention_dim=att)
        for k in ("W_Q", "b_Q", "W_K", "W_V", "b_V", "A1", "b1", "a2"):
            setattr(P, k, a)
        P.table = table
        return P

    def fwd(P="default", ids=a, mask=a, T=4, Ls=32, ws=a, nws=BIG):
        return L.digat_mhsa_fwd(params() if P == "default" else P, ids, mask, a, T, Ls, ws, nws, None)

    def fwd_train(P="default", out=a, p_in=0.2, p_ctx=0.2, T=4, Ls=32, nsave=BIG, nws=BIG):
        return L.digat_mhsa_fwd_train(params() if P == "default" else P, a, a, out, p_in, p_ctx, 1, T, Ls, a, nsave, a, nws, None)

    def bwd(P="default", dout=a, T=4, Ls=32, nsave=BIG, ld=300, da2=a, nws=BIG, p_ctx=0.2):
        return L.digat_mhsa_bwd(params() if P == "default" else P, a, a, dout, 0.2, p_ctx, 1, a, nsave, a, ld, a, a, a, a, a, a, a, da2, T, Ls, a,
                                nws, None)

    def attn(fn, qkv=a, p=0.0, T=4, Ls=32, heads=20, dk=20):
        if fn == "fwd":
            return L.digat_mhsa_attention_fwd(qkv, a, a, p, 1, T, Ls, heads, dk, None)
        return L.digat_mhsa_attention_bwd(qkv, a, a, a, p, 1, T, Ls, heads, dk, None)

    cases = [("fwd NULL params", fwd(P=None)), ("fwd NULL table", fwd(P=params(table=None))), ("fwd NULL mask", fwd(mask=None)),
             ("fwd NULL workspace", fwd(ws=None)), ("fwd T < 0", fwd(T=-1)), ("fwd L = 0", fwd(Ls=0)), ("fwd dm = 30", fwd(P=params(dm=30))),
             ("fwd dk = 129", fwd(P=params(dk=129))), ("fwd att = 0", fwd(P=params(att=0))), ("fwd L = 65", fwd(Ls=65)),
             ("fwd hd = 6", fwd(P=params(heads=2, dk=3))), ("fwd att = 6, 16-byte workspace", fwd(P=params(att=6), nws=16)),
             ("fwd L = 50, dk = 40, dense rows, 16-byte workspace", fwd(P=params(dk=40), ids=None, Ls=50, nws=16)),
             ("fwd 16-byte workspace", fwd(nws=16)), ("fwd T = 0", fwd(T=0, nws=0))]
    for name, fn in (("fwd_train", fwd_train), ("bwd", bwd)):
        cases += [(name + " NULL params", fn(P=None)), (name + " NULL table", fn(P=params(table=None))), (name + " T < 0", fn(T=-1)),
                  (name + " L = 0", fn(Ls=0)), (name + " p_ctx = 1", fn(p_ctx=1.0)), (name + " dm = 30", fn(P=params(dm=30))),
                  (name + " dk = 129", fn(P=params(dk=129))), (name + " att = 0", fn(P=params(att=0))), (name + " att = 6", fn(P=params(att=6))),
                  (name + " L = 65", fn(Ls=65)), (name + " 16-byte workspace", fn(nws=16)), (name + " 16-byte save", fn(nsave=16)),
                  (name + " 16-byte save and workspace", fn(nsave=16, nws=16))]
    cases += [("fwd_train NULL out", fwd_train(out=None)), ("fwd_train p_in = 1", fwd_train(p_in=1.0)), ("fwd_train p_in < 0", fwd_train(p_in=-0.1)),
              ("fwd_train p_in = 1, dm = 30", fwd_train(p_in=1.0, P=params(dm=30))), ("fwd_train T = 0", fwd_train(T=0, nsave=0, nws=0)),
              ("fwd_train T = 0, L = 65", fwd_train(T=0, Ls=65)),
              ("bwd NULL dout", bwd(dout=None)), ("bwd NULL da2", bwd(da2=None)), ("bwd ld = 304", bwd(ld=304)),
              ("bwd ld = 320, 16-byte workspace", bwd(ld=320, nws=16)), ("bwd ld = 304, L = 65", bwd(ld=304, Ls=65)),
              ("bwd ld = 304, 16-byte save", bwd(ld=304, nsave=16))]
    for fn in ("fwd", "bwd"):
        cases += [(f"attention {fn} NULL qkv", attn(fn, qkv=None)), (f"attention {fn} T < 0", attn(fn, T=-1)), (f"attention {fn} heads = 0", attn(fn, heads=0)),
                  (f"attention {fn} p = 1", attn(fn, p=1.0)), (f"attention {fn} L = 65", attn(fn, Ls=65)), (f"attention {fn} dk = 129", attn(fn, dk=129)),
                  (f"attention {fn} T = 0", attn(fn, T=0))]
    return cases


# The order of the family (tests/test_news_abi_cpu.py): arguments, then shapes, then the save buffer before the workspace; a bad leading
# dimension of row_grad is an argument error found after the shape; T = 0 returns OK once arguments and shapes have passed.
# digat_mhsa_bwd at T = 0 zero-fills the gradient buffers and is asserted on the GPU.
MHSA_STATUS = {
    "fwd NULL params": ARG, "fwd NULL table": ARG, "fwd NULL mask": ARG, "fwd NULL workspace": ARG, "fwd T < 0": ARG, "fwd L = 0": ARG,
    "fwd dm = 30": SHAPE, "fwd dk = 129": SHAPE, "fwd att = 0": SHAPE, "fwd L = 65": SHAPE, "fwd hd = 6": SHAPE,
    "fwd att = 6, 16-byte workspace": WORKSPACE, "fwd L = 50, dk = 40, dense rows, 16-byte workspace": WORKSPACE, "fwd 16-byte workspace": WORKSPACE,
    "fwd T = 0": OK,
    "fwd_train NULL params": ARG, "fwd_train NULL table": ARG, "fwd_train NULL out": ARG, "fwd_train T < 0": ARG, "fwd_train L = 0": ARG,
    "fwd_train p_in = 1": ARG, "fwd_train p_in < 0": ARG, "fwd_train p_ctx = 1": ARG, "fwd_train p_in = 1, dm = 30": ARG,
    "fwd_train dm = 30": SHAPE, "fwd_train dk = 129": SHAPE, "fwd_train att = 0": SHAPE, "fwd_train att = 6": SHAPE, "fwd_train L = 65": SHAPE,
    "fwd_train 16-byte workspace": WORKSPACE, "fwd_train 16-byte save": WORKSPACE, "fwd_train 16-byte save and workspace": WORKSPACE,
    "fwd_train T = 0": OK, "fwd_train T = 0, L = 65": SHAPE,
    "bwd NULL params": ARG, "bwd NULL table": ARG, "bwd NULL dout": ARG, "bwd NULL da2": ARG, "bwd T < 0": ARG, "bwd L = 0": ARG, "bwd p_ctx = 1": ARG,
    "bwd dm = 30": SHAPE, "bwd dk = 129": SHAPE, "bwd att = 0": SHAPE, "bwd att = 6": SHAPE, "bwd L = 65": SHAPE,
    "bwd ld = 304": ARG, "bwd ld = 304, L = 65": SHAPE, "bwd ld = 304, 16-byte save": ARG,
    "bwd ld = 320, 16-byte workspace": WORKSPACE,
    "bwd 16-byte workspace": WORKSPACE, "bwd 16-byte save": WORKSPACE, "bwd 16-byte save and workspace": WORKSPACE,
}
for _fn in ("fwd", "bwd"):
    MHSA_STATUS.update({f"attention {_fn} NULL qkv": ARG, f"attention {_fn} T < 0": ARG, f"attention {_fn} heads = 0": ARG, f"attention {_fn} p = 1": ARG,
                        f"attention {_fn} L = 65": SHAPE, f"attention {_fn} dk = 129": SHAPE, f"attention {_fn} T = 0": OK})


def test_mhsa_abi_without_a_device():
    _lib, L = _lib_built()
    for n in SYMBOLS:
        assert hasattr(L, n) and n in _lib.EXPORTED, n
    assert ctypes.sizeof(_lib.MhsaParams) == 16 + 11 * 8 + 8
    got = dict(mhsa_status_cases(_lib, L))
    assert got == MHSA_STATUS
    assert L.digat_version() == 4
