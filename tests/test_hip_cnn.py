"""GPU suite for the CNN news encoder on the HIP kernels (csrc/digat_cnn.inc): digat_cnn_fwd, digat_cnn_fwd_train / digat_cnn_bwd
through newsEncoders.CNN, against the vectors minted from the reference's layers.py modules (tests/golden/cnn_*.npz), the stock
PyTorch module on the CPU, and the oracle's hash dropout.  Tolerances: the project's own for this pipeline with another first
stage (tests/test_hip_news.py)."""
import types

import numpy as np
import pytest
import torch

from test_cnn_cpu import INFERENCE, TRAIN, check_training_step, close, cnn_case, cnn_encoder

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _uses_fused(t):
    """Whether ``t`` was produced through the CnnFused autograd function (the HIP training pair)."""
    todo, seen = [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "CnnFused" in type(fn).__name__:
            return True
        todo += [f for f, _ in fn.next_functions]
    return False


def _cpu_clone(enc):
    """A CPU encoder with ``enc``'s configuration and weights."""
    window = enc.conv.conv.kernel_size[0] if enc.conv.cnn_method == "naive" else 3
    ref = cnn_encoder(enc.word_embedding.num_embeddings, enc.word_embedding_dim, enc.news_embedding_dim, enc.attention.affine1.out_features,
                      enc.max_sentence_length, enc.conv.cnn_method, window, dropout=enc.dropout.p)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}, strict=True)
    return ref


def _stock_cpu(enc, text, mask):
    """forward_stock of a CPU copy of ``enc`` (fp32), eval mode."""
    ref = _cpu_clone(enc).eval()
    with torch.no_grad():
        return ref.forward_stock(text.cpu(), mask.cpu())


@pytest.mark.parametrize("name", INFERENCE)
def test_cnn_hip_matches_reference_vectors(name):
    fx, enc, text, mask, _ = cnn_case(name)
    enc = enc.to(_dev())
    tt, tm = text.to(_dev()).unsqueeze(1), mask.to(_dev()).unsqueeze(1)
    direct = enc.encode_hip(tt, tm).squeeze(1)                      # called directly: the stock path cannot satisfy this
    np.testing.assert_allclose(direct.cpu().numpy(), fx["out_news_representation"], rtol=1e-5, atol=2e-6)
    with torch.no_grad():
        assert torch.equal(enc(tt, tm).squeeze(1), direct)           # the module dispatches there under no_grad: the same bits


@pytest.mark.parametrize("T_,method,window", [(300, "naive", 3), (4099, "naive", 3), (300, "group3", 3), (301, "naive", 7)])
def test_cnn_hip_production_batches_match_the_stock_module(T_, method, window):
    """T = 300 x 32 and T = 4 099 (a ragged last tile: T is not a multiple of the four titles of a tile) vs forward_stock on the CPU."""
    from digat_amd import synthetic
    Lw, V, dm, Kc, att = 32, 2000, 300, 396 if method == "group3" else 400, 256
    state = synthetic.make_cnn_state(V, dm, Kc, att, method, window, seed=T_)
    text, mask = synthetic.make_titles(T_, Lw, V, seed=T_ + 1)
    enc = cnn_encoder(V, dm, Kc, att, Lw, method, window, state).to(_dev()).eval()
    tt, tm = torch.from_numpy(text).to(_dev()).unsqueeze(1), torch.from_numpy(mask).to(_dev()).unsqueeze(1)
    with torch.no_grad():
        got = enc(tt, tm)
    np.testing.assert_allclose(got.cpu().numpy(), _stock_cpu(enc, tt, tm).numpy(), rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("T_,Lw,V,dm,Kc,att,method,window", [(140, 20, 300, 64, 48, 100, "naive", 5), (70, 64, 200, 36, 24, 20, "group3", 3),
                                                             (5, 7, 40, 12, 8, 8, "naive", 1), (90, 33, 100, 32, 16, 12, "naive", 3)])
def test_cnn_hip_other_shapes_match_the_stock_module(T_, Lw, V, dm, Kc, att, method, window):
    """Off the fixtures' shapes: 2 800 rows of 20 tokens (six titles per tile, 8 rows of it unused), Lw = 64, a one-tap window on the
    plain kernel, Lw = 33 (three titles per tile)."""
    from digat_amd import synthetic
    state = synthetic.make_cnn_state(V, dm, Kc, att, method, window, seed=T_ + Lw)
    text, mask = synthetic.make_titles(T_, Lw, V, seed=T_ + Lw + 1)
    enc = cnn_encoder(V, dm, Kc, att, Lw, method, window, state).to(_dev()).eval()
    tt, tm = torch.from_numpy(text).to(_dev()), torch.from_numpy(mask).to(_dev())
    got = enc.encode_hip(tt, tm)
    np.testing.assert_allclose(got.cpu().numpy(), _stock_cpu(enc, tt.unsqueeze(0), tm.unsqueeze(0)).squeeze(0).numpy(), rtol=1e-5, atol=2e-6)


def test_cnn_news_cache_in_batches_equals_one_call():
    """util.cache_news_representations (util.py:24-33) needs no change for this encoder: ragged batches vs one call, same bits."""
    from digat_amd import synthetic, util
    T_, Lw, V, dm, Kc, att = 1000, 32, 3000, 300, 400, 256
    state = synthetic.make_cnn_state(V, dm, Kc, att, "naive", 3, seed=71)
    text, mask = synthetic.make_titles(T_, Lw, V, seed=72)
    enc = cnn_encoder(V, dm, Kc, att, Lw, "naive", 3, state).to(_dev()).eval()
    tt, tm = torch.from_numpy(text).to(_dev()), torch.from_numpy(mask).to(_dev())
    a = util.cache_news_representations(enc, tt, tm, 384)
    with torch.no_grad():
        b = enc(tt, tm)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", TRAIN)
def test_cnn_training_step_matches_reference_autograd(name):
    """Output, loss and every gradient (the word table's included) of one training step, dropout 0, vs the reference's autograd."""
    fx, enc, text, mask, R = cnn_case(name)
    enc = enc.to(_dev()).train()
    enc.dropout.p = 0.0
    out = enc(text.to(_dev()).unsqueeze(0), mask.to(_dev()).unsqueeze(0)).squeeze(0)
    assert _uses_fused(out)
    loss = (out * R.to(_dev())).sum()
    loss.backward()
    torch.cuda.synchronize()
    check_training_step(fx, enc, out, loss)


@pytest.mark.parametrize("name", ["cnn_train_default.npz", "cnn_train_group3.npz", "cnn_train_tiny.npz"])
def test_cnn_training_with_dropout_live_matches_stock_under_the_same_masks(name):
    """Both dropouts LIVE (p = 0.2): the library draws site 1's keep bits from the counter hash of `seed` over the [T Lw, dm] embedded
    tokens and site 2's from `seed + 1` over the [T Lw, Kc] activations.  forward_stock on the CPU with its two dropouts replaced by
    the oracle's restatement of that hash, and autograd: output and every gradient."""
    from oracle import digat_oracle as O
    fx, enc, text, mask, R = cnn_case(name)
    ref = _cpu_clone(enc).train()
    enc = enc.to(_dev()).train()
    enc.dropout.p = 0.2
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())           # what CnnFused.forward will draw
    torch.manual_seed(77)
    out = enc(text.to(_dev()).unsqueeze(0), mask.to(_dev()).unsqueeze(0)).squeeze(0)
    (out * R.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    site = iter((seed, seed + 1))
    del ref.dropout                                                  # a registered submodule: drop it, then a plain callable
    ref.dropout = lambda x: O.hash_dropout(x.contiguous(), 0.2, next(site))
    want = ref.forward_stock(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
    (want * R).sum().backward()
    close(out, want.detach().numpy(), "news representation under dropout", rtol=1e-5, atol=2e-6)
    assert float((want.detach() - torch.from_numpy(fx["out_news_representation"])).abs().max()) > 1e-3      # the dropout is live
    grads = dict(ref.named_parameters())
    for k, q in enc.named_parameters():
        close(q.grad, grads[k].grad.numpy(), "grad " + k + " under dropout")


def test_cnn_training_with_dropout_is_reproducible():
    def once():
        torch.manual_seed(11)
        fx, enc, text, mask, R = cnn_case("cnn_train_default.npz")
        enc = enc.to(_dev()).train()
        out = enc(text.to(_dev()).unsqueeze(0), mask.to(_dev()).unsqueeze(0)).squeeze(0)
        (out * R.to(_dev())).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), [p.grad.clone() for p in enc.parameters()]
    o1, g1 = once()
    o2, g2 = once()
    assert torch.isfinite(o1).all() and all(torch.isfinite(g).all() for g in g1)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_cnn_empty_batch_long_titles_and_bad_shapes():
    from digat_amd import _lib, synthetic
    V, dm, Kc, att = 60, 32, 24, 12
    state = synthetic.make_cnn_state(V, dm, Kc, att, "naive", 3, seed=3)
    enc = cnn_encoder(V, dm, Kc, att, 16, "naive", 3, state, dropout=0.0).to(_dev())
    # no title
    empty_t, empty_m = torch.zeros((0, 16), dtype=torch.int64, device=_dev()), torch.zeros((0, 16), dtype=torch.bool, device=_dev())
    assert enc.eval().encode_hip(empty_t, empty_m).shape == (0, Kc)
    out = enc.train()(empty_t.unsqueeze(0), empty_m.unsqueeze(0))
    out.sum().backward()
    assert out.shape == (1, 0, Kc) and all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in enc.parameters())
    # Lw = 33 in training: over the library's limit, the stock modules run instead and still match
    enc33 = cnn_encoder(V, dm, Kc, att, 33, "naive", 3, state, dropout=0.0).to(_dev()).train()
    text, mask = synthetic.make_titles(9, 33, V, seed=4)
    tt, tm = torch.from_numpy(text).to(_dev()).unsqueeze(0), torch.from_numpy(mask).to(_dev()).unsqueeze(0)
    got = enc33(tt, tm)
    got.sum().backward()
    assert not _uses_fused(got)
    np.testing.assert_allclose(got.detach().cpu().numpy(), _stock_cpu(enc33, tt, tm).numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(enc33.eval().encode_hip(tt, tm).cpu().numpy(), got.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
    # shapes the library does not take are errors, never a silent fall-back
    odd = cnn_encoder(V, 30, Kc, att, 16, "naive", 3, None).to(_dev()).eval()
    text, mask = synthetic.make_titles(4, 16, V, seed=5)
    with pytest.raises(_lib.DigatHipError):
        odd.encode_hip(torch.from_numpy(text).to(_dev()), torch.from_numpy(mask).to(_dev()))
    with pytest.raises(_lib.DigatHipError):
        enc.eval().encode_hip(torch.from_numpy(text), torch.from_numpy(mask))         # CPU tensors


def test_model_training_step_with_native_cnn_equals_stock_cnn():
    """Model.forward with the CNN news encoder feeding the DIGAT graph encoder: one training step (dropout 0) with the news encoder on
    its HIP pair against the same step with CNN.forward forced to forward_stock — finite, non-zero gradients on the convolution and
    the word table, every parameter gradient equal within the training tolerance."""
    from digat_amd import synthetic
    from digat_amd.model import Model
    B, K, N, H, C, Lw, V, dm, Kc, att, L = 4, 3, 4, 10, 5, 16, 200, 40, 80, 24, 2
    cfg = types.SimpleNamespace(news_encoder="CNN", graph_encoder="DIGAT", news_graph_size=N, max_history_num=H, category_num=C,
                                graph_depth=L, dropout_rate=0.0, vocabulary_size=V, word_embedding_dim=dm, max_title_length=Lw,
                                cnn_method="naive", cnn_kernel_num=Kc, cnn_window_size=3, attention_dim=att)
    torch.manual_seed(3)
    model = Model(cfg)
    model.initialize()
    with torch.no_grad():
        model.graph_encoder.topic_node_embedding.normal_(0, 0.02)
        model.news_encoder.word_embedding.weight.mul_(0.1)         # GloVe-like magnitudes (tests/test_hip_news.py: a well-conditioned step)
    model = model.to(_dev()).train()
    flat = synthetic.make_encoder_batch(B * K, N, H, C, Kc, seed=5)
    users = synthetic.make_encoder_batch(B, N, H, C, Kc, seed=6, empty_history_rows=(1,))
    nt, nm = synthetic.make_titles(B * K * N, Lw, V, seed=7)
    ut, um = synthetic.make_titles(B * H, Lw, V, seed=8)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    args = (d(ut).view(B, H, Lw), d(um).view(B, H, Lw), d(users["user_graph"]), d(users["user_category_mask"]),
            d(users["user_category_indices"]), d(nt).view(B, K, N, Lw), d(nm).view(B, K, N, Lw),
            d(flat["news_graph"]).view(B, K, N, N), d(flat["news_graph_mask"]).view(B, K, N))

    def step():
        model.zero_grad(set_to_none=True)
        logits = model(*args)
        loss = (-torch.log_softmax(logits, dim=1).select(1, 0)).mean()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}
    loss_hip, g_hip = step()
    for k in ("news_encoder.conv.conv.weight", "news_encoder.word_embedding.weight"):
        assert torch.isfinite(g_hip[k]).all() and float(g_hip[k].abs().max()) > 0.0, k
    enc = model.news_encoder
    enc.forward = enc.forward_stock
    try:
        loss_stock, g_stock = step()
    finally:
        del enc.forward
    assert abs(float(loss_hip) - float(loss_stock)) <= 1e-5 * max(1.0, abs(float(loss_stock)))
    for k in g_stock:
        close(g_hip[k], g_stock[k].cpu().numpy(), "grad " + k, rtol=2e-4, atol=1e-7)
