"""CPU suite for the CNN news encoder (newsEncoders.py:29-54, layers.Conv1D / layers.Attention): the stock PyTorch module against
the vectors minted from the reference's own modules (tools/make_cnn_golden.py), the group3 = zero-filled 5-tap identity the HIP path
rests on, the configuration flags, and the digat_cnn_* C ABI without a device."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_grad_digest, load_golden

METHODS = ("naive", "group3")
INFERENCE = ["cnn_tiny.npz", "cnn_default.npz", "cnn_w5.npz", "cnn_group3.npz"]
TRAIN = ["cnn_train_tiny.npz", "cnn_train_default.npz", "cnn_train_group3.npz"]


def cnn_encoder(V, dm, Kc, att, Lw, method, window, state=None, dropout=0.2):
    from digat_amd import newsEncoders
    cfg = types.SimpleNamespace(vocabulary_size=V, word_embedding_dim=dm, max_title_length=Lw, dropout_rate=dropout,
                                cnn_method=method, cnn_kernel_num=Kc, cnn_window_size=window, attention_dim=att)
    enc = newsEncoders.CNN(cfg)
    if state is not None:
        res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    return enc


def cnn_case(name):
    """(fixture, encoder in eval mode on the CPU, text, mask, R or None) of a cnn_*.npz fixture, inputs regenerated from its seeds."""
    from digat_amd import synthetic
    fx = load_golden(name)
    T_, Lw, V, dm, Kc, att, mi, window = (int(v) for v in fx["meta"])
    seeds = [int(v) for v in fx["seeds"]]
    state = synthetic.make_cnn_state(V, dm, Kc, att, METHODS[mi], window, seed=seeds[0])
    text, mask = synthetic.make_titles(T_, Lw, V, seed=seeds[1])
    text[2], mask[2] = 0, False                                    # one title is all padding: uniform pooling (layers.py:111)
    parts = {"t": text, "m": mask}
    R = None
    if len(seeds) == 3:
        R = np.random.default_rng(seeds[2]).standard_normal((T_, Kc)).astype(np.float32)
        parts["r"] = R
    tot = sum(float(np.asarray(v, dtype=np.float64).sum()) for v in list(parts.values()) + list(state.values()))
    assert abs(tot - float(fx["input_checksum"])) <= 1e-6 * max(1.0, abs(tot)), "synthetic generator drifted from the fixture's"
    enc = cnn_encoder(V, dm, Kc, att, Lw, METHODS[mi], window, state).eval()
    return fx, enc, torch.from_numpy(text), torch.from_numpy(mask), None if R is None else torch.from_numpy(R)


def close(got, want, what, rtol=2e-4, atol=2e-6):
    """tests/test_hip_news.py:_close."""
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    scale = max(float(np.abs(want).max()), 1e-12)
    err = np.abs(got - want)
    tol = atol + rtol * np.maximum(np.abs(want), 0.05 * scale)
    assert not (err > tol).any(), f"{what}: max|diff| {err.max():.3e} (scale {scale:.3e})"


def check_training_step(fx, enc, out, loss):
    """Output, loss and every gradient of a finished backward against a cnn_train_*.npz fixture (tolerances: tests/test_hip_news.py)."""
    close(out, fx["out_news_representation"], "news representation", rtol=1e-5, atol=2e-6)
    close(loss, fx["out_loss"], "loss", rtol=2e-5, atol=1e-5)
    for k, p in enc.named_parameters():
        assert p.grad is not None, k
        if "g_" + k in fx:
            close(p.grad, fx["g_" + k], "grad " + k)
        else:
            check_grad_digest(fx, k, p.grad.detach().cpu().numpy(), 2e-4, "grad ")


@pytest.mark.parametrize("name", INFERENCE)
def test_stock_cnn_matches_reference_vectors(name):
    fx, enc, text, mask, _ = cnn_case(name)
    with torch.no_grad():
        got = enc(text.unsqueeze(1), mask.unsqueeze(1)).squeeze(1)
    np.testing.assert_allclose(got.numpy(), fx["out_news_representation"], rtol=1e-5, atol=2e-6)
    assert np.allclose(got.numpy()[2], enc.conv(enc.word_embedding(text[2:3]).permute(0, 2, 1)).mean(dim=2).detach().numpy()[0],
                       rtol=1e-5, atol=2e-6), "an all-padding title pools uniformly"


@pytest.mark.parametrize("name", TRAIN)
def test_stock_cnn_training_step_matches_reference_autograd(name):
    fx, enc, text, mask, R = cnn_case(name)
    enc.train()
    enc.dropout.p = 0.0
    out = enc(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
    loss = (out * R).sum()
    loss.backward()
    check_training_step(fx, enc, out, loss)


def test_group3_is_the_zero_filled_five_tap_convolution():
    """The HIP path runs group3 as ONE 5-tap convolution whose weight is zero where a branch has no tap: same values up to the
    summation order (forward tolerance, not bit for bit), and the merged weight's gradient cut back gives each branch's gradient."""
    from digat_amd import newsEncoders, synthetic
    T_, Lw, V, dm, Kc, att = 72, 32, 500, 300, 396, 256
    state = synthetic.make_cnn_state(V, dm, Kc, att, "group3", 3, seed=5)
    enc = cnn_encoder(V, dm, Kc, att, Lw, "group3", 3, state)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((T_, dm, Lw)).astype(np.float32))
    c1, c2, c3 = enc.conv.conv1, enc.conv.conv2, enc.conv.conv3
    W = newsEncoders.merge_group3(c1.weight.detach(), c2.weight.detach(), c3.weight.detach())
    b = torch.cat([c1.bias, c2.bias, c3.bias]).detach()
    assert W.shape == (Kc, dm, 5) and float(W[:Kc // 3, :, [0, 1, 3, 4]].abs().max()) == 0.0 and float(W[Kc // 3:2 * Kc // 3, :, [0, 4]].abs().max()) == 0.0
    W.requires_grad_(True)
    merged = F.conv1d(x, W, b, padding=2)
    branches = torch.cat([c1(x), c2(x), c3(x)], dim=1)
    np.testing.assert_allclose(merged.detach().numpy(), branches.detach().numpy(), rtol=1e-5, atol=2e-6)
    G = torch.from_numpy(np.random.default_rng(7).standard_normal(tuple(merged.shape)).astype(np.float32))
    (merged * G).sum().backward()
    (branches * G).sum().backward()
    K3 = Kc // 3
    close(W.grad[:K3, :, 2:3], c1.weight.grad.numpy(), "conv1.weight")
    close(W.grad[K3:2 * K3, :, 1:4], c2.weight.grad.numpy(), "conv2.weight")
    close(W.grad[2 * K3:], c3.weight.grad.numpy(), "conv3.weight")


def test_config_builds_a_cnn_model_and_unsupported_methods_raise():
    from digat_amd.config import Config
    from digat_amd.model import Model
    from digat_amd import newsEncoders
    cfg = Config(['--news_encoder', 'CNN'])
    assert (cfg.cnn_method, cfg.cnn_kernel_num, cfg.cnn_window_size, cfg.attention_dim) == ('naive', 400, 3, 256)
    assert (cfg.MSA_head_num, cfg.MSA_head_dim, cfg.word_embedding_dim) == (16, 25, 300)
    cfg.vocabulary_size, cfg.max_title_length = 50, 12             # set by the corpus in the reference (MIND_corpus.py)
    model = Model(cfg)
    model.initialize()
    assert isinstance(model.news_encoder, newsEncoders.CNN) and model.news_embedding_dim == 400
    assert {"conv.conv.weight", "conv.conv.bias"} <= set(model.news_encoder.state_dict())
    text = torch.randint(1, 50, (2, 3, 12))
    out = model.news_encoder(text, torch.ones(2, 3, 12, dtype=torch.bool))
    assert out.shape == (2, 3, 400) and torch.isfinite(out).all()
    g3 = Config(['--news_encoder', 'CNN', '--cnn_method', 'group3', '--cnn_kernel_num', '396'])
    g3.vocabulary_size, g3.max_title_length = 50, 12
    assert {"conv.conv1.weight", "conv.conv2.bias", "conv.conv3.weight"} <= set(Model(g3).news_encoder.state_dict())
    for argv in (['--cnn_method', 'group5'], ['--cnn_method', 'group4'], ['--cnn_window_size', '4']):
        bad = Config(['--news_encoder', 'CNN'] + argv)
        bad.vocabulary_size, bad.max_title_length = 50, 12
        with pytest.raises(ValueError, match=r"layers\.py"):
            Model(bad)


def test_cnn_abi_without_a_device():
    """The digat_cnn_* family: exported, byte counts monotone in T and zero-safe, argument / shape / workspace codes before any launch."""
    from digat_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    names = ["digat_cnn_split_bytes", "digat_split_cnn_weights", "digat_cnn_merge_group3", "digat_cnn_workspace_bytes", "digat_cnn_fwd",
             "digat_cnn_train_save_bytes", "digat_cnn_train_workspace_bytes", "digat_cnn_fwd_train", "digat_cnn_bwd"]
    for n in names:
        assert hasattr(L, n) and n in _lib.EXPORTED, n
    assert L.digat_version() == 4
    for fn in (L.digat_cnn_workspace_bytes, L.digat_cnn_train_save_bytes, L.digat_cnn_train_workspace_bytes):
        sizes = [fn(T_, 32, 300, 400, 3, 256) for T_ in (0, 1, 72, 300, 4099)]
        assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
        assert fn(-1, 32, 300, 400, 3, 256) == 0
    assert L.digat_cnn_workspace_bytes(72, 32, 300, 400, 3, 256) >= 72 * 32 * (400 + 256) * 4
    assert L.digat_cnn_split_bytes(300, 400, 3) >= 3 * 300 * 400 * 6 and L.digat_cnn_split_bytes(300, 400, 5) > L.digat_cnn_split_bytes(300, 400, 3)
    assert L.digat_cnn_split_bytes(0, 400, 3) == 0
    ARG, SHAPE, WORKSPACE = 1, 2, 3
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)                                      # a non-null HOST address: every check below fails before it is read

    def params(dm=300, Kc=400, taps=3, att=256):
        P = _lib.CnnParams(word_embedding_dim=dm, kernel_num=Kc, taps=taps, attention_dim=att)
        for k in ("word_embedding", "W", "b", "A1", "b1", "a2"):
            setattr(P, k, a)
        return P
    assert L.digat_cnn_fwd(None, a, a, a, 4, 32, a, 1 << 30, None) == ARG
    assert L.digat_cnn_fwd(params(), None, a, a, 4, 32, a, 1 << 30, None) == ARG
    assert L.digat_cnn_fwd(params(), a, a, a, -1, 32, a, 1 << 30, None) == ARG
    for bad in (params(dm=30), params(Kc=402), params(taps=4), params(taps=9), params(att=0)):
        assert L.digat_cnn_fwd(bad, a, a, a, 4, 32, a, 1 << 30, None) == SHAPE
    assert L.digat_cnn_fwd(params(), a, a, a, 4, 65, a, 1 << 30, None) == SHAPE
    assert L.digat_cnn_fwd(params(), a, a, a, 4, 32, a, 16, None) == WORKSPACE
    assert L.digat_cnn_fwd(params(), a, a, a, 0, 32, a, 0, None) == 0            # no title: nothing is launched
    assert L.digat_cnn_fwd_train(params(), a, a, a, 0.2, 1, 4, 33, a, 1 << 30, a, 1 << 30, None) == SHAPE     # training: Lw <= 32
    assert L.digat_cnn_fwd_train(params(), a, a, a, 1.0, 1, 4, 32, a, 1 << 30, a, 1 << 30, None) == ARG
    assert L.digat_cnn_fwd_train(params(), a, a, a, 0.2, 1, 4, 32, a, 16, a, 1 << 30, None) == WORKSPACE
    assert L.digat_cnn_fwd_train(params(), a, a, a, 0.2, 1, 0, 32, a, 0, a, 0, None) == 0
    assert L.digat_cnn_bwd(params(), a, a, None, 0.2, 1, a, 1 << 30, a, 300, a, a, a, a, a, 4, 32, a, 1 << 30, None) == ARG
    assert L.digat_cnn_bwd(params(), a, a, a, 0.2, 1, a, 1 << 30, a, 298, a, a, a, a, a, 4, 32, a, 1 << 30, None) == ARG      # ld < dm
    assert L.digat_cnn_bwd(params(), a, a, a, 0.2, 1, a, 1 << 30, a, 300, a, a, a, a, a, 4, 32, a, 16, None) == WORKSPACE
    assert L.digat_split_cnn_weights(None, 300, 400, 3, a, None) == ARG
    assert L.digat_split_cnn_weights(a, 300, 400, 4, a, None) == SHAPE
    assert L.digat_cnn_merge_group3(a, a, a, a, a, a, 300, 400, a, a, None) == SHAPE             # 400 % 3
