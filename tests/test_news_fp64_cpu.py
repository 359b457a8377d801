"""CPU half of the news encoders' fp64 sweeps (tests/test_hip_news_fp64.py is the GPU half).  Two things are held here:
  * the fp64 references of tests/news_fp64_common.py reproduce the vectors minted from the reference's own modules
    (tests/golden/msa_*.npz, cnn_*.npz), forward and, under autograd, every stored gradient;
  * on every case the GPU file runs, the stock fp32 modules alone stay within a QUARTER of the tolerance of their fp64 restatement,
    output and every gradient: the tolerance the kernels are held to is not already spent by the precision of the number format."""
import numpy as np
import pytest
import torch

import news_fp64_common as C
from conftest import check_grad_digest, load_golden
from test_cnn_cpu import INFERENCE as CNN_INFERENCE, TRAIN as CNN_TRAIN_FIXTURES, check_training_step, cnn_case

QUARTER = 0.25


# ---- the references against the golden fixtures ------------------------------------------------------------------------------
def _msa_fixture(name, train):
    from digat_amd import synthetic
    fx = load_golden(name)
    T_, Lw, V, dm, h, dk, att = (int(v) for v in fx["meta"])
    seeds = [int(v) for v in fx["seeds"]]
    state = synthetic.make_msa_state(V, dm, h, dk, att, seed=seeds[0])
    text, mask = synthetic.make_titles(T_, Lw, V, seed=seeds[1])
    parts = [text, mask]
    R = None
    if train:
        text[2], mask[2] = 0, False                                # one title is all padding (tests/test_hip_news.py:_train_case)
        R = np.random.default_rng(seeds[2]).standard_normal((T_, h * dk)).astype(np.float32)
        parts.append(R)
    tot = sum(float(np.asarray(v, dtype=np.float64).sum()) for v in parts + list(state.values()))
    assert abs(tot - float(fx["input_checksum"])) <= 1e-6 * max(1.0, abs(tot)), "synthetic generator drifted from the fixture's"
    return fx, state, torch.from_numpy(text), torch.from_numpy(mask), h, R


@pytest.mark.parametrize("name", ["msa_tiny.npz", "msa_default.npz"])
def test_msa_fp64_reproduces_reference_vectors(name):
    fx, state, text, mask, h, _ = _msa_fixture(name, train=False)
    with torch.no_grad():
        got = C.msa_fp64(state, text, mask, h)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), fx["out_news_representation"], rtol=1e-5, atol=1e-6)      # tests/test_oracle_golden.py's


@pytest.mark.parametrize("name", ["msa_train_tiny.npz", "msa_train_default.npz"])
def test_msa_fp64_autograd_reproduces_reference_gradients(name):
    """Against the fixture's float64 block, at tests/test_oracle_golden.py's tolerances (allclose 1e-5 / 1e-5, digests 2e-5)."""
    f, state, text, mask, h, R = _msa_fixture(name, train=True)
    fx = {k[len("f64_"):]: v for k, v in f.items() if k.startswith("f64_")}
    p = C.fp64_params(state)
    out = C.msa_fp64(p, text, mask, h)
    loss = (out * torch.from_numpy(R).double()).sum()
    loss.backward()
    np.testing.assert_allclose(out.detach().numpy(), fx["out_news_representation"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss.detach().numpy(), fx["out_loss"], rtol=1e-5, atol=1e-5)
    for k, v in p.items():
        assert v.grad is not None and v.grad.dtype == torch.float64, k
        if "g_" + k in fx:
            np.testing.assert_allclose(v.grad.numpy(), fx["g_" + k], rtol=1e-5, atol=1e-5, err_msg="grad " + k)
        else:
            check_grad_digest(fx, k, v.grad.numpy(), 2e-5, "grad ")


@pytest.mark.parametrize("name", CNN_INFERENCE)
def test_cnn_fp64_reproduces_reference_vectors(name):
    fx, enc, text, mask, _ = cnn_case(name)
    with torch.no_grad():
        got = C.cnn_fp64(enc, text, mask)
    assert got.dtype == torch.float64 and next(enc.parameters()).dtype == torch.float32       # the encoder itself is left alone
    np.testing.assert_allclose(got.numpy(), fx["out_news_representation"], rtol=1e-5, atol=2e-6)      # tests/test_cnn_cpu.py's


@pytest.mark.parametrize("name", CNN_TRAIN_FIXTURES)
def test_cnn_fp64_autograd_reproduces_reference_gradients(name):
    fx, enc, text, mask, R = cnn_case(name)
    enc.train()
    enc.dropout.p = 0.0
    ref = C.cnn_fp64_module(enc)
    out = C.cnn_fp64(ref, text, mask)
    loss = (out * R.double()).sum()
    loss.backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float64 for p in ref.parameters())
    check_training_step(fx, ref, out, loss)


def test_case_lists_cover_what_they_are_meant_to():
    """The properties the lists are chosen for, so that an edit of the lists cannot quietly lose a kernel variant."""
    assert {(c.dk + 3) // 4 for c in C.MSA_INFER} == set(range(1, 9)) == {(c.dk + 3) // 4 for c in C.MSA_TRAIN}
    lds = lambda c: 16 * (2 * c.Lw * c.dk + c.Lw * (c.Lw + 1))
    assert max(lds(c) for c in C.MSA_INFER) == 132096
    assert [lds(C.MsaCase(1, Lw, 4, 25, 32, 12, 60)) > 65536 for Lw in (43, 44)] == [False, True]
    assert all(c.T * c.Lw >= 2048 and (c.heads * c.dk) % 80 == 0 and c.dm >= 32 for c in C.MSA_ROWLIST)
    assert all(c.T * c.Lw < 2048 for c in C.MSA_GATHER) and all(c.T * c.Lw >= 2048 for c in C.MSA_TRAIN_BIG + C.CNN_TRAIN_BIG)
    tiled = [c for c in C.CNN_INFER if c.Lw >= 16 and c.T * c.Lw >= 2048]
    assert {128 // c.Lw for c in tiled} == set(range(2, 9)) and all(c.T % (128 // c.Lw) for c in tiled + C.CNN_TRAIN_BIG)
    assert any(c.Lw == 16 and c.window == 7 and c.method == "naive" for c in tiled)              # arows = 8 x 22 = CNN_MAX_AROWS
    assert any(c.window == 1 and c.method == "naive" for c in tiled)
    assert {(c.method, c.window) for c in C.CNN_TRAIN_BIG} == set(C.WINDOWS) and all(c.Kc >= 32 and c.dm >= 32 for c in C.CNN_TRAIN_BIG)
    every = C.MSA_INFER + C.MSA_ROWLIST + C.MSA_GATHER + C.MSA_TRAIN + C.MSA_TRAIN_BIG + C.MSA_PERM + C.CNN_INFER + C.CNN_TRAIN + C.CNN_TRAIN_BIG + C.CNN_PERM
    assert all(c.T <= 140 and (c.dm <= 64 or c == C.MSA_ROWLIST[3] or c == C.MSA_GATHER[3]) for c in every)


# ---- headroom: stock fp32 against fp64, a quarter of the tolerance ------------------------------------------------------------
def _msa_headroom(case, train):
    state, text, mask, R = C.msa_inputs(case)
    enc = C.msa_encoder(case, state)
    what = f"fp32 {case}"
    if not train:
        with torch.no_grad():
            got = enc.eval().forward_stock(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
            return C.close(got, C.msa_fp64(state, text, mask, case.heads), what, **C.OUT_TOL), 0.0
    enc.train()
    out = enc.forward_stock(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
    (out * R).sum().backward()
    p = C.fp64_params(state)
    want = C.msa_fp64(p, text, mask, case.heads)
    (want * R.double()).sum().backward()
    grad = max(C.close(v.grad, p[k].grad, f"{what} grad {k}", **C.GRAD_TOL) for k, v in enc.named_parameters())
    return C.close(out, want, what, **C.OUT_TOL), grad


def _cnn_headroom(case, train):
    enc, text, mask, R = C.cnn_inputs(case)
    what = f"fp32 {case}"
    if not train:
        with torch.no_grad():
            got = enc.eval().forward_stock(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
            return C.close(got, C.cnn_fp64(enc, text, mask), what, **C.OUT_TOL), 0.0
    enc.train()
    ref = C.cnn_fp64_module(enc)
    out = enc.forward_stock(text.unsqueeze(0), mask.unsqueeze(0)).squeeze(0)
    (out * R).sum().backward()
    want = C.cnn_fp64(ref, text, mask)
    (want * R.double()).sum().backward()
    grads = dict(ref.named_parameters())
    grad = max(C.close(v.grad, grads[k].grad, f"{what} grad {k}", **C.GRAD_TOL) for k, v in enc.named_parameters())
    return C.close(out, want, what, **C.OUT_TOL), grad


def _quarter(cases, fn, train):
    worst_out = worst_grad = 0.0
    for case in cases:
        o, g = fn(case, train)
        assert o <= QUARTER and g <= QUARTER, f"{case}: fp32 alone uses {o:.3f} (output) / {g:.3f} (gradients) of the tolerance"
        worst_out, worst_grad = max(worst_out, o), max(worst_grad, g)
    print(f"fp32 against fp64, worst err/tol: output {worst_out:.3f}, gradients {worst_grad:.3f} over {len(cases)} cases")


@pytest.mark.parametrize("Lw", C.MSA_LW)
def test_fp32_headroom_msa_inference(Lw):
    _quarter([c for c in C.MSA_INFER if c.Lw == Lw], _msa_headroom, False)


def test_fp32_headroom_msa_projection_routes_and_pair_cases():
    _quarter(C.MSA_ROWLIST + C.MSA_GATHER + C.MSA_PERM, _msa_headroom, False)


@pytest.mark.parametrize("Lw", C.MSA_TRAIN_LW)
def test_fp32_headroom_msa_training(Lw):
    _quarter([c for c in C.MSA_TRAIN if c.Lw == Lw], _msa_headroom, True)


def test_fp32_headroom_msa_training_large_masked_and_pair_cases():
    _quarter(C.MSA_TRAIN_BIG + C.MSA_TRAIN_NONE + C.MSA_PAIR, _msa_headroom, True)


@pytest.mark.parametrize("Lw", C.CNN_LW)
def test_fp32_headroom_cnn_inference(Lw):
    _quarter([c for c in C.CNN_INFER if c.Lw == Lw], _cnn_headroom, False)


@pytest.mark.parametrize("Lw", C.CNN_TRAIN_LW)
def test_fp32_headroom_cnn_training(Lw):
    _quarter([c for c in C.CNN_TRAIN if c.Lw == Lw], _cnn_headroom, True)


def test_fp32_headroom_cnn_large_and_pair_cases():
    _quarter(C.CNN_PERM, _cnn_headroom, False)
    _quarter(C.CNN_TRAIN_BIG + C.CNN_PAIR, _cnn_headroom, True)
