"""GPU suite: both DIGAT news encoders (newsEncoders.MSA on digat_msa_fwd / digat_msa_fwd_train / digat_msa_bwd, newsEncoders.CNN on
digat_cnn_fwd / digat_cnn_fwd_train / digat_cnn_bwd) against fp64 references, over every kernel variant and every title length at
which the code changes its path (the case lists and what each is chosen for: tests/news_fp64_common.py).  tests/test_news_fp64_cpu.py
pins the references to the golden fixtures and holds fp32 arithmetic alone to a quarter of the tolerances used here.

Tolerances: the project's for this pipeline (tests/test_hip_news.py) — the news representation rtol 1e-5 / atol 2e-6, every gradient
rtol 2e-4 / atol 2e-6, relative to max(|want|, 5 % of the tensor's scale).  Two checks need none: a permutation of the titles of a batch
permutes the output bit for bit (no bleed between the titles of a tile), and scratch memory filled with 0xFF changes no bit (nothing
is read before it is written; the padded columns of `pre` are never read).

Worst err / tol per group, measured on an MI355X (every figure is to stay below 1; nothing is tuned to them):
    MSA inference     output 0.057 (Lw = 1); 0.031 at Lw >= 33, 0.027 on the row-list / gather cases
    MSA training      output 0.046, gradients 0.098 (Lw = 31); 0.025 / 0.089 on the >= 2 048-row cases
    CNN inference     output 0.107 (Lw = 16)
    CNN training      output 0.092, gradients 0.121 (Lw = 17); 0.062 / 0.045 on the >= 2 048-row cases
    permutation       bit-identical in all seven cases (0)
    poisoned scratch  bit-identical and finite in all four cases, inference and training pair (0)
The stock fp32 modules on a CPU, held to 0.25 on the same cases by tests/test_news_fp64_cpu.py, reach 0.07 (output) / 0.10 (gradients)
for MSA and 0.11 / 0.07 for CNN: the kernels are no further from fp64 than fp32 arithmetic is.
"""
import pytest
import torch

import news_fp64_common as C

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _uses_fused(t, name):
    """Whether ``t`` was produced through the autograd function ``name`` (the HIP training pair): tests/test_hip_cnn.py:_uses_fused."""
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


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(group, cases, out, grad=None):
    print(f"{group}: worst err/tol output {out:.3f}" + ("" if grad is None else f", gradients {grad:.3f}") + f" over {cases} cases")


# ---- MSA inference ---------------------------------------------------------------------------------------------------------------
def _msa_infer(case, dispatch):
    state, text, mask, _ = C.msa_inputs(case)
    enc = C.msa_encoder(case, state).to(_dev()).eval()
    tt, tm = text.to(_dev()), mask.to(_dev())
    got = enc.encode_hip(tt, tm)                                    # called directly: the stock path cannot satisfy this
    with torch.no_grad():
        want = C.msa_fp64(state, text, mask, case.heads)
        none = mask.sum(dim=1) == 0
        if bool(none.any()):                                        # guards the reference: -1e9 on every position pools uniformly
            h = C.msa_h_fp64(state, text[none], case.heads)
            assert torch.allclose(want[none], h.mean(dim=1), rtol=1e-12, atol=1e-12), case
    ratio = C.close(got, want, f"MSA inference {case}", **C.OUT_TOL)
    if dispatch:                                                    # the module goes there under no_grad, whatever the length
        with torch.no_grad():
            assert _same_bits(enc(tt.unsqueeze(0), tm.unsqueeze(0)).squeeze(0), got), case
    return ratio


@pytest.mark.parametrize("Lw", C.MSA_LW)
def test_msa_inference_sweep_against_fp64(Lw):
    cases = [c for c in C.MSA_INFER if c.Lw == Lw]
    assert C.MASKS[4] == "none" and any(c.T >= 5 and c.kind == "mixed" for c in cases)               # an all-masked title is among them
    worst = max(_msa_infer(c, dispatch=(c.T == 3)) for c in cases)
    _report(f"MSA inference Lw={Lw}", len(cases), worst)


@pytest.mark.parametrize("case", C.MSA_ROWLIST + C.MSA_GATHER, ids=lambda c: f"T{c.T}-Lw{c.Lw}-dm{c.dm}")
def test_msa_inference_projection_routes_against_fp64(case):
    """The Q|K|V product with the token ids as its row list (>= 2 048 rows) and on gathered embeddings (just below)."""
    _report(f"MSA inference {case}", 1, _msa_infer(case, dispatch=True))


# ---- MSA training pair ----------------------------------------------------------------------------------------------------------
def _msa_train(case):
    """(worst err/tol of the output, of the gradients, {parameter: fp64 gradient})"""
    state, text, mask, R = C.msa_inputs(case)
    enc = C.msa_encoder(case, state).to(_dev()).train()
    enc.dropout.p = 0.0
    out = enc(text.to(_dev()).unsqueeze(0), mask.to(_dev()).unsqueeze(0)).squeeze(0)
    assert _uses_fused(out, "MsaFused"), case
    (out * R.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    p = C.fp64_params(state)
    want = C.msa_fp64(p, text, mask, case.heads)
    (want * R.double()).sum().backward()
    o = C.close(out, want, f"MSA training {case}", **C.OUT_TOL)
    g = 0.0
    for k, v in enc.named_parameters():
        assert v.grad is not None, k
        g = max(g, C.close(v.grad, p[k].grad, f"MSA training {case} grad {k}", **C.GRAD_TOL))
    return o, g, {k: v.grad for k, v in p.items()}


def _worst(results):
    results = list(results)
    return max(r[0] for r in results), max(r[1] for r in results)


@pytest.mark.parametrize("Lw", C.MSA_TRAIN_LW)
def test_msa_training_sweep_against_fp64_autograd(Lw):
    """Output and every gradient, the word table's included (V = 20: its rows collect several tokens each)."""
    cases = [c for c in C.MSA_TRAIN if c.Lw == Lw]
    _report(f"MSA training Lw={Lw}", len(cases), *_worst(_msa_train(c) for c in cases))


@pytest.mark.parametrize("case", C.MSA_TRAIN_BIG, ids=lambda c: f"T{c.T}-Lw{c.Lw}")
def test_msa_training_on_the_matrix_core_products_against_fp64_autograd(case):
    _report(f"MSA training {case}", 1, *_msa_train(case)[:2])


@pytest.mark.parametrize("case", C.MSA_TRAIN_NONE, ids=lambda c: f"Lw{c.Lw}")
def test_msa_title_masked_throughout_sends_no_gradient_to_the_pooling_weights(case):
    """-1e9 replaces every score of the title: nothing flows to affine1 / affine2 through it (read off the fp64 gradient), while the
    uniform pooling still carries the gradient to the projections and the word table."""
    o, g, ref = _msa_train(case)
    for k in ("attention.affine1.weight", "attention.affine1.bias", "attention.affine2.weight"):
        assert float(ref[k].abs().max()) == 0.0, k
    assert float(ref["multiheadSelfattention.W_V.weight"].abs().max()) > 0.0 and float(ref["word_embedding.weight"].abs().max()) > 0.0
    _report(f"MSA training {case}", 1, o, g)


# ---- CNN -------------------------------------------------------------------------------------------------------------------------
def _cnn_infer(case, dispatch):
    enc, text, mask, _ = C.cnn_inputs(case)
    with torch.no_grad():
        want = C.cnn_fp64(enc, text, mask)
    enc = enc.to(_dev()).eval()
    tt, tm = text.to(_dev()), mask.to(_dev())
    got = enc.encode_hip(tt, tm)
    ratio = C.close(got, want, f"CNN inference {case}", **C.OUT_TOL)
    if dispatch:
        with torch.no_grad():
            assert _same_bits(enc(tt.unsqueeze(0), tm.unsqueeze(0)).squeeze(0), got), case
    return ratio


@pytest.mark.parametrize("Lw", C.CNN_LW)
def test_cnn_inference_sweep_against_fp64(Lw):
    """Every window on the plain kernel and, from Lw = 16, on the tiled one with a ragged last tile."""
    cases = [c for c in C.CNN_INFER if c.Lw == Lw]
    worst = max(_cnn_infer(c, dispatch=(c.window == 3 and c.method == "naive")) for c in cases)
    _report(f"CNN inference Lw={Lw}", len(cases), worst)


def _cnn_train(case):
    enc, text, mask, R = C.cnn_inputs(case)
    enc.train()
    ref = C.cnn_fp64_module(enc)
    want = C.cnn_fp64(ref, text, mask)
    (want * R.double()).sum().backward()
    enc = enc.to(_dev())
    out = enc(text.to(_dev()).unsqueeze(0), mask.to(_dev()).unsqueeze(0)).squeeze(0)
    assert _uses_fused(out, "CnnFused"), case
    (out * R.to(_dev())).sum().backward()
    torch.cuda.synchronize()
    o = C.close(out, want, f"CNN training {case}", **C.OUT_TOL)
    grads = dict(ref.named_parameters())
    g = 0.0
    for k, v in enc.named_parameters():
        assert v.grad is not None, k
        g = max(g, C.close(v.grad, grads[k].grad, f"CNN training {case} grad {k}", **C.GRAD_TOL))
    return o, g


@pytest.mark.parametrize("Lw", C.CNN_TRAIN_LW)
def test_cnn_training_sweep_against_fp64_autograd(Lw):
    cases = [c for c in C.CNN_TRAIN if c.Lw == Lw]
    _report(f"CNN training Lw={Lw}", len(cases), *_worst(_cnn_train(c) for c in cases))


@pytest.mark.parametrize("case", C.CNN_TRAIN_BIG, ids=lambda c: f"{c.method}{c.window}-Lw{c.Lw}")
def test_cnn_training_on_the_tiled_kernel_against_fp64_autograd(case):
    """>= 2 048 rows: the forward and the flipped-weight input gradient both on cnn_conv_tiled_kernel."""
    _report(f"CNN training {case}", 1, *_cnn_train(case))


# ---- what a tolerance cannot show ------------------------------------------------------------------------------------------------
def _encoder_and_titles(case):
    if isinstance(case, C.MsaCase):
        state, text, mask, R = C.msa_inputs(case)
        enc = C.msa_encoder(case, state)
    else:
        enc, text, mask, R = C.cnn_inputs(case)
    return enc.to(_dev()), text.to(_dev()), mask.to(_dev()), R.to(_dev())


@pytest.mark.parametrize("case", C.MSA_PERM + C.CNN_PERM, ids=lambda c: f"{type(c).__name__}-T{c.T}-Lw{c.Lw}")
def test_permuting_the_titles_permutes_the_output_bit_for_bit(case):
    """The same T in both calls, so the same kernels and tiles: each output element's summation order depends on K alone, and a title
    reads nothing of its neighbours in a tile.  A random permutation, and a rotation by one: every title changes its slot in its tile."""
    enc, tt, tm, _ = _encoder_and_titles(case)
    enc.eval()
    base = enc.encode_hip(tt, tm)
    assert torch.isfinite(base).all()
    g = torch.Generator().manual_seed(case.T)
    for name, perm in (("random", torch.randperm(case.T, generator=g)), ("rotation", torch.roll(torch.arange(case.T), 1))):
        perm = perm.to(_dev())
        assert _same_bits(enc.encode_hip(tt[perm].contiguous(), tm[perm].contiguous()), base[perm]), (case, name)


def _fill_scratch(byte):
    """Every cached workspace of the library calls (digat_amd._lib.workspace) filled with ``byte``."""
    from digat_amd import _lib
    for buf in _lib._workspaces.values():
        buf.fill_(byte)


@pytest.mark.parametrize("case", C.MSA_PAIR + C.CNN_PAIR, ids=lambda c: f"{type(c).__name__}-T{c.T}-Lw{c.Lw}")
def test_poisoned_scratch_changes_no_bit(case, monkeypatch):
    """tests/test_hip_nrms.py:test_nan_filled_workspace_and_save_change_no_bit for these two encoders: the cached workspace filled with
    zeros and then with 0xFF bytes (NaN as floats) between identical calls; for the training pair the `save` buffer and the workspace
    before the forward, and the workspace again before the backward.  att = 100 and 12: `pre` has padded columns."""
    from digat_amd import _lib
    enc, tt, tm, R = _encoder_and_titles(case)
    enc.eval()
    enc.encode_hip(tt, tm)                                          # allocates the workspace the next calls reuse
    outs = []
    for byte in (0x00, 0xFF):
        _fill_scratch(byte)
        outs.append(enc.encode_hip(tt, tm).clone())
    assert torch.isfinite(outs[0]).all() and _same_bits(outs[0], outs[1]), case

    enc.train()
    enc.dropout.p = 0.0
    fill = [0x00]
    monkeypatch.setattr(_lib, "save_buffer", lambda nbytes, device: torch.full((max(int(nbytes), 256),), fill[0], dtype=torch.uint8, device=device))

    def step():
        enc.zero_grad(set_to_none=True)
        _fill_scratch(fill[0])
        out = enc(tt.unsqueeze(0), tm.unsqueeze(0)).squeeze(0)
        assert _uses_fused(out, "MsaFused" if isinstance(case, C.MsaCase) else "CnnFused")
        _fill_scratch(fill[0])
        (out * R).sum().backward()
        torch.cuda.synchronize()
        return [out.detach().clone()] + [p.grad.clone() for p in enc.parameters()]
    step()                                                          # allocates the workspaces (the embedding backward's included)
    clean = step()
    fill[0] = 0xFF
    poisoned = step()
    assert all(torch.isfinite(t).all() for t in clean), case
    assert all(_same_bits(a, b) for a, b in zip(clean, poisoned)), case
