"""Shared by tests/test_nrms_cpu.py and tests/test_hip_nrms.py: the nrms_*.npz fixtures (tools/make_golden_nrms.py) with their inputs
and weights regenerated from the stored seeds, and the comparison the news-encoder tests use."""
import functools
import types

import numpy as np
import torch

from conftest import check_grad_digest, load_golden

MODELS = {"nrms": "NRMS", "sa": "NRMS-SA"}


def close(got, want, what, rtol=1e-5, atol=2e-6):
    """tests/test_hip_news.py:_close: relative to the larger of |want| and 5 % of the tensor's scale."""
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    scale = max(float(np.abs(want).max()), 1e-12)
    err = np.abs(got - want)
    tol = atol + rtol * np.maximum(np.abs(want), 0.05 * scale)
    assert not (err > tol).any(), f"{what}: max|diff| {err.max():.3e} (scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def case(name):
    """(fixture, config fields, inputs as numpy, {prefix: state}) of an nrms_*.npz fixture; the regenerated inputs are held to its checksum."""
    from digat_amd import synthetic
    fx = load_golden(name)
    N, A, Lw, V, dm, heads, dk, att, U, H, K = (int(v) for v in fx["meta"])
    s_w, s_in = (int(v) for v in fx["seeds"])
    inp = synthetic.make_nrms_inputs(N, A, Lw, V, U, H, K, seed=s_in)
    states, tot = {}, 0.0
    for pre in MODELS:
        states[pre] = synthetic.make_nrms_state(V, dm, heads, dk, att, sa=(pre == "sa"), seed=s_w, user_qk_gain=float(fx["user_qk_gain"]))
        tot += sum(float(np.asarray(v, dtype=np.float64).sum()) for v in list(inp.values()) + list(states[pre].values()))
    assert abs(tot - float(fx["input_checksum"])) <= 1e-6 * max(1.0, abs(tot)), "synthetic generator drifted from the fixture's"
    cfg = dict(vocabulary_size=V, word_embedding_dim=dm, head_num=heads, head_dim=dk, attention_dim=att, max_title_length=Lw,
               max_history_num=H, augmented_news_num=A)
    return fx, cfg, inp, states


def model(name, pre, device="cpu", dropout=0.0):
    from digat_amd import nrms
    fx, cfg, inp, states = case(name)
    m = nrms.Model(nrms.make_config(model=MODELS[pre], dropout_rate=dropout, **cfg))
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in states[pre].items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(device)


def tensors(name, device="cpu"):
    _, _, inp, _ = case(name)
    return {k: torch.from_numpy(v.astype(np.int64)).to(device) for k, v in inp.items()}


def dev_set(name, device="cpu"):
    """The fixture's impressions as the corpus-like object nrms.compute_scores reads: every user's candidates, impression-major."""
    _, _, inp, _ = case(name)
    t = tensors(name, device)
    U, K = inp["candidate_ids"].shape
    return types.SimpleNamespace(title_text=t["title_text"], title_mask=t["title_mask"], augmented_title_text=t["augmented_title_text"],
                                 augmented_title_mask=t["augmented_title_mask"], history_ids=t["history_ids"], history_mask=t["history_mask"],
                                 row_candidate=inp["candidate_ids"].reshape(-1), row_impression=np.repeat(np.arange(U), K))


def training_step(m, t, stock=False):
    """Appendix-B model.py:24-31 on the fixture's impressions, cross-entropy over 1 + 4 candidates with the clicked one first."""
    hid, cid = t["history_ids"], t["candidate_ids"]
    fn = m.forward_stock if stock else m
    logits = fn(t["title_text"][hid], t["title_mask"][hid], t["history_mask"], t["title_text"][cid], t["title_mask"][cid],
                t["augmented_title_text"][cid], t["augmented_title_mask"][cid])
    loss = torch.nn.functional.cross_entropy(logits, torch.zeros(logits.shape[0], dtype=torch.long, device=logits.device))
    loss.backward()
    return logits, loss


def check_training_step(fx, pre, m, logits, loss, rtol_out=1e-5):
    """Logits, loss and every gradient against an nrms_train_*.npz fixture at the training tolerance 2e-4.  The fixture's gradients are
    the reference's in fp64.  No absolute slack: an element is held relative to the larger of its own size and 5 % of its tensor's
    largest, so a gradient that is small as a whole is checked like any other."""
    close(logits, fx[f"{pre}_logits"], f"{pre} logits", rtol=rtol_out, atol=2e-6)
    close(loss, fx[f"{pre}_loss"], f"{pre} loss", rtol=2e-5, atol=1e-5)
    sub = {k[len(pre) + 1:]: v for k, v in fx.items() if k.startswith(pre + "_g")}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if "g_" + k in sub:
            close(p.grad, sub["g_" + k], f"{pre} grad {k}", rtol=2e-4, atol=0.0)
        else:
            check_grad_digest(sub, k, p.grad.detach().cpu().numpy(), 2e-4, f"{pre} grad ")


def reference_fp32_errors(fx, pre):
    """{parameter: relative error of the reference's own fp32 gradient against its fp64 one}, as stored when the fixture was minted."""
    return {k[len(pre) + 4:]: float(v) for k, v in fx.items() if k.startswith(pre + "_ge_")}
