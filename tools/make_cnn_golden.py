#!/usr/bin/env python
"""Mint the CNN news encoder's golden vectors (tests/golden/cnn_*.npz) from the reference's own modules.

    python tools/make_cnn_golden.py [REFERENCE_DIR]

Imports ``layers.Conv1D`` and ``layers.Attention`` from the reference tree (default: the directory oracle/make_golden.py uses) and
composes them exactly as ``newsEncoders.CNN.forward`` does (newsEncoders.py:41-54: embedding -> dropout -> Conv1D on the permuted
tensor -> dropout -> Attention with the title mask); ``NewsEncoder.__init__`` itself needs the data set's word-embedding pickle, so
the modules are built directly, as oracle/make_golden.py does for MSA.  Only data is written: seeds, shapes, a checksum of the
regenerated inputs, outputs, and gradients (whole when tiny, else the digest of tests/conftest.py).  One title per fixture is all
padding (its pooling is uniform, layers.py:111).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from digat_amd import synthetic  # noqa: E402
from oracle import make_golden as G  # noqa: E402  (save / checksum / grad_digest / T: the fixture conventions)

INFERENCE = {   # tag: (T, Lw, V, dm, Kc, att, method, window, seed)
    "cnn_tiny": (6, 8, 40, 20, 12, 12, "naive", 3, 81),
    "cnn_default": (72, 32, 500, 300, 400, 256, "naive", 3, 82),
    "cnn_w5": (72, 32, 500, 300, 400, 256, "naive", 5, 83),
    "cnn_group3": (72, 32, 500, 300, 396, 256, "group3", 3, 84),
}
TRAIN = {
    "cnn_train_tiny": (6, 8, 40, 20, 12, 12, "naive", 3, 85),
    "cnn_train_default": (72, 32, 500, 300, 400, 256, "naive", 3, 86),
    "cnn_train_group3": (72, 32, 500, 300, 396, 256, "group3", 3, 87),
}
METHODS = ("naive", "group3")


def modules(layers, state, dm, Kc, att, method, window, dtype=torch.float32):
    conv = layers.Conv1D(method, dm, Kc, window)
    attn = layers.Attention(Kc, att)
    conv.load_state_dict({k[len("conv."):]: G.T(v) for k, v in state.items() if k.startswith("conv.")})
    attn.load_state_dict({k[len("attention."):]: G.T(v) for k, v in state.items() if k.startswith("attention.")})
    return conv.to(dtype), attn.to(dtype)


def inputs(T_, Lw, V, seed):
    text, mask = synthetic.make_titles(T_, Lw, V, seed=seed + 1)
    text[2], mask[2] = 0, False                                                    # an empty (all-padding) title
    return text, mask


def main(reference):
    if not os.path.isdir(reference):
        raise SystemExit(f"{reference}: the reference tree is needed to mint fixtures")
    sys.path.insert(0, reference)
    import layers  # the reference's layers.py
    torch.manual_seed(0)
    for tag, (T_, Lw, V, dm, Kc, att, method, window, seed) in INFERENCE.items():
        state = synthetic.make_cnn_state(V, dm, Kc, att, method, window, seed=seed)
        text, mask = inputs(T_, Lw, V, seed)
        conv, attn = modules(layers, state, dm, Kc, att, method, window)
        conv.eval(); attn.eval()
        with torch.no_grad():
            w = torch.nn.functional.embedding(G.T(text), G.T(state["word_embedding.weight"]))       # newsEncoders.py:48 (dropout off)
            h = conv(w.permute(0, 2, 1)).permute(0, 2, 1)                                           # :50
            out = attn(h, mask=G.T(mask.astype(np.int64)))                                          # :52
        G.save(f"{tag}.npz", meta=np.array([T_, Lw, V, dm, Kc, att, METHODS.index(method), window]), seeds=np.array([seed, seed + 1]),
               input_checksum=G.checksum({"t": text, "m": mask}, state), out_news_representation=out.numpy())
    for tag, (T_, Lw, V, dm, Kc, att, method, window, seed) in TRAIN.items():
        state = synthetic.make_cnn_state(V, dm, Kc, att, method, window, seed=seed)
        text, mask = inputs(T_, Lw, V, seed)
        R = np.random.default_rng(seed + 2).standard_normal((T_, Kc)).astype(np.float32)
        conv, attn = modules(layers, state, dm, Kc, att, method, window)
        conv.train(); attn.train()
        emb = torch.nn.Embedding(V, dm)
        emb.weight.data.copy_(G.T(state["word_embedding.weight"]))
        w = emb(G.T(text))                                                                           # dropout 0
        h = conv(w.permute(0, 2, 1)).permute(0, 2, 1)
        out = attn(h, mask=G.T(mask.astype(np.int64)))
        loss = (out * G.T(R)).sum()
        loss.backward()
        named = [("word_embedding.weight", emb.weight)] + [("conv." + k, v) for k, v in conv.named_parameters()] \
            + [("attention." + k, v) for k, v in attn.named_parameters()]
        res = {"out_news_representation": out.detach().numpy(), "out_loss": loss.detach().numpy()}
        for k, v in named:
            if tag == "cnn_train_tiny":
                res["g_" + k] = v.grad.numpy()
            else:
                res.update(G.grad_digest(k, v.grad.numpy()))
        G.save(f"{tag}.npz", meta=np.array([T_, Lw, V, dm, Kc, att, METHODS.index(method), window]),
               seeds=np.array([seed, seed + 1, seed + 2]), input_checksum=G.checksum({"t": text, "m": mask, "r": R}, state), **res)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else G.REFERENCE)
