"""The NRMS and NRMS-SA baselines of the reference's second experiment (``Appendix-B/``) on the HIP kernels.

``NRMS_NewsEncoder``, ``SA_NRMS_NewsEncoder``, ``NRMS_UserEncoder`` and ``Model`` keep the reference's constructor arguments, method
signatures and ``state_dict`` keys (Appendix-B newsEncoders.py, userEncoders.py, model.py).  The word-embedding pickle is not
required: the table keeps its init, as in ``newsEncoders.py`` here.

On the GPU an encoder is one library call: ``digat_mhsa_fwd`` in inference, ``digat_mhsa_fwd_train`` / ``digat_mhsa_bwd`` under
autograd (``MhsaFused``) — the stacked Q|K|V projection, the key-masked attention (csrc/digat_mhsa.inc), the additive pooling.  The
news encoder hands over token ids and the word embedding, the user encoder dense rows (training) or news ids and the cached news
representations (dev scoring).  The SA gate is the news-graph context call ``digat_news_ctx_*`` on ``[orig ; aug]`` with node 0
masked out: it takes its query from node 0, attends over the unmasked nodes, gates and mixes (Appendix-B newsEncoders.py:100-102).
``recommend`` answers "which k news for this user": the logit is a plain inner product, so a shared candidate pool runs on the fused
inner-product + top-k kernel (``evaluate.dot_topk``: no [users, news] score matrix), and ``candidates_csr`` hands the lists to
``util.recommend`` for a DIGAT re-ranking.
Every class has a ``forward_stock`` on stock PyTorch: the CPU path and the yardstick.  There is no fall-back on the GPU: a shape the
library refuses raises.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .layers import ScaledDotProductAttention
from .newsEncoders import Attention, _embedding_grad
from .training import NewsCtxFused, RowLogits, _seed


class MultiHeadAttention(nn.Module):
    """Appendix-B layers.py:50-95: no output projection, K without bias, -1e9 over masked keys after the scale."""

    def __init__(self, h: int, d_model: int, len_q: int, len_k: int, d_k: int, d_v: int):
        super().__init__()
        self.h, self.d_model, self.len_q, self.len_k, self.d_k, self.d_v = h, d_model, len_q, len_k, d_k, d_v
        self.out_dim = h * d_v
        self.attention_scalar = math.sqrt(float(d_k))
        self.W_K = nn.Linear(d_model, h * d_k, bias=False)
        self.W_Q = nn.Linear(d_model, h * d_k, bias=True)
        self.W_V = nn.Linear(d_model, h * d_v, bias=True)

    def initialize(self):
        nn.init.xavier_uniform_(self.W_K.weight)
        nn.init.xavier_uniform_(self.W_Q.weight)
        nn.init.zeros_(self.W_Q.bias)
        nn.init.xavier_uniform_(self.W_V.weight)
        nn.init.zeros_(self.W_V.bias)

    def forward(self, Q, K, V, mask=None):
        B, Lq, Lk = Q.shape[0], Q.shape[1], K.shape[1]
        q = self.W_Q(Q).view(B, Lq, self.h, self.d_k).transpose(1, 2)
        k = self.W_K(K).view(B, Lk, self.h, self.d_k).transpose(1, 2)
        v = self.W_V(V).view(B, Lk, self.h, self.d_v).transpose(1, 2)
        a = q @ k.transpose(2, 3) / self.attention_scalar
        if mask is not None:
            a = a.masked_fill(mask.view(B, 1, 1, Lk) == 0, -1e9)
        return (F.softmax(a, dim=3) @ v).transpose(1, 2).reshape(B, Lq, self.out_dim)


def _stock_sdpa(att: ScaledDotProductAttention, feature, query):
    """Appendix-B layers.py:206-213 without a mask (the parameter container's own forward raises: the product path is the kernels')."""
    a = (att.K(feature) @ att.Q(query).unsqueeze(2)).squeeze(2) / att.attention_scalar
    return (F.softmax(a, dim=1).unsqueeze(1) @ feature).squeeze(1)


# ---- the library calls -------------------------------------------------------------------------------------------------------
def _mhsa_params(table, WQ, bQ, WK, WV, bV, A1, b1, a2, heads, dk, flags):
    P = _lib.MhsaParams(in_dim=WQ.shape[1], head_num=heads, head_dim=dk, attention_dim=A1.shape[0], flags=flags)
    for name, w in zip(("table", "W_Q", "b_Q", "W_K", "W_V", "b_V", "A1", "b1", "a2"), (table, WQ, bQ, WK, WV, bV, A1, b1, a2)):
        setattr(P, name, w.data_ptr())
    return P


def _weights(mha: MultiHeadAttention, att: Attention):
    return [mha.W_Q.weight, mha.W_Q.bias, mha.W_K.weight, mha.W_V.weight, mha.W_V.bias, att.affine1.weight, att.affine1.bias,
            att.affine2.weight]


class _InferenceBlock:
    """The parameter block of one encoder for inference, with the split images of the bf16x6 matrix-core GEMM path when
    ``hd % 80 == 0`` (else the fp32 path, as ``MSA._build_hip_params`` decides); rebuilt when a parameter has moved or been written."""

    def __init__(self, mha, att, flags):
        self.mha, self.att, self.flags, self.key, self.P, self.keep = mha, att, flags, None, None, None

    def params(self, table):
        ws = _weights(self.mha, self.att)
        key = tuple((w.data_ptr(), w._version) for w in ws)
        if key != self.key:
            L = _lib.lib()
            keep = [w.detach().float().contiguous() for w in ws]
            mha = self.mha
            dm, hd, natt, dev = mha.d_model, mha.h * mha.d_k, keep[5].shape[0], keep[0].device
            P = _mhsa_params(keep[0], *keep, mha.h, mha.d_k, self.flags)
            if hd % 80 == 0 and dm % 4 == 0 and dm >= 32:
                qkv = _lib.split_buffer(L.digat_msa_split_bytes(dm, mha.h, mha.d_k), dev)
                _lib.check(L.digat_split_msa_weights(keep[0].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), dm, hd, qkv.data_ptr(),
                                                     _lib.stream_ptr()), "digat_split_msa_weights")
                a1 = _lib.split_buffer(L.digat_split_weights_bytes(natt, hd), dev)
                _lib.check(L.digat_split_weights(keep[5].data_ptr(), natt, hd, a1.data_ptr(), _lib.GEMM_BF16X6, _lib.stream_ptr()),
                           "digat_split_weights")
                P.qkv_wsplit, P.a1_wsplit = qkv.data_ptr(), a1.data_ptr()
                keep += [qkv, a1]
            self.key, self.P, self.keep = key, P, keep
        self.P.table = table.data_ptr()
        return self.P


def mhsa_infer(block: _InferenceBlock, table, ids, mask):
    """``digat_mhsa_fwd``: table [V, in_dim] with ids [T, L] (any integer dtype), or ids None and table = dense rows [T L, in_dim];
    mask [T, L] -> [T, hd]."""
    L = _lib.lib()
    table = table.detach().float().contiguous()
    msk = (mask != 0).to(torch.uint8).contiguous()
    T, Ls = msk.shape
    idx = ids.reshape(T, Ls).to(torch.int32).contiguous() if ids is not None else None
    dev = _lib.require_device(table, msk)
    P = block.params(table)
    out = torch.empty((T, P.head_num * P.head_dim), dtype=torch.float32, device=dev)
    if T:
        dims = (T, Ls, P.in_dim, P.head_num, P.head_dim, P.attention_dim)
        nb = L.digat_mhsa_workspace_bytes(*dims)
        ws = _lib.workspace(nb, dev, "mhsa")
        _lib.check(L.digat_mhsa_fwd(P, _lib.ptr(idx), msk.data_ptr(), out.data_ptr(), T, Ls, ws.data_ptr(), nb, _lib.stream_ptr()),
                   "digat_mhsa_fwd")
    return out


class MhsaFused(torch.autograd.Function):
    """One encoder as one library call per direction (``digat_mhsa_fwd_train`` / ``digat_mhsa_bwd``).  ``ids`` int32 [T, L] with
    ``table`` [V, in_dim] (its gradient: ``digat_embedding_bwd``), or ``ids`` None with ``table`` = dense rows [T L, in_dim] (its
    gradient: the rows the library writes)."""

    @staticmethod
    def forward(ctx, ids, mask, table, WQ, bQ, WK, WV, bV, A1, b1, a2, heads, dk, p_in, p_ctx, flags):
        L = _lib.lib()
        ws_ = [w.detach().float().contiguous() for w in (table, WQ, bQ, WK, WV, bV, A1, b1, a2)]
        dev = _lib.require_device(mask, *ws_)
        T, Ls = mask.shape
        dims = (T, Ls, ws_[1].shape[1], heads, dk, ws_[6].shape[0])
        P = _mhsa_params(*ws_, heads, dk, flags)
        out = torch.empty((T, heads * dk), dtype=torch.float32, device=dev)
        nsave, nws = L.digat_mhsa_train_save_bytes(*dims), L.digat_mhsa_train_workspace_bytes(*dims)
        save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "mhsa_train")
        p_in, p_ctx = float(p_in), float(p_ctx)
        seed = _seed() if (p_in > 0 or p_ctx > 0) else 0
        if T:
            _lib.check(L.digat_mhsa_fwd_train(P, _lib.ptr(ids), mask.data_ptr(), out.data_ptr(), p_in, p_ctx, seed, T, Ls, save.data_ptr(),
                                              nsave, ws.data_ptr(), nws, _lib.stream_ptr()), "digat_mhsa_fwd_train")
        ctx.save_for_backward(mask, save, *ws_)
        ctx.ids, ctx.dims, ctx.p, ctx.seed, ctx.sizes, ctx.flags = ids, (heads, dk), (p_in, p_ctx), seed, (nsave, nws), flags
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        mask, save, *ws_ = ctx.saved_tensors
        table, WQ, bQ, WK, WV, bV, A1, b1, a2 = ws_
        ids = ctx.ids
        heads, dk = ctx.dims
        T, Ls = mask.shape
        dm, hd, att = WQ.shape[1], heads * dk, A1.shape[0]
        dev = mask.device
        if T == 0:                                # no sequence: every gradient is zero
            z = [torch.zeros_like(w) for w in ws_]
            return (None, None, z[0] if ctx.needs_input_grad[2] else None, *z[1:], None, None, None, None, None)
        dout = dout.float().contiguous()
        P = _mhsa_params(*ws_, heads, dk, ctx.flags)
        nsave, nws = ctx.sizes
        ws = _lib.workspace(nws, dev, "mhsa_train")
        f = dict(dtype=torch.float32, device=dev)
        ld = int(L.digat_msa_row_grad_ld(T, Ls, dm))
        row_grad = torch.empty((T * Ls, ld), **f)
        dW3 = torch.empty((3, hd, dm), **f)       # one buffer: the library writes its single [3 hd, dm] weight-gradient product in place
        dWQ, dWK, dWV = dW3[0], dW3[1], dW3[2]
        dbQ, dbV = torch.empty(hd, **f), torch.empty(hd, **f)
        dA1, db1, da2 = torch.empty((att, hd), **f), torch.empty(att, **f), torch.empty(att, **f)
        _lib.check(L.digat_mhsa_bwd(P, _lib.ptr(ids), mask.data_ptr(), dout.data_ptr(), ctx.p[0], ctx.p[1], ctx.seed, save.data_ptr(), nsave,
                                    row_grad.data_ptr(), ld, dWQ.data_ptr(), dbQ.data_ptr(), dWK.data_ptr(), dWV.data_ptr(), dbV.data_ptr(),
                                    dA1.data_ptr(), db1.data_ptr(), da2.data_ptr(), T, Ls, ws.data_ptr(), nws, _lib.stream_ptr()),
                   "digat_mhsa_bwd")
        dtable = None
        if ctx.needs_input_grad[2]:
            dtable = _embedding_grad(ids, row_grad, ld, table) if ids is not None else row_grad[:, :dm].reshape(table.shape)
        return None, None, dtable, dWQ, dbQ, dWK, dWV, dbV, dA1, db1, da2.view_as(a2), None, None, None, None, None


def _sa_gate_hip(orig, aug, sa_attention, sa_transformation, p_gate):
    """Appendix-B newsEncoders.py:100-102 as the news-graph context call: nodes [orig ; aug] with node 0 masked out of the attention."""
    T, A, hd = aug.shape
    X = torch.cat([orig.unsqueeze(1), aug], dim=1).contiguous()
    mask = torch.ones((T, 1 + A), dtype=torch.uint8, device=X.device)
    mask[:, 0] = 0
    Kc, Qc, bQc = sa_attention.K.weight, sa_attention.Q.weight, sa_attention.Q.bias
    Wg, bg = sa_transformation.weight, sa_transformation.bias
    if torch.is_grad_enabled():
        return NewsCtxFused.apply(X, mask, Kc, Qc, bQc, Wg, bg, p_gate)
    L = _lib.lib()
    ws_ = [w.detach().float().contiguous() for w in (Kc, Qc, bQc, Wg, bg)]
    out = torch.empty((T, hd), dtype=torch.float32, device=X.device)
    nb = L.digat_news_ctx_workspace_bytes(T, 1 + A, hd)
    ws = _lib.workspace(nb, X.device, "nrms_sa")
    _lib.check(L.digat_news_ctx_fwd(X.data_ptr(), mask.data_ptr(), *(w.data_ptr() for w in ws_), None, out.data_ptr(), T, 1 + A, hd,
                                    ws.data_ptr(), nb, _lib.stream_ptr()), "digat_news_ctx_fwd")
    return out


# ---- the reference's classes ---------------------------------------------------------------------------------------------------
class NewsEncoder(nn.Module):
    """Appendix-B newsEncoders.py:8-31 without the pickle."""

    def __init__(self, config):
        super().__init__()
        self.max_sentence_length = config.max_title_length
        self.word_embedding_dim = config.word_embedding_dim
        self.word_embedding = nn.Embedding(config.vocabulary_size, self.word_embedding_dim)
        self.dropout = nn.Dropout(p=config.dropout_rate)
        self.dropout_ = nn.Dropout(p=config.dropout_rate / 2)
        self.augmented_news_num = config.augmented_news_num

    def initialize(self):
        pass


class NRMS_NewsEncoder(NewsEncoder):
    """Appendix-B newsEncoders.py:34-58."""

    def __init__(self, config):
        super().__init__(config)
        self.news_embedding_dim = config.head_num * config.head_dim
        self.multiheadAttention = MultiHeadAttention(config.head_num, config.word_embedding_dim, config.max_title_length,
                                                     config.max_title_length, config.head_dim, config.head_dim)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        super().initialize()
        self.multiheadAttention.initialize()
        self.attention.initialize()

    def _block(self):
        if getattr(self, "_hip_block", None) is None:
            self._hip_block = _InferenceBlock(self.multiheadAttention, self.attention, 0)
        return self._hip_block

    def encode_titles(self, text, mask):
        """text / mask [T, Lw] -> [T, news_embedding_dim]: the HIP encoder on the GPU, the stock modules on the CPU."""
        if not text.is_cuda:
            return self._titles_stock(text, mask)
        if not torch.is_grad_enabled() and (not self.training or self.dropout.p == 0):
            return mhsa_infer(self._block(), self.word_embedding.weight, text, mask)
        mha = self.multiheadAttention
        p = float(self.dropout.p) if self.training else 0.0
        return MhsaFused.apply(text.to(torch.int32).contiguous(), (mask != 0).to(torch.uint8).contiguous(), self.word_embedding.weight,
                               *_weights(mha, self.attention), mha.h, mha.d_k, p, p, 0)

    def _titles_stock(self, text, mask):
        w = self.dropout(self.word_embedding(text.long()))
        c = self.dropout(self.multiheadAttention(w, w, w, mask))
        return self.attention(c, mask=mask)

    def forward(self, title_text, title_mask, augmented_news_title_text=None, augmented_news_title_mask=None):
        B, n = title_text.shape[:2]
        L = self.max_sentence_length
        return self.encode_titles(title_text.reshape(B * n, L), title_mask.reshape(B * n, L)).view(B, n, self.news_embedding_dim)

    def forward_stock(self, title_text, title_mask, augmented_news_title_text=None, augmented_news_title_mask=None):
        B, n = title_text.shape[:2]
        L = self.max_sentence_length
        return self._titles_stock(title_text.reshape(B * n, L), title_mask.reshape(B * n, L)).view(B, n, self.news_embedding_dim)


class SA_NRMS_NewsEncoder(NRMS_NewsEncoder):
    """Appendix-B newsEncoders.py:61-103: the same encoder over the augmented titles, attention of the original over them, a gate."""

    def __init__(self, config):
        super().__init__(config)
        d = self.news_embedding_dim
        self.SA_attention = ScaledDotProductAttention(d, d, d)
        self.SA_transformation = nn.Linear(2 * d, d, bias=True)

    def initialize(self):
        super().initialize()
        self.SA_attention.initialize()
        nn.init.xavier_uniform_(self.SA_transformation.weight)
        nn.init.zeros_(self.SA_transformation.bias)

    def sa_gate(self, orig, aug):
        """orig [T, hd], aug [T, A, hd] -> [T, hd] (newsEncoders.py:100-102)."""
        if orig.is_cuda:
            return _sa_gate_hip(orig, aug, self.SA_attention, self.SA_transformation, float(self.dropout_.p) if self.training else 0.0)
        return self.sa_gate_stock(orig, aug)

    def sa_gate_stock(self, orig, aug):
        g = _stock_sdpa(self.SA_attention, aug, orig)
        gate = torch.sigmoid(self.dropout_(self.SA_transformation(torch.cat([orig, g], dim=1))))
        return gate * orig + (1 - gate) * g

    def _forward(self, titles, gate, title_text, title_mask, aug_text, aug_mask):
        B, n = title_text.shape[:2]
        L, A, d = self.max_sentence_length, self.augmented_news_num, self.news_embedding_dim
        orig = titles(title_text.reshape(B * n, L), title_mask.reshape(B * n, L))
        if aug_text is not None:
            aug = titles(aug_text.reshape(B * n * A, L), aug_mask.reshape(B * n * A, L)).view(B * n, A, d)
            orig = gate(orig, aug)
        return orig.view(B, n, d)

    def forward(self, title_text, title_mask, augmented_news_title_text=None, augmented_news_title_mask=None):
        return self._forward(self.encode_titles, self.sa_gate, title_text, title_mask, augmented_news_title_text, augmented_news_title_mask)

    def forward_stock(self, title_text, title_mask, augmented_news_title_text=None, augmented_news_title_mask=None):
        return self._forward(self._titles_stock, self.sa_gate_stock, title_text, title_mask, augmented_news_title_text,
                             augmented_news_title_mask)


class UserEncoder(nn.Module):
    """Appendix-B userEncoders.py:8-31."""

    def __init__(self, news_encoder, config):
        super().__init__()
        self.news_embedding_dim = news_encoder.news_embedding_dim
        self.news_encoder = news_encoder
        self.max_history_num = config.max_history_num


class NRMS_UserEncoder(UserEncoder):
    """Appendix-B userEncoders.py:34-52: the history mask is the key mask, the pooling is unmasked."""

    def __init__(self, news_encoder, config):
        super().__init__(news_encoder, config)
        self.multiheadAttention = MultiHeadAttention(config.head_num, self.news_embedding_dim, config.max_history_num,
                                                     config.max_history_num, config.head_dim, config.head_dim)
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        self.multiheadAttention.initialize()
        self.attention.initialize()

    def _block(self):
        if getattr(self, "_hip_block", None) is None:
            self._hip_block = _InferenceBlock(self.multiheadAttention, self.attention, _lib.MHSA_POOL_UNMASKED)
        return self._hip_block

    def encode(self, history_embedding, user_history_mask):
        if not history_embedding.is_cuda:
            return self.encode_stock(history_embedding, user_history_mask)
        B, H, d = history_embedding.shape
        if not torch.is_grad_enabled():
            return mhsa_infer(self._block(), history_embedding.reshape(B * H, d), None, user_history_mask)
        mha = self.multiheadAttention
        return MhsaFused.apply(None, (user_history_mask != 0).to(torch.uint8).contiguous(), history_embedding.reshape(B * H, d),
                               *_weights(mha, self.attention), mha.h, mha.d_k, 0.0, 0.0, _lib.MHSA_POOL_UNMASKED)

    def encode_cached(self, news_embeddings, history_ids, user_history_mask):
        """Dev scoring: the histories are rows of the cached news representations, looked up by id inside the library."""
        if not news_embeddings.is_cuda:
            return self.encode_stock(news_embeddings[history_ids.long()], user_history_mask)
        return mhsa_infer(self._block(), news_embeddings, history_ids, user_history_mask)

    def encode_stock(self, history_embedding, user_history_mask):
        h = self.multiheadAttention(history_embedding, history_embedding, history_embedding, user_history_mask)
        return self.attention(h)

    def forward(self, user_title_text, user_title_mask, user_history_mask):
        return self.encode(self.news_encoder(user_title_text, user_title_mask), user_history_mask)

    def forward_stock(self, user_title_text, user_title_mask, user_history_mask):
        return self.encode_stock(self.news_encoder.forward_stock(user_title_text, user_title_mask), user_history_mask)


class Model(nn.Module):
    """Appendix-B model.py: the logit is <user, news>."""

    def __init__(self, config):
        super().__init__()
        if config.model == 'NRMS':
            self.news_encoder = NRMS_NewsEncoder(config)
        elif config.model == 'NRMS-SA':
            self.news_encoder = SA_NRMS_NewsEncoder(config)
        else:
            raise Exception(config.model + ' is not implemented')
        self.user_encoder = NRMS_UserEncoder(self.news_encoder, config)
        self.model_name = config.model
        self.news_embedding_dim = self.news_encoder.news_embedding_dim

    def initialize(self):
        self.news_encoder.initialize()
        self.user_encoder.initialize()

    def forward(self, user_title_text, user_title_mask, user_history_mask, news_title_text, news_title_mask,
                augmented_news_title_text=None, augmented_news_title_mask=None):
        if not news_title_text.is_cuda:
            return self.forward_stock(user_title_text, user_title_mask, user_history_mask, news_title_text, news_title_mask,
                                      augmented_news_title_text, augmented_news_title_mask)
        B, K = news_title_text.shape[:2]
        news = self.news_encoder(news_title_text, news_title_mask, augmented_news_title_text, augmented_news_title_mask)
        user = self.user_encoder(user_title_text, user_title_mask, user_history_mask)
        return row_logits(news.reshape(B * K, -1), user.unsqueeze(1).expand(B, K, -1).reshape(B * K, -1)).view(B, K)

    def forward_stock(self, user_title_text, user_title_mask, user_history_mask, news_title_text, news_title_mask,
                      augmented_news_title_text=None, augmented_news_title_mask=None):
        news = self.news_encoder.forward_stock(news_title_text, news_title_mask, augmented_news_title_text, augmented_news_title_mask)
        user = self.user_encoder.forward_stock(user_title_text, user_title_mask, user_history_mask)
        return (user.unsqueeze(1) * news).sum(dim=2)


def row_logits(news, user):
    """<news[r], user[r]> per row on the device (``digat_row_logits``), with autograd when gradients are enabled."""
    news, user = news.float().contiguous(), user.float().contiguous()
    if torch.is_grad_enabled() and (news.requires_grad or user.requires_grad):
        return RowLogits.apply(news, user)
    out = torch.empty(news.shape[0], dtype=torch.float32, device=news.device)
    if news.shape[0]:
        _lib.binding().row_logits(news, user, out)
    return out


def make_config(model='NRMS', vocabulary_size=1000, word_embedding_dim=300, head_num=20, head_dim=20, attention_dim=200, max_title_length=32,
                max_history_num=50, augmented_news_num=10, dropout_rate=0.2):
    """The fields of the reference's Config that these classes read, at the Appendix-B defaults."""
    return SimpleNamespace(**locals())


# ---- the dev run (Appendix-B util.py:10-72) ------------------------------------------------------------------------------------
def news_caches(model, title_text, title_mask, augmented_title_text, augmented_title_mask, batch_size=1024):
    """(plain, augmented) news representations [N, hd], built in batches.  NRMS ignores the augmented titles: one cache serves both.
    NRMS-SA encodes a batch's original titles once and gates them with their augmented titles (the reference encodes them twice,
    util.py:37-38: the same values)."""
    enc = model.news_encoder
    plain, aug = [], []
    sa = isinstance(enc, SA_NRMS_NewsEncoder)
    with torch.no_grad():
        for lo in range(0, title_text.shape[0], batch_size):
            sl = slice(lo, lo + batch_size)
            orig = enc.encode_titles(title_text[sl], title_mask[sl])
            plain.append(orig)
            if sa:
                at, am = augmented_title_text[sl], augmented_title_mask[sl]
                n, A, L = at.shape
                aug.append(enc.sa_gate(orig, enc.encode_titles(at.reshape(n * A, L), am.reshape(n * A, L)).view(n, A, -1)))
    plain = torch.cat(plain) if plain else title_text.new_zeros((0, enc.news_embedding_dim), dtype=torch.float32)
    return plain, (torch.cat(aug) if sa and aug else plain)


def compute_scores(model, dev, batch_size=1024, grouped=True, result_file=None, news_batch_size=None):
    """The dev run on a corpus-like object with ``title_text / title_mask`` [N, Lw], ``augmented_title_text / augmented_title_mask``
    [N, A, Lw], ``history_ids / history_mask`` [I, H] (one row per impression), ``row_candidate / row_impression`` [R]
    (impression-major) and optionally ``row_label`` [R]; tensors on the model's device, the row arrays on the host.
    Candidates are read from the augmented cache, histories from the plain one.  ``grouped``: each impression's user is encoded
    once and its representation gathered per row; else once per row, as the reference does — the same scores.
    ``news_batch_size``: titles per batch of the news caches, by default 4 x batch_size as in the reference (util.py:16).
    -> (scores [R] tensor, ranks int64 numpy [R], (auc, mrr, ndcg5, ndcg10) or None); ``result_file`` gets the rank file."""
    from . import evaluate
    model.eval()
    plain, aug = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask,
                             news_batch_size or 4 * batch_size)
    device = plain.device
    row_imp = np.asarray(dev.row_impression, dtype=np.int64)
    cand = torch.from_numpy(np.asarray(dev.row_candidate, dtype=np.int64)).to(device)
    imp = torch.from_numpy(row_imp).to(device)
    R = len(row_imp)
    ue = model.user_encoder
    scores = torch.empty(R, dtype=torch.float32, device=device)
    with torch.no_grad():
        if grouped:
            users = [ue.encode_cached(plain, dev.history_ids[lo:lo + batch_size], dev.history_mask[lo:lo + batch_size])
                     for lo in range(0, dev.history_ids.shape[0], batch_size)]
            users = torch.cat(users) if users else plain.new_zeros((0, plain.shape[1]))
        for lo in range(0, R, batch_size):
            sl = slice(lo, lo + batch_size)
            if grouped:
                u = users.index_select(0, imp[sl])
            else:
                u = ue.encode_cached(plain, dev.history_ids.index_select(0, imp[sl]), dev.history_mask.index_select(0, imp[sl]))
            c = aug.index_select(0, cand[sl])
            scores[sl] = row_logits(c, u) if device.type == "cuda" else (c * u).sum(dim=1)
    ranks, metrics = evaluate.ranks_metrics_file(scores, row_imp, getattr(dev, "row_label", None), result_file)
    return scores, ranks, metrics


# ---- retrieval: which k news of the corpus for this user -----------------------------------------------------------------------
def _histories(dev, users):
    """``users`` of ``recommend`` as ``(history_ids [G,H] int64, history_mask [G,H])`` on the device of ``dev.history_ids``: a 1-D
    integer array of impression indices of ``dev``, or a pair ``(history_ids, history_mask)`` of people who are no rows of it."""
    from . import util
    idx, hist, mask = util.recommend_user_arrays(users, int(dev.history_ids.shape[0]), int(dev.history_ids.shape[1]),
                                                 int(dev.title_text.shape[0]), dev.history_ids.device, ("history_ids", "history_mask"))
    if idx is None:
        return hist, mask
    return dev.history_ids.index_select(0, idx).to(torch.int64), dev.history_mask.index_select(0, idx)


def _encode_users(model, plain, hist, mask, batch_size):
    ue = model.user_encoder
    with torch.no_grad():
        out = [ue.encode_cached(plain, hist[lo:lo + batch_size], mask[lo:lo + batch_size]) for lo in range(0, hist.shape[0], batch_size)]
    return torch.cat(out) if out else plain.new_zeros((0, plain.shape[1]))


def user_vectors(model, dev, users, batch_size=1024):
    """The user representations [G, hd] of ``users`` (``_histories``: impression indices of ``dev`` or a ``(history_ids,
    history_mask)`` pair), encoded through ``encode_cached`` on the plain news cache in batches, in eval mode."""
    hist, mask = _histories(dev, users)
    model.eval()
    plain, _ = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)
    return _encode_users(model, plain, hist, mask, batch_size)


def recommend(model, dev, users, candidates=None, k=10, exclude_history=True, batch_size=1024, diversity=None, shortlist=None, category=None,
              max_per_category=0, calibration=None, calibration_target=None, alpha=0.01, index=None, refine=None, sample=None, seed=0,
              streams=None, rerank=None, exposure_cap=None):
    """For every user, which k news, in order: ``(news_ids [G,k] int64, scores [G,k] float32, count [G] int32)`` on the model's
    device.  Order: score descending, equal scores in candidate order; slots at or beyond ``count[g]`` hold id -1 and score -inf.

    ``dev`` is the corpus-like object of ``compute_scores``; candidates are read from the augmented cache, histories from the plain
    one, as there.  ``users``: impression indices of ``dev`` or ``(history_ids [G,H], history_mask [G,H])``.  ``candidates``: None =
    every news but row 0 (<PAD>); a 1-D id array = one pool for all users — ``evaluate.dot_topk``, the fused inner-product + top-k
    kernel, which never writes the [G, P] scores; ``(ids [R], start [G+1])`` = per-user lists (``util.recommend_candidates``) —
    gather, ``row_logits``, ``evaluate.topk_segments``.  ``exclude_history``: a news of the user's history (mask non-zero) is never
    returned, nor is row 0; False takes the candidates at their word.  On CPU tensors: stock PyTorch and ``topk_segments_host``.

    ``diversity`` in [0, 1] (None: off, the call above and nothing else): retrieval runs at ``k' = shortlist or min(128, 4 k)`` and
    ``util.diversify`` cuts every list to k by greedy maximal-marginal relevance with ``lam = 1 - diversity`` over the plain news
    cache; ``max_per_category`` q >= 1 lets at most q news of one ``category`` [N] (None: ``dev.news_category``) into a list.

    ``calibration`` in [0, 1] (None: off): retrieval runs at ``k' = shortlist or min(1024, 8 k)`` (``shortlist``'s kernels beyond
    128) and ``util.calibrate`` cuts every list to k with ``lam = 1 - calibration`` towards the category mix of the user's history
    (``evaluate.category_share`` under ``category``, None: ``dev.news_category``; at most 64 categories) or towards
    ``calibration_target`` [G, C]; ``alpha`` smooths the list's mix.  ``util.recommend`` has the details; ``calibration`` and
    ``diversity`` do not combine.

    ``index`` (``build_index``; None: the call above, bit for bit): a quantised first stage.  The users are encoded as always and
    quantised on the device, ``evaluate.qdot_shortlist`` (``qdot_topk`` up to 128) retrieves ``M = refine or min(1024, max(8 k, 64))``
    news per user on the int8 matrix cores from the shared pool, and ``evaluate.refine_lists`` re-scores those M in fp32 and cuts
    them to k: the scores returned are exact (``dot_scores``' bits), and wherever the exact top-k lies inside the quantised
    shortlist the result is the plain call's, bit for bit (``index_report`` measures how often that is).  Per-user candidate lists
    are refused.  ``diversity`` composes — its shortlist of k' comes from the indexed call —; ``calibration`` does not: its
    shortlist may be longer than the 128 entries ``refine_lists`` returns.

    ``sample`` — a temperature > 0 (None: off, the call as it was, bit for bit): retrieval runs at ``k' = shortlist or min(1024,
    8 k)`` and ``util.sample_lists`` draws one Plackett-Luce slate of k from ``softmax(score / sample)`` over that shortlist;
    ``seed`` and ``streams`` [G] name the draws (None: the impression indices where ``users`` are indices).  ``util.recommend`` has
    the details; ``sample`` does not combine with ``diversity``, ``calibration`` or ``index``.

    ``rerank=(diversity, calibration)`` (None: off, the call as it was, bit for bit): both at once in one objective — retrieval runs
    at ``k' = shortlist or min(1024, 8 k)`` and ``util.rerank`` cuts every list to k over the plain news cache (the vectors
    ``diversity`` uses) towards the category mix of the history or ``calibration_target``; ``shortlist``, ``category``,
    ``max_per_category`` and ``alpha`` compose.  ``util.recommend`` has the details; ``rerank`` does not combine with
    ``diversity``, ``calibration``, ``sample`` or ``index``.

    ``exposure_cap`` (None: off, the call as it was, bit for bit): an int c >= 0 — no news in more than c lists of THIS call — or an
    integer array [N] of capacities.  Retrieval runs once over all users at ``k' = shortlist or min(1024, 8 k)`` and
    ``util.cap_exposure`` cuts the lists to k together (a stable assignment, not the one of largest total score; the cap holds per
    call; a list whose shortlist runs out comes back short — name a deeper ``shortlist``).  ``util.recommend`` has the details;
    ``exposure_cap`` does not combine with ``diversity``, ``calibration``, ``rerank``, ``sample``, ``max_per_category`` or ``index``."""
    from . import util

    def select(wide, long_lists):
        if index is not None:
            return _retrieve_indexed(model, dev, users, candidates, wide, exclude_history, batch_size, index, refine, True)
        return _retrieve(model, dev, users, candidates, wide, exclude_history, batch_size, long_lists)

    def history():
        hist, mask = _histories(dev, users)
        return torch.where(mask != 0, hist, torch.zeros_like(hist))

    def own_refusals():
        if index is None and refine is not None:
            raise ValueError("refine belongs to an indexed call: name index (build_index)")
        if calibration is not None and index is not None:
            raise ValueError("calibration does not combine with index: its shortlist may exceed the 128 entries the re-score returns")
    plain = lambda: news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)[0]
    return util.recommend_dispatch(select, plain, history, k, getattr(dev, "news_category", None), util.user_streams(users), diversity,
                                   shortlist, category, max_per_category, calibration, calibration_target, alpha, sample, seed, streams, rerank,
                                   {"index": index, "refine": refine}, own_refusals, exposure_cap=exposure_cap,
                                   news_num=lambda: int(dev.title_text.shape[0]))


def _retrieve(model, dev, users, candidates, k, exclude_history, batch_size, long_lists):
    """``recommend`` without diversity (k <= 128: ``dot_topk`` / ``topk_segments``) or, with ``long_lists``, ``shortlist`` (k <= 1024:
    ``dot_shortlist`` / ``shortlist_segments``): the same caches, user vectors, skip rows and chunk loop."""
    from . import evaluate, util
    hist, mask = _histories(dev, users)
    G, N = int(hist.shape[0]), int(dev.title_text.shape[0])
    k = util.recommend_limits(k, int(hist.shape[1]) if exclude_history else 0, long_lists)
    if candidates is None:
        candidates = np.arange(1, N, dtype=np.int64)
    ids, start = util.recommend_candidates(candidates, G, N)
    model.eval()
    plain, aug = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)
    cuda = plain.device.type == "cuda"
    ids = ids.to(plain.device)
    user = _encode_users(model, plain, hist, mask, batch_size)
    skip = torch.where(mask != 0, hist, torch.zeros_like(hist)) if exclude_history else None
    if cuda and start is None:
        s, i, c = (evaluate.dot_shortlist if long_lists else evaluate.dot_topk)(user, aug, k, pool=ids, skip=skip)
        return i, s, c

    def score(g0, g1, row_user, row_cand):
        c, u = aug.index_select(0, row_cand), user.index_select(0, row_user)
        return row_logits(c, u) if cuda else (c * u).sum(dim=1)
    # on the CPU one chunk holds all pairs
    return util.recommend_select(G, k, ids, start, skip, util.RECOMMEND_MAX_ROWS if cuda else max(1, G * int(ids.shape[0])), score,
                                 long_lists=long_lists)


class RetrievalIndex:
    """What ``build_index`` returns: ``codes`` [N, dq] int8 and ``scales`` [N] float32 of the augmented news cache
    (``evaluate.quantize_rows``), ``vectors`` [N, hd] — that cache in fp32, for the re-score —, ``plain`` [N, hd] — the plain cache
    the user encoder reads (the same tensor for NRMS) — and ``news_num`` = N.  It is a snapshot of the model's weights."""

    def __init__(self, codes, scales, vectors, plain):
        self.codes, self.scales, self.vectors, self.plain, self.news_num = codes, scales, vectors, plain, int(vectors.shape[0])


def build_index(model, dev, batch_size=1024):
    """The quantised index of ``dev``'s news for ``recommend(index=)`` / ``shortlist(index=)``: the news caches, encoded once, and
    the augmented cache's per-row int8 codes and scales — 1 byte per channel beside the 4 of the fp32 cache.  Rebuild it when the
    model's weights change."""
    from . import evaluate
    model.eval()
    plain, aug = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)
    codes, scales = evaluate.quantize_rows(aug)
    return RetrievalIndex(codes, scales, aug, plain)


def _retrieve_indexed(model, dev, users, candidates, k, exclude_history, batch_size, index, refine, rescore):
    """``recommend(index=)`` (``rescore``: M quantised candidates, then the exact k) or ``shortlist(index=)`` (the k quantised lists
    themselves): ``_retrieve``'s users, pool and skip rows on ``index``'s caches and codes."""
    from . import evaluate, util
    if not isinstance(index, RetrievalIndex):
        raise ValueError("index must come from build_index")
    hist, mask = _histories(dev, users)
    G, N = int(hist.shape[0]), int(dev.title_text.shape[0])
    if index.news_num != N:
        raise ValueError(f"the index holds {index.news_num} news, this corpus {N}: rebuild it (build_index)")
    k = util.recommend_limits(k, int(hist.shape[1]) if exclude_history else 0, not rescore)
    if rescore:
        M = int(refine) if refine else min(evaluate.SHORTLIST_MAX_K, max(8 * k, 64))
        if not k <= M <= evaluate.SHORTLIST_MAX_K:
            raise ValueError(f"refine must lie in [k, {evaluate.SHORTLIST_MAX_K}] = [{k}, {evaluate.SHORTLIST_MAX_K}], got {refine}")
    elif refine is not None:
        raise ValueError("refine belongs to recommend: shortlist returns the quantised lists themselves")
    else:
        M = k
    if candidates is None:
        candidates = np.arange(1, N, dtype=np.int64)
    ids, start = util.recommend_candidates(candidates, G, N)
    if start is not None:
        raise ValueError("an index retrieves from one pool shared by all users: per-user candidate lists go through the call without index=")
    model.eval()
    device = index.vectors.device
    pool = ids.to(device)
    user = _encode_users(model, index.plain, hist, mask, batch_size)
    skip = torch.where(mask != 0, hist, torch.zeros_like(hist)) if exclude_history else None
    qu, su = evaluate.quantize_rows(user)
    if M <= evaluate.TOPK_MAX_K:
        s, i, c = evaluate.qdot_topk(qu, su, index.codes, index.scales, M, pool=pool, skip=skip)
    else:
        s, i, c = evaluate.qdot_shortlist(qu, su, index.codes, index.scales, M, pool=pool, skip=skip)
    if not rescore:
        return i, s, c
    # exact ties go by pool position, as in the plain call: hand the lists to the re-score in pool order
    where = torch.full((N + 1,), int(pool.shape[0]), dtype=torch.int64, device=device)
    where[pool.flip(0)] = torch.arange(int(pool.shape[0]) - 1, -1, -1, dtype=torch.int64, device=device)
    order = torch.argsort(where[torch.where(i >= 0, i, torch.full_like(i, N))], dim=1, stable=True)
    s, i, c = evaluate.refine_lists(user, index.vectors, torch.gather(i, 1, order), c, k)
    return i, s, c


def index_report(model, dev, users, k=10, ms=(32, 64, 128, 256), batch_size=1024, index=None, replicates=2000, seed=0):
    """What a quantised first stage of length M loses, per M of ``ms``: ``containment`` — the share of users whose exact top-k
    (``recommend``) lies wholly inside the quantised shortlist (``shortlist(index=)``), where ``recommend(index=, refine=M)`` returns
    the exact lists bit for bit — and ``agreement`` — ``teacher_agreement@k`` of the shortlist with the exact top-k as the teacher,
    the mean share of the exact top-k that the shortlist holds.  Both come with ``evaluate.metric_intervals`` over users.  Returns
    one dict per M: ``{"m": M, "containment": .., "agreement": .., "intervals": {...}}``.  ``index`` None: ``build_index`` here."""
    from . import evaluate
    index = build_index(model, dev, batch_size) if index is None else index
    t_ids, _, t_cnt = recommend(model, dev, users, k=k, batch_size=batch_size)
    rows = []
    for M in ms:
        s_ids, _, s_cnt = shortlist(model, dev, users, m=max(int(M), 1), batch_size=batch_size, index=index)
        agree = teacher_agreement(s_ids, s_cnt, t_ids, t_cnt, ks=(int(k),))["per_user"][:, 0]
        # the teacher's list is never longer than its user's elements, so a full share is containment (an empty list is contained)
        inside = np.where(_host_array(t_cnt) > 0, agree >= 1.0, True).astype(np.float64)
        per_user = np.stack([inside, agree], axis=1)
        iv = evaluate.metric_intervals(per_user, names=["containment", "agreement"], replicates=replicates, seed=seed)
        rows.append({"m": int(M), "containment": float(inside.mean()) if len(inside) else float("nan"),
                     "agreement": float(agree.mean()) if len(agree) else float("nan"), "intervals": iv})
    return rows


def shortlist(model, dev, users, candidates=None, m=512, exclude_history=True, batch_size=1024, index=None):
    """``recommend`` for the retrieval stage in front of a re-rank: for every user the m <= ``evaluate.SHORTLIST_MAX_K`` = 1024 best
    news, in order — ``(news_ids [G,m] int64, scores [G,m] float32, count [G] int32)`` — where ``recommend`` stops at 128.  ``dev``,
    ``users``, ``candidates``, ``exclude_history`` and ``batch_size`` are ``recommend``'s, and so are the caches, the user vectors,
    the skip rows, the order and the fill; for ``m <= 128`` the lists are ``recommend``'s, bit for bit.  A shared pool goes through
    ``evaluate.dot_shortlist`` (scores stored a slab of users at a time, then selected), per-user lists through gather,
    ``row_logits`` and ``evaluate.shortlist_segments``; on CPU tensors: stock PyTorch and ``shortlist_segments_host``.  How long the
    list must be: ``retrieval_metrics`` and ``evaluate.shortlist_for``; ``candidates_csr`` turns the result into the per-user
    lists ``util.recommend`` re-ranks.

    ``index`` (``build_index``; None: the call above, bit for bit): the lists come from ``evaluate.qdot_shortlist`` (``qdot_topk`` up
    to 128) on the int8 codes, and both their order and their SCORES are the quantised ones — ``evaluate.qdot_scores``' bits, within
    ``evaluate.qdot_bound`` of the real products —, not ``dot_scores``'.  A shared pool only."""
    if index is not None:
        return _retrieve_indexed(model, dev, users, candidates, m, exclude_history, batch_size, index, None, False)
    return _retrieve(model, dev, users, candidates, m, exclude_history, batch_size, True)


def recommend_report(model, dev, users, candidates=None, k=10, diversities=(0.0, 0.1, 0.3, 0.5), shortlist=None, category=None,
                     max_per_category=0, targets=None, exclude_history=True, batch_size=1024, return_lists=False):
    """``util.recommend_report`` on NRMS's own retrieval: one ``recommend`` at the shortlist's width, then every diversity's lists
    from it — bit for bit the lists ``recommend(..., diversity=f)`` returns — and their quality, one dict per diversity
    (``util.quality_report``).  The maximal-marginal-relevance stage keeps the vectors it uses in ``recommend``, the plain news
    cache; the QUALITY is always measured on ``util.unit_rows`` of those vectors, so ``ild`` and ``max_sim`` are cosine figures
    for both models whatever the cache's norms.  ``candidates`` None: every news but row 0, which is then the coverage pool too.
    ``targets = (target_ids [T], target_start [G+1])`` (``_clicked_targets`` reads a labelled corpus's) adds ``recall@k``,
    ``user_recall@k`` and ``mrr``.  The category figures go by ``category``, else ``dev.news_category`` where there is one."""
    from . import util
    N = int(dev.title_text.shape[0])
    select = lambda wide, long_lists: _retrieve(model, dev, users, candidates, wide, exclude_history, batch_size, long_lists)
    plain = functools.lru_cache(maxsize=None)(
        lambda: news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)[0])
    pool = np.arange(1, N, dtype=np.int64) if candidates is None else util.candidate_pool(candidates)
    return util.quality_report(select, plain, lambda: util.unit_rows(plain()), k, diversities, shortlist, category, max_per_category,
                               getattr(dev, "news_category", None), pool, targets, return_lists)


def _clicked_targets(dev, users):
    """``(impression indices [G], target_ids [T], target_start [G+1])`` from the rows of ``dev`` with ``row_label == 1``: every
    user's clicked candidates in row order.  ``users`` None: every impression that has a clicked row, ascending."""
    for name in ("row_candidate", "row_impression", "row_label"):
        if getattr(dev, name, None) is None:
            raise ValueError(f"the clicked targets come from dev.{name}, which this corpus does not carry: pass targets=(target_ids, target_start)")
    cand = np.asarray(dev.row_candidate, dtype=np.int64)
    imp = np.asarray(dev.row_impression, dtype=np.int64)
    label = np.asarray(dev.row_label)
    if not (cand.shape == imp.shape == label.shape and cand.ndim == 1):
        raise ValueError("row_candidate, row_impression and row_label must be 1-D arrays of one length")
    I = int(dev.history_ids.shape[0])
    if imp.size and (int(imp.min()) < 0 or int(imp.max()) >= I):
        raise ValueError(f"row_impression must lie in [0, {I})")
    rows = np.flatnonzero(label == 1)
    rows = rows[np.argsort(imp[rows], kind="stable")]               # impression-major already; any other order keeps rows in order per user
    per = np.bincount(imp[rows], minlength=I)
    first = np.r_[0, np.cumsum(per)]
    idx = np.flatnonzero(per > 0) if users is None else np.asarray(users.cpu() if torch.is_tensor(users) else users)
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise ValueError("the clicked targets belong to impressions: users must be a 1-D integer array of impression indices (or pass targets)")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= I):
        raise ValueError(f"impression indices must lie in [0, {I})")
    idx = idx.astype(np.int64)
    n = per[idx]
    start = np.r_[0, np.cumsum(n)].astype(np.int64)
    take = np.repeat(first[idx] - start[:-1], n) + np.arange(int(start[-1]), dtype=np.int64)
    return idx, cand[rows[take]], start


def retrieval_metrics(model, dev, users=None, targets=None, candidates=None, ks=(10, 50, 100, 128), exclude_history=True, batch_size=1024,
                      intervals=None, level=0.95, seed=0):
    """Full-catalogue retrieval metrics of the first stage: where in a user's whole ordered pool the target news stand — how long
    ``recommend``'s shortlist must be for a clicked news to survive into a re-rank (``evaluate.shortlist_for`` on the returned
    ranks).  Returns ``evaluate.rank_metrics``' dict plus ``rank`` [T] int32 (0-based, -1: not ranked), ``target_start`` [G+1] and
    ``target_ids`` [T], numpy arrays.

    ``dev``, ``exclude_history`` and ``batch_size`` are ``recommend``'s: candidates are read from the augmented cache, histories
    from the plain one, a news of the user's history (mask non-zero) is no element, nor is row 0.  ``users``: impression indices of
    ``dev`` (or a ``(history_ids, history_mask)`` pair together with explicit targets); None = every impression with a clicked row.
    ``targets``: None = every user's clicked candidates — ``dev.row_candidate`` where ``dev.row_label == 1`` —, else ``(target_ids
    [T], target_start [G+1])``.  ``candidates``: None = every news but row 0, or one 1-D pool shared by all users; per-user lists
    have no whole-pool rank — score such lists with ``evaluate.list_ranks``.  A target takes the first pool position of its id; a
    target that is not in the pool, is row 0, or — under ``exclude_history`` — is in its user's history is NOT RANKED (-1): it
    counts as a miss in every recall, and ``not_ranked`` says how many there are.

    On CUDA tensors the ranks come from ``evaluate.dot_rank`` (``digat_dot_rank``: no [users, news] score matrix); on CPU tensors
    from the stock product and ``evaluate.dot_rank_host``.

    ``intervals``: None returns exactly the dict above; an integer B adds ``"intervals"`` — ``evaluate.rank_metrics_intervals``'
    percentile intervals (``level``, ``seed``) of every ``recall@k``, ``user_recall@k`` and ``mrr`` from B bootstrap replicates over
    the users with a target, resampled on the GPU for CUDA tensors; ``median_rank`` has none."""
    from . import evaluate, util
    N = int(dev.title_text.shape[0])
    if targets is None:
        users, target_ids, target_start = _clicked_targets(dev, users)
    else:
        if users is None:
            raise ValueError("explicit targets need users: the impressions (or histories) target_start refers to")
        if not (isinstance(targets, (tuple, list)) and len(targets) == 2):
            raise ValueError("targets must be None or a pair (target_ids [T], target_start [G+1])")
        target_ids = np.asarray(targets[0].cpu() if torch.is_tensor(targets[0]) else targets[0])
        if target_ids.ndim != 1 or (target_ids.size and target_ids.dtype.kind not in "iu"):
            raise ValueError("target_ids must be a 1-D integer array of news ids")
        target_ids, target_start = target_ids.astype(np.int64), targets[1]
    hist, mask = _histories(dev, users)
    G = int(hist.shape[0])
    target_start = evaluate._check_target_start(target_start, G, len(target_ids))
    if target_ids.size and (int(target_ids.min()) < 0 or int(target_ids.max()) >= N):
        raise ValueError(f"target ids must lie in [0, {N})")
    util.recommend_limits(1, int(hist.shape[1]) if exclude_history else 0)
    if candidates is None:
        candidates = np.arange(1, N, dtype=np.int64)
    ids, start = util.recommend_candidates(candidates, G, N)
    if start is not None:
        raise ValueError("retrieval_metrics ranks targets in one pool shared by all users; per-user candidate lists have no such rank: "
                         "score them with evaluate.list_ranks on the lists recommend returns")
    # every target's first position in the pool, on the host; -1: not in it
    pool = ids.cpu().numpy()
    order = np.argsort(pool, kind="stable")
    at = np.searchsorted(pool[order], target_ids, side="left")
    inside = at < len(pool)
    inside[inside] = pool[order[at[inside]]] == target_ids[inside]
    target_pos = np.where(inside, order[np.minimum(at, max(len(pool) - 1, 0))] if len(pool) else -1, -1).astype(np.int64)
    model.eval()
    plain, aug = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)
    ids = ids.to(plain.device)
    user = _encode_users(model, plain, hist, mask, batch_size)
    skip = torch.where(mask != 0, hist, torch.zeros_like(hist)) if exclude_history else None
    if plain.device.type == "cuda":
        rank = evaluate.dot_rank(user, aug, target_pos, target_start, pool=ids, skip=skip)[0].cpu().numpy()
    else:
        rank = np.full(len(target_ids), -1, dtype=np.int32)
        rows = aug.index_select(0, ids)
        P = int(ids.shape[0])
        for g0 in range(0, G, max(1, int(batch_size))):
            g1 = min(G, g0 + max(1, int(batch_size)))
            t0, t1 = int(target_start[g0]), int(target_start[g1])
            if t0 == t1:
                continue
            S = (rows.repeat(g1 - g0, 1) * user[g0:g1].repeat_interleave(P, dim=0)).sum(dim=1).view(g1 - g0, P)
            rank[t0:t1] = evaluate.dot_rank_host(S.numpy(), target_pos[t0:t1], target_start[g0:g1 + 1] - t0, pool=pool,
                                                 skip=None if skip is None else skip[g0:g1].numpy(), news_num=N)
    out = evaluate.rank_metrics(rank, target_start, ks)
    out.update(rank=rank, target_start=target_start, target_ids=target_ids)
    if intervals is not None:
        out["intervals"] = evaluate.rank_metrics_intervals(rank, target_start, ks, replicates=intervals, level=level, seed=seed,
                                                           device=plain.device if plain.device.type == "cuda" else None)
    return out


def _first_positions(pool, N):
    """[N] int64: the first position of every news id in ``pool``, -1 for an id that is not in it."""
    where = np.full(N, -1, dtype=np.int64)
    where[pool[::-1]] = np.arange(len(pool) - 1, -1, -1, dtype=np.int64)
    return where


def retrieval_loss(model, dev, users=None, targets=None, candidates=None, exclude_history=True, batch_size=1024, scale=1.0):
    """The quantity ``fit_retriever`` minimises, measured as ``retrieval_metrics`` measures ranks: for every target its full-pool
    softmax loss ``logsumexp(scale * <user, news>) - scale * <user, target>`` over the user's elements, in eval mode under
    ``no_grad``.  ``dev``, ``users``, ``targets``, ``candidates`` (None or ONE shared 1-D pool), ``exclude_history`` and
    ``batch_size`` are ``retrieval_metrics``'; a target that has no rank there has no loss here.  Returns ``{"nll": the mean loss
    over the ranked targets (NaN without one), "not_ranked", "targets", "users": those with a target, "loss" [T], "lse" [G]}`` —
    numpy float64 arrays, ``loss`` 0 where the target is not ranked.

    On CUDA tensors ``evaluate.pool_softmax`` (``digat_pool_softmax_fwd``: no [users, news] score matrix); on CPU tensors the stock
    product per batch of users and ``evaluate.pool_softmax_host``."""
    from . import evaluate, util
    N = int(dev.title_text.shape[0])
    if targets is None:
        users, target_ids, target_start = _clicked_targets(dev, users)
    else:
        if users is None:
            raise ValueError("explicit targets need users: the impressions (or histories) target_start refers to")
        if not (isinstance(targets, (tuple, list)) and len(targets) == 2):
            raise ValueError("targets must be None or a pair (target_ids [T], target_start [G+1])")
        target_ids = np.asarray(targets[0].cpu() if torch.is_tensor(targets[0]) else targets[0])
        if target_ids.ndim != 1 or (target_ids.size and target_ids.dtype.kind not in "iu"):
            raise ValueError("target_ids must be a 1-D integer array of news ids")
        target_ids, target_start = target_ids.astype(np.int64), targets[1]
    hist, mask = _histories(dev, users)
    G = int(hist.shape[0])
    target_start = evaluate._check_target_start(target_start, G, len(target_ids))
    if target_ids.size and (int(target_ids.min()) < 0 or int(target_ids.max()) >= N):
        raise ValueError(f"target ids must lie in [0, {N})")
    util.recommend_limits(1, int(hist.shape[1]) if exclude_history else 0)
    ids, start = util.recommend_candidates(np.arange(1, N, dtype=np.int64) if candidates is None else candidates, G, N)
    if start is not None:
        raise ValueError("retrieval_loss takes the softmax over one pool shared by all users, not over per-user candidate lists")
    pool = ids.cpu().numpy()
    target_pos = _first_positions(pool, N)[target_ids]
    model.eval()
    plain, aug = news_caches(model, dev.title_text, dev.title_mask, dev.augmented_title_text, dev.augmented_title_mask, 4 * batch_size)
    ids = ids.to(plain.device)
    user = _encode_users(model, plain, hist, mask, batch_size)
    skip = torch.where(mask != 0, hist, torch.zeros_like(hist)) if exclude_history else None
    if plain.device.type == "cuda":
        with torch.no_grad():
            loss, lse, score = evaluate.pool_softmax(user, aug, target_pos, target_start, pool=ids, skip=skip, scale=scale)
        loss, lse, ranked = loss.double().cpu().numpy(), lse.double().cpu().numpy(), ~torch.isnan(score).cpu().numpy()
    else:
        loss, lse, ranked = np.zeros(len(target_ids)), np.zeros(G), np.zeros(len(target_ids), dtype=bool)
        rows = aug.index_select(0, ids)
        P = int(ids.shape[0])
        step = max(1, int(batch_size))
        for g0 in range(0, G, step):
            g1 = min(G, g0 + step)
            t0, t1 = int(target_start[g0]), int(target_start[g1])
            S = (rows.repeat(g1 - g0, 1) * user[g0:g1].repeat_interleave(P, dim=0)).sum(dim=1).view(g1 - g0, P)
            loss[t0:t1], lse[g0:g1], ranked[t0:t1] = evaluate.pool_softmax_host(
                S.numpy(), target_pos[t0:t1], target_start[g0:g1 + 1] - t0, pool=pool, skip=None if skip is None else skip[g0:g1].numpy(),
                news_num=N, scale=scale)
    return {"nll": float(loss[ranked].mean()) if ranked.any() else float("nan"), "not_ranked": int((~ranked).sum()),
            "targets": len(target_ids), "users": int((np.diff(target_start) > 0).sum()), "loss": loss, "lse": lse}


def retrieval_step(model, train, users, pool=None, exclude_history=True, scale=1.0):
    """One training step's loss for the first stage, with its graph: the full-pool softmax loss of the clicked candidates of
    ``users`` (impression indices of ``train``; ``_clicked_targets``), summed over the ranked targets and divided by their number
    (by 1 when there is none).  ``pool``: a 1-D array of news ids (None: every news but row 0).  The pool's titles go through
    ``model.news_encoder`` WITH gradients — the augmented titles too for NRMS-SA, as in ``Model.forward`` — into a compact [P, d]
    table, the users' histories through ``model.user_encoder`` on their title texts; history ids and targets are mapped to pool
    POSITIONS (-1: not in the pool), so the skip rows and the targets speak in positions and no [N, d] table is built.  A target
    outside the pool or — under ``exclude_history`` — inside its user's history is not ranked and carries no loss.  The model's
    mode (dropout) is the caller's.  On CUDA tensors the loss is ``evaluate.pool_softmax`` on the HIP encoders; on CPU tensors
    ``forward_stock`` and the stock composition."""
    from . import evaluate
    N, H = int(train.title_text.shape[0]), int(train.history_ids.shape[1])
    device = train.title_text.device
    idx, target_ids, target_start = _clicked_targets(train, users)
    pl = np.arange(1, N, dtype=np.int64) if pool is None else np.asarray(pool.cpu() if torch.is_tensor(pool) else pool)
    if pl.ndim != 1 or (pl.size and pl.dtype.kind not in "iu"):
        raise ValueError("pool must be a 1-D integer array of news ids")
    pl = pl.astype(np.int64)
    if pl.size and (int(pl.min()) < 0 or int(pl.max()) >= N):
        raise ValueError(f"pool ids must lie in [0, {N})")
    if exclude_history and H > evaluate.TOPK_MAX_SKIP:
        raise ValueError(f"exclude_history takes histories of at most {evaluate.TOPK_MAX_SKIP} news, got {H}")
    where = _first_positions(pl, N)
    ids = torch.from_numpy(pl).to(device)
    enc, ue = model.news_encoder, model.user_encoder
    cuda = device.type == "cuda"
    sa = isinstance(enc, SA_NRMS_NewsEncoder)
    table = (enc if cuda else enc.forward_stock)(
        train.title_text.index_select(0, ids)[None], train.title_mask.index_select(0, ids)[None],
        train.augmented_title_text.index_select(0, ids)[None] if sa else None,
        train.augmented_title_mask.index_select(0, ids)[None] if sa else None)[0]                       # [P, d]
    at = torch.from_numpy(idx).to(device)
    hist, mask = train.history_ids.index_select(0, at).to(torch.int64), train.history_mask.index_select(0, at)
    user = (ue if cuda else ue.forward_stock)(train.title_text[hist], train.title_mask[hist], mask)    # [G, d]
    skip = None
    if exclude_history:
        skip = torch.where(mask != 0, torch.from_numpy(where).to(device)[hist], torch.full_like(hist, -1))
    loss, _, score = evaluate.pool_softmax(user, table, where[target_ids], target_start, skip=skip, scale=scale)
    return loss.sum() / (~torch.isnan(score)).sum().clamp(min=1)


def _retriever_optimizer(model, lr, optimizer=None):
    """``optimizer``, or the one ``Trainer`` builds: Adam(``lr``) over ``trainer.parameter_groups``, ``optim.ClipAdam`` on the GPU."""
    if optimizer is not None:
        return optimizer
    from .trainer import parameter_groups
    groups = parameter_groups(model, 0.0)
    if all(p.is_cuda and p.dtype == torch.float32 for g in groups for p in g["params"]):
        from .optim import ClipAdam
        return ClipAdam(groups, lr=lr)
    return torch.optim.Adam(groups, lr=lr)


def fit_retriever(model, train, steps, batch_users=64, pool_size=None, lr=1e-4, seed=0, exclude_history=True, scale=1.0, optimizer=None):
    """Train ``model`` for retrieval: ``steps`` times one ``retrieval_step`` on a seeded draw of ``batch_users`` impressions of
    ``train`` that have a click (without replacement inside a step; all of them when there are fewer), one backward and one
    optimizer step, in train mode.  The pool is every news but row 0 (``pool_size`` None), or the sorted union of the batch's targets
    and ``pool_size`` uniformly drawn ids — never row 0.  ``optimizer``: None = the one ``Trainer`` builds — Adam(``lr``) over
    ``trainer.parameter_groups``, ``optim.ClipAdam`` on the GPU — and its state lives for this call only.  Returns the per-step
    losses as Python floats.  The draws depend on ``seed`` and the corpus alone, so CPU tensors see the same steps — through
    ``forward_stock`` and the stock composition."""
    N = int(train.title_text.shape[0])
    clicked, _, _ = _clicked_targets(train, None)
    if len(clicked) == 0:
        raise ValueError("no impression of this corpus has a clicked row: nothing to train on")
    if N < 2:
        raise ValueError("the corpus holds no news but row 0")
    optimizer = _retriever_optimizer(model, lr, optimizer)
    rng = np.random.default_rng(seed)
    model.train()
    losses = []
    for _ in range(int(steps)):
        batch = np.sort(rng.choice(clicked, size=min(int(batch_users), len(clicked)), replace=False))
        pool = None
        if pool_size is not None:
            _, target_ids, _ = _clicked_targets(train, batch)
            drawn = rng.integers(1, N, size=int(pool_size), dtype=np.int64)
            pool = np.union1d(target_ids[target_ids > 0], drawn)
        optimizer.zero_grad()
        loss = retrieval_step(model, train, batch, pool=pool, exclude_history=exclude_history, scale=scale)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return losses


# ---- listwise distillation: teach the first stage what the second stage ranks high ----------------------------------------------
def _host_array(x):
    return np.asarray(x.cpu() if torch.is_tensor(x) else x)


def _check_lists(users, ids, teacher, count, rows):
    """``(users [U] int64, ids [U,M] int64, teacher [U,M] float32, count [U] int64)`` as host arrays, checked."""
    from . import evaluate
    users, ids, teacher = _host_array(users), _host_array(ids), _host_array(teacher)
    if users.ndim != 1 or users.dtype.kind not in "iu":
        raise ValueError("users must be a 1-D integer array of impression indices")
    if users.size and (int(users.min()) < 0 or int(users.max()) >= rows):
        raise ValueError(f"impression indices must lie in [0, {rows})")
    U = len(users)
    if ids.ndim != 2 or ids.shape[0] != U or ids.dtype.kind not in "iu":
        raise ValueError(f"ids must be an integer array [users = {U}, M], got {ids.shape} {ids.dtype}")
    M = ids.shape[1]
    if not 1 <= M <= evaluate.SHORTLIST_MAX_K:
        raise ValueError(f"a list holds between 1 and SHORTLIST_MAX_K = {evaluate.SHORTLIST_MAX_K} slots, got M = {M}")
    if teacher.shape != ids.shape or teacher.dtype.kind != "f":
        raise ValueError(f"teacher must be a floating-point array with one value per slot {ids.shape}, got {teacher.shape} {teacher.dtype}")
    count = np.full(U, M, dtype=np.int64) if count is None else _host_array(count)
    if count.shape != (U,) or count.dtype.kind not in "iu":
        raise ValueError(f"count must be an integer array with one entry per list ({U}), got {count.shape} {count.dtype}")
    return users.astype(np.int64), ids.astype(np.int64), teacher.astype(np.float32), count.astype(np.int64)


def _list_front(model, train, idx, ids, count):
    """The front half of a step over per-user lists (``distil_step``, ``rank_step``), on checked host arrays: the distinct ids of the
    batch's lists form a compact pool whose titles go through ``model.news_encoder`` WITH gradients — the augmented titles too for
    NRMS-SA — into a [P, d] table; histories go through ``model.user_encoder`` on their title texts; list ids are mapped to pool
    positions.  Returns ``(user [G, d], table [P, d], pos [G, M] int64 (-1: no element), count [G] int32, elem [G, M] numpy bool)``."""
    N = int(train.title_text.shape[0])
    device = train.title_text.device
    M = ids.shape[1]
    elem = (np.arange(M)[None, :] < np.clip(count, 0, M)[:, None]) & (ids >= 0) & (ids < N)
    pl = np.unique(ids[elem])
    where = np.full(N, -1, dtype=np.int64)
    where[pl] = np.arange(len(pl), dtype=np.int64)
    pos = np.where(elem, where[np.where(elem, ids, 0)], -1)
    if len(pl) == 0:
        pl = np.zeros(1, dtype=np.int64)                             # no list names a news: one row nobody points at keeps the graph
    pool = torch.from_numpy(pl).to(device)
    enc, ue = model.news_encoder, model.user_encoder
    cuda = device.type == "cuda"
    sa = isinstance(enc, SA_NRMS_NewsEncoder)
    table = (enc if cuda else enc.forward_stock)(
        train.title_text.index_select(0, pool)[None], train.title_mask.index_select(0, pool)[None],
        train.augmented_title_text.index_select(0, pool)[None] if sa else None,
        train.augmented_title_mask.index_select(0, pool)[None] if sa else None)[0]                      # [P, d]
    at = torch.from_numpy(idx).to(device)
    hist, mask = train.history_ids.index_select(0, at).to(torch.int64), train.history_mask.index_select(0, at)
    user = (ue if cuda else ue.forward_stock)(train.title_text[hist], train.title_mask[hist], mask)    # [G, d]
    return user, table, torch.from_numpy(pos).to(device), torch.from_numpy(count.clip(0, M).astype(np.int32)).to(device), elem


def distil_step(model, train, users, ids, teacher, count=None, scale=1.0, temperature=1.0):
    """One listwise step's loss for the first stage, with its graph — ``retrieval_step``'s twin over per-user lists: for every user of
    ``users`` (impression indices of ``train``) the KL divergence of ``softmax(teacher / temperature)`` from the model's
    ``softmax(scale * <user, news>)`` over the user's OWN list ``ids[g, :count[g]]`` (``evaluate.list_softmax``), summed over the valid
    lists — those with an element and an element whose teacher value is finite — and divided by their number (by 1 when there is
    none).  ``ids`` [G, M], ``count`` [G] (None: M) and ``teacher`` [G, M] are what ``shortlist`` and ``util.score_lists`` return; an
    id outside the corpus is no element, ``-inf`` (and ``+inf``, NaN) in ``teacher`` means no target mass.  The distinct ids of the
    batch's lists form a compact pool whose titles go through ``model.news_encoder`` WITH gradients — the augmented titles too for
    NRMS-SA — into a [P, d] table; histories go through ``model.user_encoder`` on their title texts; list ids are mapped to pool
    positions.  The model's mode (dropout) is the caller's.  On CUDA tensors ``digat_list_softmax_fwd`` / ``_bwd`` on the HIP encoders;
    on CPU tensors ``forward_stock`` and the stock composition."""
    from . import evaluate
    idx, ids, teacher, count = _check_lists(users, ids, teacher, count, int(train.history_ids.shape[0]))
    user, table, pos, cnt, elem = _list_front(model, train, idx, ids, count)
    cuda = user.device.type == "cuda"
    tch = torch.from_numpy(teacher).to(user.device)
    loss, _, _ = evaluate.list_softmax(user, table, pos, cnt, tch if cuda else tch.to(user.dtype), scale=scale, temperature=temperature)
    valid = int((elem & np.isfinite(teacher)).any(axis=1).sum())
    return loss.sum() / max(valid, 1)


def distil_retriever(model, train, lists, steps, batch_users=64, lr=1e-4, seed=0, scale=1.0, temperature=1.0, optimizer=None):
    """Train ``model`` to keep in its shortlist what a teacher ranks high: ``steps`` times one ``distil_step`` on a seeded draw of
    ``batch_users`` of the given lists (without replacement inside a step; all of them when there are fewer), one backward and one
    optimizer step, in train mode.  ``lists = (users [U], ids [U, M], teacher [U, M], count [U] or None)`` is computed ONCE by the
    caller — ``shortlist`` + ``util.score_lists`` for a DIGAT teacher, ``impression_lists`` for the listwise click loss — and not
    refreshed here: recompute it between calls to follow the student's shortlist.  ``optimizer``: ``fit_retriever``'s choice.  Returns
    the per-step losses as Python floats.  The draws depend on ``seed`` and the number of lists alone, so CPU tensors see the same
    steps."""
    if not (isinstance(lists, (tuple, list)) and len(lists) == 4):
        raise ValueError("lists must be (users [U], ids [U, M], teacher [U, M], count [U] or None)")
    users, ids, teacher, count = _check_lists(*lists[:3], lists[3], int(train.history_ids.shape[0]))
    if len(users) == 0:
        raise ValueError("no list to train on")
    optimizer = _retriever_optimizer(model, lr, optimizer)
    rng = np.random.default_rng(seed)
    model.train()
    losses = []
    for _ in range(int(steps)):
        b = np.sort(rng.choice(len(users), size=min(int(batch_users), len(users)), replace=False))
        optimizer.zero_grad()
        loss = distil_step(model, train, users[b], ids[b], teacher[b], count[b], scale=scale, temperature=temperature)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return losses


def impression_lists(train, users=None):
    """Every impression's own candidates as a training list: ``(users [U] int64, ids [U, M] int64, teacher [U, M] float32, count [U]
    int32)``, numpy arrays — the rows of ``train`` (``row_impression``, ``row_candidate``, ``row_label``) in row order, M the longest
    impression (at most ``evaluate.SHORTLIST_MAX_K``), slots beyond ``count`` holding id -1.  ``teacher`` is 0 at clicked rows and
    ``-inf`` elsewhere: through ``distil_retriever`` this is the listwise click loss over whole impressions — with one click,
    ``-log softmax`` of the clicked row over the impression's candidates.  ``users`` None: every impression with a clicked row."""
    from . import evaluate
    idx, _, _ = _clicked_targets(train, users)
    cand = np.asarray(train.row_candidate, dtype=np.int64)
    imp = np.asarray(train.row_impression, dtype=np.int64)
    label = np.asarray(train.row_label)
    I = int(train.history_ids.shape[0])
    order = np.argsort(imp, kind="stable")
    per = np.bincount(imp, minlength=I)
    first = np.r_[0, np.cumsum(per)]
    n = per[idx]
    M = int(n.max()) if len(idx) else 1
    if M > evaluate.SHORTLIST_MAX_K:
        raise ValueError(f"an impression of this corpus has {M} candidates, a list holds at most SHORTLIST_MAX_K = {evaluate.SHORTLIST_MAX_K}")
    M = max(M, 1)
    ids = np.full((len(idx), M), -1, dtype=np.int64)
    teacher = np.full((len(idx), M), -np.inf, dtype=np.float32)
    slot = np.arange(M)[None, :] < n[:, None]
    rows = order[(first[idx][:, None] + np.arange(M)[None, :])[slot]]
    ids[slot] = cand[rows]
    teacher[slot] = np.where(label[rows] == 1, 0.0, -np.inf).astype(np.float32)
    return idx, ids, teacher, n.astype(np.int32)


# ---- training for the metric the evaluation prints: the pairwise nDCG loss over per-user lists ----------------------------------
def rank_step(model, train, users, ids, gain, count=None, scale=1.0, k=0):
    """One pairwise-nDCG step's loss for the first stage, with its graph — ``distil_step``'s twin on ``evaluate.list_pairwise``: for
    every user of ``users`` (impression indices of ``train``) the LambdaRank loss of the model's scores ``scale * <user, news>`` over
    the user's OWN list ``ids[g, :count[g]]`` against the relevance ``gain`` [G, M] (finite and >= 0; NaN, an infinity or a negative
    value: no label), with the discount ``evaluate.ndcg_discount(M, k)`` — ``k`` > 0 trains for nDCG@k —, summed over the valid lists —
    those with a labelled element of positive gain — and divided by their number (by 1 when there is none).  The compact pool, the
    encoders and the devices are ``distil_step``'s.  The model's mode (dropout) is the caller's."""
    from . import evaluate
    idx, ids, gain, count = _check_lists(users, ids, gain, count, int(train.history_ids.shape[0]))
    user, table, pos, cnt, elem = _list_front(model, train, idx, ids, count)
    cuda = user.device.type == "cuda"
    gn = torch.from_numpy(gain).to(user.device)
    D = evaluate.ndcg_discount(ids.shape[1], k)
    loss, _, _ = evaluate.list_pairwise(user, table, pos, cnt, gn if cuda else gn.to(user.dtype), scale=scale, discount=D)
    with np.errstate(invalid="ignore"):
        valid = int((elem & np.isfinite(gain) & (gain > 0)).any(axis=1).sum()) if len(D) and D[0] > 0 else 0
    return loss.sum() / max(valid, 1)


def fit_ranker(model, train, lists, steps, batch_users=64, lr=1e-4, seed=0, scale=1.0, k=0, optimizer=None):
    """Train ``model`` for the nDCG the evaluation prints: ``distil_retriever``'s loop on ``rank_step`` — ``steps`` times one step on a
    seeded draw of ``batch_users`` of the given lists (the same draws as ``distil_retriever``'s for the same ``seed`` and number of
    lists), one backward and one optimizer step, in train mode.  ``lists = (users [U], ids [U, M], gain [U, M], count [U] or None)``:
    ``impression_gain_lists`` for click gains on whole impressions, or graded gains from a teacher's scores.  ``optimizer``:
    ``fit_retriever``'s choice.  Returns the per-step losses as Python floats."""
    if not (isinstance(lists, (tuple, list)) and len(lists) == 4):
        raise ValueError("lists must be (users [U], ids [U, M], gain [U, M], count [U] or None)")
    users, ids, gain, count = _check_lists(*lists[:3], lists[3], int(train.history_ids.shape[0]))
    if len(users) == 0:
        raise ValueError("no list to train on")
    optimizer = _retriever_optimizer(model, lr, optimizer)
    rng = np.random.default_rng(seed)
    model.train()
    losses = []
    for _ in range(int(steps)):
        b = np.sort(rng.choice(len(users), size=min(int(batch_users), len(users)), replace=False))
        optimizer.zero_grad()
        loss = rank_step(model, train, users[b], ids[b], gain[b], count[b], scale=scale, k=k)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return losses


def impression_gain_lists(train, users=None):
    """``impression_lists`` with relevance gains in place of the teacher: ``(users [U] int64, ids [U, M] int64, gain [U, M] float32,
    count [U] int32)`` — ``gain`` 1.0 at clicked rows, 0.0 at the impression's other rows and NaN (no label) beyond ``count``: through
    ``fit_ranker`` the pairwise nDCG loss over whole impressions."""
    idx, ids, teacher, n = impression_lists(train, users)
    slot = np.arange(ids.shape[1])[None, :] < n[:, None]
    gain = np.where(slot, np.where(teacher == 0, 1.0, 0.0), np.nan).astype(np.float32)
    return idx, ids, gain, n


# ---- policy gradient: the Plackett-Luce likelihood of slates over per-user lists (evaluate.list_pl) -----------------------------
def _slate_tensor(x, dims, G, name, device, floating):
    """A per-slate argument of ``policy_step`` as a tensor on ``device`` (a tensor already there is not copied), checked."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() != dims or int(t.shape[0]) != G or t.is_floating_point() != floating or t.dtype == torch.bool:
        raise ValueError(f"{name} must be {'a floating-point' if floating else 'an integer'} array with {dims} axes, the first of length "
                         f"{G}, got {tuple(t.shape)} {t.dtype}")
    return t.to(device)


def policy_step(model, train, users, ids, slates, weight, count=None, scale=1.0, temperature=1.0):
    """One policy-gradient step's loss for the first stage, with its graph — ``distil_step``'s twin on ``evaluate.list_pl``: for every
    user of ``users`` (impression indices of ``train``) and every slate ``slates[g, s]`` (news ids [G, S, k], -1 ends a slate; matched
    to positions of the user's OWN list ``ids[g, :count[g]]`` with ``util.slate_positions``) the log-probability ``logp[g, s]`` of the
    slate under the Plackett-Luce policy ``softmax(scale * <user, news> / temperature)`` drawn without replacement.  ``weight`` [G, S]
    is a constant per slate — an advantage, a clipped importance weight times a reward, or 1 for maximum likelihood (ListMLE when the
    slate is the ground-truth order).  The loss is ``-sum(weight * logp)`` divided by the number of slates that have a non-zero
    weight and a non-empty cut (by 1 when there is none).  Returns ``(loss, logp.detach() [G, S])`` — the second for importance
    weights.  The compact pool, the encoders and the devices are ``distil_step``'s; the model's mode (dropout) is the caller's."""
    from . import evaluate, util
    ids_in = _host_array(ids)
    idx, ids, _, count = _check_lists(users, ids_in, np.zeros(np.shape(ids_in), dtype=np.float32), count, int(train.history_ids.shape[0]))
    user, table, pos, cnt, _ = _list_front(model, train, idx, ids, count)
    dev = user.device
    G = len(idx)
    sl = _slate_tensor(slates, 3, G, "slates", dev, False)
    wt = _slate_tensor(weight, 2, G, "weight", dev, True)
    if tuple(wt.shape) != tuple(sl.shape[:2]):
        raise ValueError(f"weight must have one entry per slate {tuple(sl.shape[:2])}, got {tuple(wt.shape)}")
    picks = util.slate_positions(torch.from_numpy(ids).to(dev), cnt, sl)
    logp, _, scores = evaluate.list_pl(user, table, pos, cnt, picks, scale=scale, temperature=temperature)
    first = picks[:, :, 0].to(torch.int64)
    begun = (first >= 0) & torch.isfinite(scores.gather(1, first.clamp(min=0)))       # the cut is not empty: its first entry is live
    wt = wt.to(logp.dtype)
    n = ((wt != 0) & begun).sum().clamp(min=1)
    return -(wt * logp).sum() / n, logp.detach()


def _list_scores(model, train, idx, ids, count):
    """The batch's list scores without a graph — ``list_softmax``'s forward, as ``evaluate.refine_lists`` uses it: ``(scores [G, M]
    float32-or-model dtype, NaN at slots that are no element, count [G] int32)``."""
    from . import evaluate
    with torch.no_grad():
        user, table, pos, cnt, _ = _list_front(model, train, idx, ids, count)
        _, _, scores = evaluate.list_softmax(user, table, pos, cnt, torch.zeros(pos.shape, dtype=user.dtype, device=user.device))
    return scores, cnt


def slate_ndcg(gain, picks, k: int):
    """The nDCG@k of slates: ``gain`` [G, M] (NaN, an infinity or a negative value: 0), ``picks`` [G, S, k'] positions (-1: no
    entry) -> [G, S] float64: the slate's DCG under ``evaluate.ndcg_discount(k', k)`` over the list's ideal DCG@k; 0 where that is 0."""
    from . import evaluate
    G, S, kk = (int(x) for x in picks.shape)
    g = torch.where(torch.isfinite(gain) & (gain > 0), gain, torch.zeros_like(gain)).to(torch.float64)
    disc = torch.from_numpy(evaluate.ndcg_discount(kk, k)).to(g.device)
    at = picks.to(torch.int64)
    got = torch.where(at >= 0, g.gather(1, at.clamp(min=0).view(G, S * kk)).view(G, S, kk), torch.zeros((), dtype=torch.float64, device=g.device))
    dcg = (got * disc).sum(dim=2)
    top = g.sort(dim=1, descending=True).values[:, :kk]
    idcg = (top * disc[:top.shape[1]]).sum(dim=1)
    return torch.where(idcg[:, None] > 0, dcg / idcg.clamp(min=1e-300)[:, None], torch.zeros_like(dcg))


def plrank_step(model, train, users, ids, gain, count=None, k=10, samples=4, scale=1.0, temperature=1.0, seed=0, first_sample=0):
    """One PL-Rank step's loss for the first stage, with its graph — ``rank_step``'s twin on ``evaluate.list_plrank``, in ONE scoring
    pass: a single ``_list_front`` call with the graph scores the batch's lists; ``samples`` Plackett-Luce slates of ``k`` are drawn
    per list from ``softmax(scale * <user, news> / temperature)`` inside the kernel that scored them (the impression indices
    ``users`` are the streams, ``first_sample`` the first sample index: ``pl_sample``'s draw); a slate's value is its DCG@k against
    ``gain`` [G, M] (``slate_ndcg``'s rule for NaN, infinite and negative gains) and ``list_weight = 1 / IDCG@k`` (0 where that is 0)
    makes it nDCG@k.  The loss is minus the mean of ``value`` over the lists with a positive ideal DCG (divided by 1 when there is
    none).  ``value`` is the sample mean of the slates' nDCG@k; its backward is the PL-Rank-2 estimator of the gradient of the
    EXPECTED nDCG@k — no baseline, no second encoder pass, no second dropout mask, no id-to-position matching.  Returns ``(loss,
    mean slate nDCG@k)``, the second a detached scalar over all lists and slates, as ``fit_policy`` reports its rewards.  The compact
    pool, the encoders and the devices are ``distil_step``'s; the model's mode (dropout) is the caller's."""
    from . import evaluate
    idx, ids, gain, count = _check_lists(users, ids, gain, count, int(train.history_ids.shape[0]))
    user, table, pos, cnt, _ = _list_front(model, train, idx, ids, count)
    dev = user.device
    k = int(k)
    D = evaluate.ndcg_discount(k)
    with np.errstate(invalid="ignore"):
        clean = np.where(np.isfinite(gain) & (gain > 0), gain, np.float32(0)).astype(np.float64)
    top = -np.sort(-clean, axis=1)[:, :k]
    idcg = (top * D[:top.shape[1]]).sum(axis=1)
    lw = np.where(idcg > 0, 1.0 / np.where(idcg > 0, idcg, 1.0), 0.0)
    gn = torch.from_numpy(gain).to(dev)
    value, slate_value, _, _ = evaluate.list_plrank(user, table, pos, cnt, gn if dev.type == "cuda" else gn.to(user.dtype), k, samples, D, lw,
                                                    scale=scale, temperature=temperature, seed=seed, first_sample=first_sample,
                                                    streams=torch.from_numpy(idx).to(dev))
    reward = (slate_value * torch.from_numpy(lw).to(dev)[:, None]).mean()
    return -value.sum() / max(int((idcg > 0).sum()), 1), reward.detach()


def fit_policy(model, train, lists, steps, k=10, samples=4, temperature=1.0, batch_users=64, lr=1e-4, seed=0, scale=1.0, optimizer=None,
               estimator="reinforce"):
    """``estimator="plrank"``: the same seeded batches, one ``plrank_step`` a step with ``first_sample = step * samples`` — one scoring
    pass, the PL-Rank-2 estimator in place of REINFORCE with a leave-one-out baseline; any other value but ``"reinforce"`` is a
    ``ValueError``.  ``"reinforce"`` (the default), as it always was:

    On-policy REINFORCE on the expected nDCG@k of a sampled slate: ``steps`` times, on the same seeded draw of ``batch_users``
    lists as ``fit_ranker`` and ``distil_retriever`` make, (1) the batch's lists are scored without a graph (``list_softmax``'s
    forward), (2) ``samples`` Plackett-Luce slates of ``k`` are drawn per list from ``softmax(scale * score / temperature)``
    (``evaluate.pl_sample`` with the impression index as stream and ``first_sample = step * samples``; CPU tensors:
    ``pl_sample_host``), (3) a slate's reward is its nDCG@k against ``gain`` (``slate_ndcg``), its weight the reward minus the mean
    reward of the list's OTHER samples (leave-one-out; the reward itself when ``samples == 1``), (4) one ``policy_step``, one
    backward, one optimizer step, in train mode.  The lists are therefore scored twice a step, and the two passes draw their own
    dropout masks; the sampler also takes ``temperature / scale`` as its temperature, so its ``1 / (T / scale)`` and the gradient's
    ``scale * (1 / T)`` may differ in the last bit — harmless for REINFORCE, whose weights do not use the sampler's ``logp``.
    ``lists = (users [U], ids [U, M], gain [U, M], count [U] or None)`` is ``fit_ranker``'s format
    (``impression_gain_lists``).  Returns ``(losses, mean rewards)`` per step as Python floats."""
    from . import evaluate
    if not (isinstance(lists, (tuple, list)) and len(lists) == 4):
        raise ValueError("lists must be (users [U], ids [U, M], gain [U, M], count [U] or None)")
    users, ids, gain, count = _check_lists(*lists[:3], lists[3], int(train.history_ids.shape[0]))
    if len(users) == 0:
        raise ValueError("no list to train on")
    if estimator not in ("reinforce", "plrank"):
        raise ValueError(f"estimator must be 'reinforce' or 'plrank', got {estimator!r}")
    k, samples = int(k), int(samples)
    evaluate._check_pl_args((1, ids.shape[1]), None, k, float(temperature) / float(scale), samples, max(int(steps) - 1, 0) * samples)
    optimizer = _retriever_optimizer(model, lr, optimizer)
    rng = np.random.default_rng(seed)
    model.train()
    losses, rewards = [], []
    for step in range(int(steps)):
        b = np.sort(rng.choice(len(users), size=min(int(batch_users), len(users)), replace=False))
        if estimator == "plrank":
            optimizer.zero_grad()
            loss, r = plrank_step(model, train, users[b], ids[b], gain[b], count[b], k=k, samples=samples, scale=scale, temperature=temperature,
                                  seed=seed, first_sample=step * samples)
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
            rewards.append(float(r))
            continue
        scores, cnt = _list_scores(model, train, users[b], ids[b], count[b])
        dev = scores.device
        if dev.type == "cuda":
            picks = evaluate.pl_sample(scores, cnt, k, float(temperature) / float(scale), seed, samples, step * samples,
                                       torch.from_numpy(users[b]).to(dev))[0]
        else:
            picks = torch.from_numpy(evaluate.pl_sample_host(scores.float().numpy(), cnt.numpy(), k, float(temperature) / float(scale), seed,
                                                             samples, step * samples, users[b])[0])
        at = picks.to(torch.int64)
        idt = torch.from_numpy(ids[b]).to(dev)
        slates = torch.where(at >= 0, idt.gather(1, at.clamp(min=0).view(len(b), -1)).view(at.shape), torch.full_like(at, -1))
        r = slate_ndcg(torch.from_numpy(gain[b]).to(dev), picks, k)
        weight = r if samples == 1 else r - (r.sum(dim=1, keepdim=True) - r) / (samples - 1)
        optimizer.zero_grad()
        loss, _ = policy_step(model, train, users[b], ids[b], slates, weight, count[b], scale=scale, temperature=temperature)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
        rewards.append(float(r.mean()))
    return losses, rewards


def fit_from_logs(model, train, log, reward, steps, clip=10.0, users=None, batch_users=64, lr=1e-4, seed=0, scale=1.0, temperature=None,
                  optimizer=None):
    """Off-policy training on a log of slates with their propensities: maximise the clipped-IPS value ``evaluate.off_policy_value``
    reports.  ``log`` is the dict ``util.recommend_slates`` returns — ``ids`` [U, M], ``count`` [U], ``slates`` [U, S, k] news ids,
    ``logp`` [U, S] the logging policy's log-probabilities, ``temperature`` — for the impression indices ``users`` [U] (or
    ``log["users"]``); ``reward`` [U, S]; ``temperature`` None: the log's.  Every step takes ``fit_ranker``'s seeded draw of
    ``batch_users`` lists and scores them TWICE: a first ``policy_step`` without a graph gives ``logp_now`` and the importance
    weights ``w = exp(logp_now - logp_logged)``; a slate's weight is ``w * reward`` where ``w < clip`` and 0 where it is clipped —
    the gradient of ``mean(min(w, clip) * reward)`` in the model, ``w`` held as a number —; the second ``policy_step`` carries the
    graph.  Both passes draw their own dropout masks in train mode.  Returns the per-step losses as Python floats."""
    users = log.get("users") if users is None else users
    if users is None:
        raise ValueError("name the impression indices of the log's rows: users=, or log['users']")
    idx = _host_array(users).astype(np.int64)
    ids, count, slates = _host_array(log["ids"]).astype(np.int64), _host_array(log["count"]).astype(np.int64), _host_array(log["slates"]).astype(np.int64)
    logged, rw = _host_array(log["logp"]).astype(np.float64), _host_array(reward).astype(np.float64)
    U = len(idx)
    if ids.ndim != 2 or slates.ndim != 3 or len(ids) != U or len(slates) != U or count.shape != (U,) or logged.shape != slates.shape[:2] \
            or rw.shape != logged.shape:
        raise ValueError("log must hold ids [U, M], count [U], slates [U, S, k] and logp [U, S] for the U users, and reward must be [U, S]")
    if U == 0:
        raise ValueError("no list to train on")
    if not float(clip) > 0.0:
        raise ValueError(f"clip must be positive, got {clip}")
    temperature = float(log["temperature"]) if temperature is None else float(temperature)
    optimizer = _retriever_optimizer(model, lr, optimizer)
    rng = np.random.default_rng(seed)
    model.train()
    losses = []
    for _ in range(int(steps)):
        b = np.sort(rng.choice(U, size=min(int(batch_users), U), replace=False))
        with torch.no_grad():
            _, now = policy_step(model, train, idx[b], ids[b], slates[b], np.zeros(rw[b].shape), count[b], scale=scale, temperature=temperature)
        w = torch.exp(now.to(torch.float64) - torch.from_numpy(logged[b]).to(now.device))
        weight = torch.where(w < float(clip), w * torch.from_numpy(rw[b]).to(now.device), torch.zeros_like(w))
        optimizer.zero_grad()
        loss, _ = policy_step(model, train, idx[b], ids[b], slates[b], weight, count[b], scale=scale, temperature=temperature)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return losses


def teacher_agreement(student_ids, student_count, teacher_ids, teacher_count, ks=(10,)):
    """How much of the teacher's top-k the student's list holds: per user the share of the first ``min(k, teacher_count[g])`` slots of
    ``teacher_ids`` [G, kt] — a list ordered best first, as ``util.recommend`` returns it — whose id stands anywhere in
    ``student_ids[g, :student_count[g]]`` (``evaluate.list_ranks``); 0 for a user whose teacher list is empty.  Returns
    ``{"agreement@k": the mean over all users, ..., "per_user": [G, len(ks)] float64, "names": [...]}``; the ``per_user`` matrix goes
    into ``evaluate.metric_intervals(per_user, names=names)`` unchanged for intervals over users."""
    from . import evaluate
    t_ids = torch.as_tensor(teacher_ids)
    if t_ids.dim() != 2:
        raise ValueError(f"teacher_ids must be [G, k], got {tuple(t_ids.shape)}")
    G, kt = int(t_ids.shape[0]), int(t_ids.shape[1])
    t_cnt = np.full(G, kt, dtype=np.int64) if teacher_count is None else _host_array(teacher_count).astype(np.int64)
    if t_cnt.shape != (G,):
        raise ValueError(f"teacher_count must have one entry per list ({G}), got shape {t_cnt.shape}")
    s_ids = torch.as_tensor(student_ids)
    if s_ids.dim() != 2 or int(s_ids.shape[0]) != G:
        raise ValueError(f"student_ids must be [G = {G}, m], got {tuple(s_ids.shape)}")
    t_host = t_ids.cpu().numpy().astype(np.int64)
    per_user, names = np.zeros((G, len(ks)), dtype=np.float64), []
    for c, k in enumerate(ks):
        if int(k) != k or k < 1:
            raise ValueError(f"every k must be a positive integer, got {k}")
        n = np.clip(t_cnt, 0, min(int(k), kt))
        start = np.r_[0, np.cumsum(n)].astype(np.int64)
        take = np.arange(kt)[None, :] < n[:, None]
        rank = evaluate.list_ranks(s_ids, student_count, t_host[take], start).cpu().numpy()
        held = np.add.reduceat(np.r_[(rank >= 0).astype(np.float64), 0.0], start[:-1])[:G] if G else np.zeros(0)
        held = np.where(n > 0, held, 0.0)                             # reduceat of an empty slice takes the next entry
        per_user[:, c] = held / np.maximum(n, 1)
        names.append(f"agreement@{int(k)}")
    out = {name: float(per_user[:, c].mean()) if G else float("nan") for c, name in enumerate(names)}
    out.update(per_user=per_user, names=names)
    return out


def candidates_csr(news_ids, count):
    """The valid slots of a ``[G,k]`` result (``recommend``'s ``news_ids`` and ``count``) as the per-user lists
    ``util.recommend(candidates=...)`` takes: ``(ids [R] int64 tensor, start [G+1] int64 numpy)`` — NRMS retrieves, DIGAT re-ranks."""
    news_ids = torch.as_tensor(news_ids)
    cnt = torch.as_tensor(count).to(torch.int64).cpu()
    if news_ids.dim() != 2 or tuple(cnt.shape) != (news_ids.shape[0],):
        raise ValueError(f"news_ids must be [G,k] and count [G], got {tuple(news_ids.shape)} and {tuple(cnt.shape)}")
    if cnt.numel() and (int(cnt.min()) < 0 or int(cnt.max()) > news_ids.shape[1]):
        raise ValueError(f"count must lie in [0, {int(news_ids.shape[1])}]")
    keep = torch.arange(news_ids.shape[1])[None, :] < cnt[:, None]
    start = np.zeros(news_ids.shape[0] + 1, dtype=np.int64)
    np.cumsum(cnt.numpy(), out=start[1:])
    return news_ids[keep.to(news_ids.device)].to(torch.int64).contiguous(), start
