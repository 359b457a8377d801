"""News encoders: UPSTREAM of the hot path.  ``MSA`` on the GPU runs on the HIP kernels: inference on
``digat_msa_fwd`` (``csrc/digat_news.inc``), training forward / backward on ``digat_msa_fwd_train`` / ``digat_msa_bwd``
(``csrc/digat_news_train.inc``); ``CNN`` likewise on ``digat_cnn_fwd`` / ``digat_cnn_fwd_train`` / ``digat_cnn_bwd``
(``csrc/digat_cnn.inc``); on the CPU (tests without a GPU) the stock PyTorch modules below.

Their output ``[., news_embedding_dim]`` is the graph encoder's input.  They are restated here
so that ``Model.forward`` (training) and the news-representation cache of ``compute_scores``
have a producer with the reference's parameter names (``word_embedding``, ``multiheadSelfattention.
W_{K,Q,V}``, ``attention.affine{1,2}``, ``conv.conv`` / ``conv.conv{1,2,3}``) and the same semantics:
word embedding -> dropout -> MSA (16 heads x 25) + ReLU | Conv1d + ReLU -> additive tanh attention.
GloVe initialisation needs the downloaded vectors; without them the table keeps its random init.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .training import _seed


class MultiHeadAttention(nn.Module):
    """layers.py:50-88 (no output projection, K without bias)."""

    def __init__(self, h: int, d_model: int, d_k: int, d_v: int):
        super().__init__()
        self.h, self.d_k, self.d_v = h, d_k, d_v
        self.W_K = nn.Linear(d_model, h * d_k, bias=False)
        self.W_Q = nn.Linear(d_model, h * d_k, bias=True)
        self.W_V = nn.Linear(d_model, h * d_v, bias=True)

    def initialize(self):
        nn.init.zeros_(self.W_Q.bias)
        nn.init.zeros_(self.W_V.bias)

    def forward(self, x):
        B, T, _ = x.shape
        q = self.W_Q(x).view(B, T, self.h, self.d_k).transpose(1, 2)
        k = self.W_K(x).view(B, T, self.h, self.d_k).transpose(1, 2)
        v = self.W_V(x).view(B, T, self.h, self.d_v).transpose(1, 2)
        alpha = F.softmax(q @ k.transpose(2, 3) / math.sqrt(float(self.d_k)), dim=3)
        return (alpha @ v).transpose(1, 2).reshape(B, T, self.h * self.d_v)


class Attention(nn.Module):
    """layers.py:91-115: additive attention pooling, -1e9 mask."""

    def __init__(self, feature_dim: int, attention_dim: int):
        super().__init__()
        self.affine1 = nn.Linear(feature_dim, attention_dim, bias=True)
        self.affine2 = nn.Linear(attention_dim, 1, bias=False)

    def initialize(self):
        nn.init.xavier_uniform_(self.affine1.weight, gain=nn.init.calculate_gain('tanh'))
        nn.init.zeros_(self.affine1.bias)
        nn.init.xavier_uniform_(self.affine2.weight)

    def forward(self, feature, mask=None):
        a = self.affine2(torch.tanh(self.affine1(feature))).squeeze(2)
        if mask is not None:
            a = a.masked_fill(mask == 0, -1e9)
        return (F.softmax(a, dim=1).unsqueeze(1) @ feature).squeeze(1)


class Conv1D(nn.Module):
    """layers.py:7-47 with the reference's parameter names: ``naive`` (``conv``: one window, odd, 1..7) and ``group3``
    (``conv1/2/3``: windows 1, 3, 5 on a third of the kernels each, concatenated along channels before the ReLU).  The reference's
    ``group5`` raises inside its forward (layers.py:41-46: ``torch.cat(..., dim=1)`` of a length-1 tensor), ``group4`` fails its
    constructor's assert (layers.py:10) and an even window yields Lw - 1 positions, which the attention's mask rejects: all three
    raise here, at construction."""

    def __init__(self, cnn_method: str, in_channels: int, cnn_kernel_num: int, cnn_window_size: int):
        super().__init__()
        if cnn_method not in ('naive', 'group3'):
            raise ValueError(f"cnn_method {cnn_method!r} is not supported: the reference's group5 fails in its forward "
                             "(layers.py:41-46) and anything else fails its constructor's assert (layers.py:10); use naive or group3")
        self.cnn_method, self.in_channels, self.cnn_kernel_num = cnn_method, in_channels, cnn_kernel_num
        if cnn_method == 'naive':
            if cnn_window_size % 2 == 0 or not 1 <= cnn_window_size <= 7:
                raise ValueError(f"cnn_window_size {cnn_window_size}: an even window gives Lw - 1 positions (layers.py:14: padding "
                                 "(w - 1) // 2), which the attention's mask rejects; odd windows 1..7 are supported")
            self.taps = cnn_window_size
            self.conv = nn.Conv1d(in_channels, cnn_kernel_num, kernel_size=cnn_window_size, padding=(cnn_window_size - 1) // 2)
        else:
            if cnn_kernel_num % 3:
                raise ValueError(f"group3 needs cnn_kernel_num % 3 == 0 (layers.py:16), got {cnn_kernel_num}")
            self.taps = 5
            self.conv1 = nn.Conv1d(in_channels, cnn_kernel_num // 3, kernel_size=1, padding=0)
            self.conv2 = nn.Conv1d(in_channels, cnn_kernel_num // 3, kernel_size=3, padding=1)
            self.conv3 = nn.Conv1d(in_channels, cnn_kernel_num // 3, kernel_size=5, padding=2)

    def initialize(self):
        pass

    def branches(self):
        return (self.conv,) if self.cnn_method == 'naive' else (self.conv1, self.conv2, self.conv3)

    def forward(self, x):
        if self.cnn_method == 'naive':
            return F.relu(self.conv(x))
        return F.relu(torch.cat([self.conv1(x), self.conv2(x), self.conv3(x)], dim=1))


def merge_group3(w1, w2, w3):
    """The three branch weights [K3, dm, {1,3,5}] as one zero-filled 5-tap weight [3 K3, dm, 5] (same convolution: the extra
    products are x * 0)."""
    K3, dm = w1.shape[0], w1.shape[1]
    W = w1.new_zeros((3 * K3, dm, 5))
    W[:K3, :, 2:3] = w1
    W[K3:2 * K3, :, 1:4] = w2
    W[2 * K3:] = w3
    return W


def _embedding_grad(tokens, row_grad, ld, table):
    """The word-embedding gradient: the rows of ``row_grad`` ([T Lw, ld]) summed per token.  Index plumbing only here — the rows in
    token order (stable); the sums run in the library (``digat_embedding_bwd``), in that fixed order."""
    L = _lib.lib()
    M, dm = tokens.numel(), table.shape[1]
    stok, order = torch.sort(tokens.reshape(-1).to(torch.int64), stable=True)
    stok, order = stok.to(torch.int32), order.to(torch.int32)
    dtable = torch.zeros_like(table)
    nb = L.digat_embedding_bwd_workspace_bytes(M, dm)
    ews = _lib.workspace(nb, tokens.device, "emb_bwd")
    _lib.check(L.digat_embedding_bwd(row_grad.data_ptr(), ld, order.data_ptr(), stok.data_ptr(), M, dm, dtable.data_ptr(),
                                     ews.data_ptr(), nb, _lib.stream_ptr()), "digat_embedding_bwd")
    return dtable


class CnnFused(torch.autograd.Function):
    """The CNN news encoder as one library call per direction (``digat_cnn_fwd_train`` / ``digat_cnn_bwd``, then
    ``digat_embedding_bwd`` for the word-embedding rows).  ``conv`` is (W, b) for ``naive`` or (W1, b1, W2, b2, W3, b3) for ``group3``:
    the latter run as the zero-filled 5-tap convolution and each branch's gradient is cut from its own taps."""

    @staticmethod
    def _merged(conv, dev):
        """(W [Kc, dm, taps], b [Kc]) fp32 contiguous."""
        c = [w.detach().float().contiguous() for w in conv]
        if len(c) == 2:
            return c[0], c[1]
        K3, dm = c[0].shape[0], c[0].shape[1]
        W = torch.empty((3 * K3, dm, 5), dtype=torch.float32, device=dev)
        b = torch.empty(3 * K3, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().digat_cnn_merge_group3(*(t.data_ptr() for t in c), dm, 3 * K3, W.data_ptr(), b.data_ptr(), _lib.stream_ptr()),
                   "digat_cnn_merge_group3")
        return W, b

    @staticmethod
    def _params(table, W, b, A1, b1, a2):
        P = _lib.CnnParams(word_embedding_dim=table.shape[1], kernel_num=W.shape[0], taps=W.shape[2], attention_dim=A1.shape[0])
        for name, w in zip(("word_embedding", "W", "b", "A1", "b1", "a2"), (table, W, b, A1, b1, a2)):
            setattr(P, name, w.data_ptr())
        return P

    @staticmethod
    def forward(ctx, tokens, mask, table, A1, b1, a2, p_drop, *conv):
        L = _lib.lib()
        table_, A1_, b1_, a2_ = (w.detach().float().contiguous() for w in (table, A1, b1, a2))
        dev = _lib.require_device(tokens, mask, table_, A1_, b1_, a2_, *conv)
        W, b = CnnFused._merged(conv, dev)
        T, Lw = tokens.shape
        dims = (T, Lw, table_.shape[1], W.shape[0], W.shape[2], A1_.shape[0])
        P = CnnFused._params(table_, W, b, A1_, b1_, a2_)
        out = torch.empty((T, W.shape[0]), dtype=torch.float32, device=dev)
        nsave, nws = L.digat_cnn_train_save_bytes(*dims), L.digat_cnn_train_workspace_bytes(*dims)
        save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "cnn_train")
        p = float(p_drop)
        seed = _seed() if p > 0 else 0
        if T:
            _lib.check(L.digat_cnn_fwd_train(P, tokens.data_ptr(), mask.data_ptr(), out.data_ptr(), p, seed, T, Lw, save.data_ptr(), nsave,
                                             ws.data_ptr(), nws, _lib.stream_ptr()), "digat_cnn_fwd_train")
        ctx.save_for_backward(tokens, mask, save, table_, W, b, A1_, b1_, a2_)
        ctx.p, ctx.seed, ctx.sizes, ctx.group3, ctx.a2_shape = p, seed, (nsave, nws), len(conv) == 6, a2.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        tokens, mask, save, table, W, b, A1, b1, a2 = ctx.saved_tensors
        T, Lw = tokens.shape
        dm, Kc, att = table.shape[1], W.shape[0], A1.shape[0]
        dev = tokens.device
        f = dict(dtype=torch.float32, device=dev)

        def conv_grads(dW, db):
            if not ctx.group3:
                return dW, db
            K3 = Kc // 3                              # each branch from its own taps only
            return (dW[:K3, :, 2:3].contiguous(), db[:K3].contiguous(), dW[K3:2 * K3, :, 1:4].contiguous(), db[K3:2 * K3].contiguous(),
                    dW[2 * K3:].contiguous(), db[2 * K3:].contiguous())
        if T == 0:                                    # no title: every gradient is zero
            return (None, None, torch.zeros_like(table) if ctx.needs_input_grad[2] else None, torch.zeros_like(A1), torch.zeros_like(b1),
                    torch.zeros(ctx.a2_shape, **f), None, *conv_grads(torch.zeros_like(W), torch.zeros_like(b)))
        dout = dout.float().contiguous()
        P = CnnFused._params(table, W, b, A1, b1, a2)
        nsave, nws = ctx.sizes
        ws = _lib.workspace(nws, dev, "cnn_train")
        row_grad = torch.empty((T * Lw, dm), **f)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        dA1, db1, da2 = torch.empty((att, Kc), **f), torch.empty(att, **f), torch.empty(att, **f)
        _lib.check(L.digat_cnn_bwd(P, tokens.data_ptr(), mask.data_ptr(), dout.data_ptr(), ctx.p, ctx.seed, save.data_ptr(), nsave,
                                   row_grad.data_ptr(), dm, dW.data_ptr(), db.data_ptr(), dA1.data_ptr(), db1.data_ptr(), da2.data_ptr(),
                                   T, Lw, ws.data_ptr(), nws, _lib.stream_ptr()), "digat_cnn_bwd")
        dtable = _embedding_grad(tokens, row_grad, dm, table) if ctx.needs_input_grad[2] else None
        return (None, None, dtable, dA1, db1, da2.view(ctx.a2_shape), None, *conv_grads(dW, db))


class MsaFused(torch.autograd.Function):
    """The MSA news encoder as one library call per direction (``digat_msa_fwd_train`` / ``digat_msa_bwd``,
    ``digat_embedding_bwd`` for the word-embedding rows)."""

    @staticmethod
    def _params(table, WQ, bQ, WK, WV, bV, A1, b1, a2, heads, dk):
        P = _lib.MsaParams(word_embedding_dim=table.shape[1], head_num=heads, head_dim=dk, attention_dim=A1.shape[0])
        for name, w in zip(("word_embedding", "W_Q", "b_Q", "W_K", "W_V", "b_V", "A1", "b1", "a2"), (table, WQ, bQ, WK, WV, bV, A1, b1, a2)):
            setattr(P, name, w.data_ptr())
        return P

    @staticmethod
    def forward(ctx, tokens, mask, table, WQ, bQ, WK, WV, bV, A1, b1, a2, heads, dk, p_drop):
        L = _lib.lib()
        ws_ = [w.detach().float().contiguous() for w in (table, WQ, bQ, WK, WV, bV, A1, b1, a2)]
        dev = _lib.require_device(tokens, mask, *ws_)
        T, Lw = tokens.shape
        dims = (T, Lw, ws_[0].shape[1], heads, dk, ws_[6].shape[0])
        P = MsaFused._params(*ws_, heads, dk)
        out = torch.empty((T, heads * dk), dtype=torch.float32, device=dev)
        nsave, nws = L.digat_msa_train_save_bytes(*dims), L.digat_msa_train_workspace_bytes(*dims)
        save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "msa_train")
        p = float(p_drop)
        seed = _seed() if p > 0 else 0
        if T:
            _lib.check(L.digat_msa_fwd_train(P, tokens.data_ptr(), mask.data_ptr(), out.data_ptr(), p, seed, T, Lw, save.data_ptr(),
                                             nsave, ws.data_ptr(), nws, _lib.stream_ptr()), "digat_msa_fwd_train")
        ctx.save_for_backward(tokens, mask, save, *ws_)
        ctx.dims, ctx.p, ctx.sizes = (heads, dk), p, (nsave, nws)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        tokens, mask, save, *ws_ = ctx.saved_tensors
        table, WQ, bQ, WK, WV, bV, A1, b1, a2 = ws_
        heads, dk = ctx.dims
        T, Lw = tokens.shape
        dm, hd, att = table.shape[1], heads * dk, A1.shape[0]
        dev = tokens.device
        if T == 0:                                # no title: every gradient is zero
            z = [torch.zeros_like(w) for w in ws_]
            return (None, None, z[0] if ctx.needs_input_grad[2] else None, *z[1:], None, None, None)
        dout = dout.float().contiguous()
        P = MsaFused._params(*ws_, heads, dk)
        nsave, nws = ctx.sizes
        ws = _lib.workspace(nws, dev, "msa_train")
        f = dict(dtype=torch.float32, device=dev)
        ld = int(L.digat_msa_row_grad_ld(T, Lw, dm))
        row_grad = torch.empty((T * Lw, ld), **f)
        dW3 = torch.empty((3, hd, dm), **f)       # one buffer: the library writes its single [3 hd, dm] weight-gradient product in place
        dWQ, dWK, dWV = dW3[0], dW3[1], dW3[2]
        dbQ, dbV = torch.empty(hd, **f), torch.empty(hd, **f)
        dA1, db1, da2 = torch.empty((att, hd), **f), torch.empty(att, **f), torch.empty(att, **f)
        _lib.check(L.digat_msa_bwd(P, tokens.data_ptr(), mask.data_ptr(), dout.data_ptr(), ctx.p, save.data_ptr(), nsave,
                                   row_grad.data_ptr(), ld, dWQ.data_ptr(), dbQ.data_ptr(), dWK.data_ptr(), dWV.data_ptr(), dbV.data_ptr(),
                                   dA1.data_ptr(), db1.data_ptr(), da2.data_ptr(), T, Lw, ws.data_ptr(), nws, _lib.stream_ptr()),
                   "digat_msa_bwd")
        dtable = _embedding_grad(tokens, row_grad, ld, table) if ctx.needs_input_grad[2] else None
        return None, None, dtable, dWQ, dbQ, dWK, dWV, dbV, dA1, db1, da2.view_as(a2), None, None, None


class NewsEncoder(nn.Module):
    """What both encoders share: the word embedding and its dropout, and the call path of the HIP kernels.  A subclass names its
    library entry (``_hip_entry``) and builds its parameter block (``_hip_tensors`` / ``_build_hip_params``)."""

    def __init__(self, config):
        super().__init__()
        self.word_embedding_dim = config.word_embedding_dim
        self.max_sentence_length = config.max_title_length
        self.word_embedding = nn.Embedding(config.vocabulary_size, self.word_embedding_dim)
        self.dropout = nn.Dropout(p=config.dropout_rate)

    def initialize(self):
        pass

    def _words(self, title_text):
        B, n = title_text.shape[:2]
        w = self.dropout(self.word_embedding(title_text.long()))
        return w.view(B * n, self.max_sentence_length, self.word_embedding_dim), B, n

    @staticmethod
    def _flat(title_text, title_mask):
        """[..., Lw] -> tokens int32 [T, Lw], mask uint8 [T, Lw], contiguous: what the library reads."""
        Lw = title_text.shape[-1]
        return title_text.reshape(-1, Lw).to(torch.int32).contiguous(), (title_mask.reshape(-1, Lw) != 0).to(torch.uint8).contiguous()

    def _hip_params(self):
        """(parameter block, the tensors it points into) for inference, rebuilt when a parameter has moved or been written."""
        ws = self._hip_tensors()
        key = tuple((w.data_ptr(), w._version) for w in ws)
        cached = getattr(self, "_hip_cache", None)
        if cached is None or cached[0] != key:
            cached = self._hip_cache = (key, self._build_hip_params(ws))
        return cached[1]

    def encode_hip(self, title_text, title_mask):
        """title_text / title_mask [B, n, Lw] (or [T, Lw]) on the GPU -> [B, n, news_embedding_dim] ([T, ...])."""
        tok, msk = self._flat(title_text, title_mask)
        dev = _lib.require_device(tok, msk)
        T, Lw = tok.shape
        P, _keep = self._hip_params()
        out = torch.empty((T, self.news_embedding_dim), dtype=torch.float32, device=dev)
        if T:
            L = _lib.lib()
            name, dims = self._hip_entry(P)
            nbytes = getattr(L, f"digat_{name}_workspace_bytes")(T, Lw, *dims)
            ws = _lib.workspace(nbytes, dev, name)
            _lib.check(getattr(L, f"digat_{name}_fwd")(P, tok.data_ptr(), msk.data_ptr(), out.data_ptr(), T, Lw, ws.data_ptr(), nbytes,
                                                      _lib.stream_ptr()), f"digat_{name}_fwd")
        return out.view(*title_text.shape[:-1], self.news_embedding_dim)


class MSA(NewsEncoder):
    """newsEncoders.py:58-82."""

    def __init__(self, config):
        super().__init__(config)
        self.multiheadSelfattention = MultiHeadAttention(config.MSA_head_num, config.word_embedding_dim,
                                                         config.MSA_head_dim, config.MSA_head_dim)
        self.news_embedding_dim = config.MSA_head_num * config.MSA_head_dim
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        self.multiheadSelfattention.initialize()
        self.attention.initialize()

    def forward(self, title_text, title_mask):
        if title_text.is_cuda and not torch.is_grad_enabled():
            if not self.training or self.dropout.p == 0:
                return self.encode_hip(title_text, title_mask)  # inference: the HIP kernels (digat_msa_fwd)
        if title_text.is_cuda and torch.is_grad_enabled() and title_text.shape[-1] <= 32:
            return self.train_hip(title_text, title_mask)       # training: digat_msa_fwd_train / digat_msa_bwd
        return self.forward_stock(title_text, title_mask)       # CPU (tests without a GPU)

    def forward_stock(self, title_text, title_mask):
        """The same function on stock PyTorch modules (CPU runs; the yardstick of tools/kbench.py msa-train)."""
        w, B, n = self._words(title_text)
        h = F.relu(self.multiheadSelfattention(w))
        return self.attention(h, mask=title_mask.view(B * n, -1)).view(B, n, self.news_embedding_dim)

    def _hip_tensors(self):
        mha, att = self.multiheadSelfattention, self.attention
        return [self.word_embedding.weight, mha.W_Q.weight, mha.W_Q.bias, mha.W_K.weight, mha.W_V.weight, mha.W_V.bias,
                att.affine1.weight, att.affine1.bias, att.affine2.weight]

    def train_hip(self, title_text, title_mask):
        """Forward with autograd through the HIP pair (newsEncoders.py:70-82; dropout on the embedded tokens in train mode)."""
        mha = self.multiheadSelfattention
        out = MsaFused.apply(*self._flat(title_text, title_mask), *self._hip_tensors(), mha.h, mha.d_k,
                             float(self.dropout.p) if self.training else 0.0)
        return out.view(*title_text.shape[:-1], self.news_embedding_dim)

    # ---- inference on the HIP kernels (digat_news.inc)
    def _hip_entry(self, P):
        return "msa", (P.word_embedding_dim, P.head_num, P.head_dim, P.attention_dim)

    def _build_hip_params(self, ws):
        L = _lib.lib()
        mha = self.multiheadSelfattention
        dm, hd, att = self.word_embedding_dim, mha.h * mha.d_k, self.attention.affine1.out_features
        dev = ws[0].device
        keep = [w.detach().float().contiguous() for w in ws]
        P = MsaFused._params(*keep, mha.h, mha.d_k)
        if hd % 80 == 0 and dm % 4 == 0 and dm >= 32:          # the bf16x6 matrix-core path (fp32-grade)
            qkv = _lib.split_buffer(L.digat_msa_split_bytes(dm, mha.h, mha.d_k), dev)
            _lib.check(L.digat_split_msa_weights(keep[1].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), dm, hd,
                                                 qkv.data_ptr(), _lib.stream_ptr()), "digat_split_msa_weights")
            a1 = _lib.split_buffer(L.digat_split_weights_bytes(att, hd), dev)
            # the MSA encoder's operand format is bf16x6 (no range limit: word embeddings are whatever the vocabulary file holds)
            _lib.check(L.digat_split_weights(keep[6].data_ptr(), att, hd, a1.data_ptr(), _lib.GEMM_BF16X6, _lib.stream_ptr()), "digat_split_weights")
            P.qkv_wsplit, P.a1_wsplit = qkv.data_ptr(), a1.data_ptr()
            keep += [qkv, a1]
        return P, keep


class CNN(NewsEncoder):
    """newsEncoders.py:29-54 with layers.Conv1D (``naive`` or ``group3``)."""

    def __init__(self, config):
        super().__init__(config)
        self.conv = Conv1D(getattr(config, 'cnn_method', 'naive'), config.word_embedding_dim, config.cnn_kernel_num, config.cnn_window_size)
        self.news_embedding_dim = config.cnn_kernel_num
        self.attention = Attention(self.news_embedding_dim, config.attention_dim)

    def initialize(self):
        self.conv.initialize()
        self.attention.initialize()

    def _hip_shape_ok(self, training: bool) -> bool:
        """What the library takes (include/digat_hip.h): float4 rows everywhere; group3 additionally whole float4 rows per branch."""
        ok = self.word_embedding_dim % 4 == 0 and self.news_embedding_dim % (12 if self.conv.cnn_method == 'group3' else 4) == 0
        return ok and (not training or self.attention.affine1.out_features % 4 == 0)

    def forward(self, title_text, title_mask):
        if title_text.is_cuda and not torch.is_grad_enabled() and self._hip_shape_ok(False) and title_text.shape[-1] <= 64:
            if not self.training or self.dropout.p == 0:
                return self.encode_hip(title_text, title_mask)  # inference: the HIP kernels (digat_cnn_fwd)
        if title_text.is_cuda and torch.is_grad_enabled() and title_text.shape[-1] <= 32 and self._hip_shape_ok(True):
            return self.train_hip(title_text, title_mask)       # training: digat_cnn_fwd_train / digat_cnn_bwd
        return self.forward_stock(title_text, title_mask)       # CPU (tests without a GPU)

    def forward_stock(self, title_text, title_mask):
        """The same function on stock PyTorch modules (CPU runs; the yardstick of tools/kbench.py cnn / cnn-train)."""
        w, B, n = self._words(title_text)
        h = self.dropout(self.conv(w.permute(0, 2, 1)).permute(0, 2, 1))
        return self.attention(h, mask=title_mask.view(B * n, -1)).view(B, n, self.news_embedding_dim)

    def _hip_tensors(self):
        """table, A1, b1, a2, then (weight, bias) of every convolution branch."""
        att = self.attention
        out = [self.word_embedding.weight, att.affine1.weight, att.affine1.bias, att.affine2.weight]
        for c in self.conv.branches():
            out += [c.weight, c.bias]
        return out

    def train_hip(self, title_text, title_mask):
        """Forward with autograd through the HIP pair (both dropouts of newsEncoders.py:46-48 live in train mode)."""
        ws = self._hip_tensors()
        out = CnnFused.apply(*self._flat(title_text, title_mask), *ws[:4], float(self.dropout.p) if self.training else 0.0, *ws[4:])
        return out.view(*title_text.shape[:-1], self.news_embedding_dim)

    # ---- inference on the HIP kernels (digat_cnn.inc)
    def _hip_entry(self, P):
        return "cnn", (P.word_embedding_dim, P.kernel_num, P.taps, P.attention_dim)

    def _build_hip_params(self, ws):
        L = _lib.lib()
        dev = ws[0].device
        table, A1, b1, a2 = (w.detach().float().contiguous() for w in ws[:4])
        W, b = CnnFused._merged(ws[4:], dev)
        P = CnnFused._params(table, W, b, A1, b1, a2)
        keep = [table, A1, b1, a2, W, b]
        dm, Kc, taps, natt = table.shape[1], W.shape[0], W.shape[2], A1.shape[0]
        if dm % 4 == 0 and dm >= 32 and Kc % 4 == 0:            # the bf16x6 matrix-core path (fp32-grade)
            img = torch.empty(int(L.digat_cnn_split_bytes(dm, Kc, taps)), dtype=torch.uint8, device=dev)
            _lib.check(L.digat_split_cnn_weights(W.data_ptr(), dm, Kc, taps, img.data_ptr(), _lib.stream_ptr()), "digat_split_cnn_weights")
            a1 = _lib.split_buffer(L.digat_split_weights_bytes(natt, Kc), dev)
            _lib.check(L.digat_split_weights(A1.data_ptr(), natt, Kc, a1.data_ptr(), _lib.GEMM_BF16X6, _lib.stream_ptr()), "digat_split_weights")
            P.w_split, P.a1_wsplit = img.data_ptr(), a1.data_ptr()
            keep += [img, a1]
        return P, keep
