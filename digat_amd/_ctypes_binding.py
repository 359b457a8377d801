"""The ctypes twin of the thin torch extension (csrc/digat_torch_ext.cpp): the same twelve functions — names, argument order,
return shapes — over the signature table of ``_lib.py``.  ``_lib.binding()`` hands out one or the other, so a call site is written
once.  This is the only road to a library named by ``DIGAT_HIP_LIB`` (the extension is linked to lib/libdigat_hip.so), and the
reference the extension is held to bit for bit (tests/test_hip_parity.py, tests/test_hip_training.py).

Nothing is checked here beyond the library's own status codes: shapes, dtypes and contiguity are the extension's to refuse, and
the callers hand both bindings the same prepared tensors.  tests/test_abi_cpu.py holds the two surfaces to each other.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

L = _lib.lib
S = _lib.stream_ptr
ptr = _lib.ptr


def _params(addr):
    return C.cast(addr, C.POINTER(_lib.Params))


def encoder_fwd(params, shared, Xn, An, Mn, ue, Au, cm, ci, c_n0, out_n, out_u, ws):
    B, N, H = Xn.shape[0], Xn.shape[1], ue.shape[1]
    fn, what = (L().digat_encoder_fwd_shared, "digat_encoder_fwd_shared") if shared else (L().digat_encoder_fwd, "digat_encoder_fwd")
    _lib.check(fn(_params(params), Xn.data_ptr(), An.data_ptr(), Mn.data_ptr(), ue.data_ptr(), Au.data_ptr(),
                  cm.data_ptr(), ci.data_ptr(), ptr(c_n0), out_n.data_ptr(), out_u.data_ptr(),
                  B, N, H, ws.data_ptr(), ws.numel(), S()), what)


def encoder_fwd_grouped(params, Xn, An, Mn, ue_g, Au_g, cm_g, ci_g, row_group, c_n0, news_hpq0, hist_hpq0, topic_hpq0, ctxq0,
                        news_index, out_n, out_u, ws):
    B, N, G, H = An.shape[0], Xn.shape[1], ue_g.shape[0], ue_g.shape[1]
    if news_hpq0 is None and hist_hpq0 is None and ctxq0 is None and news_index is None:
        _lib.check(L().digat_encoder_fwd_grouped(_params(params), Xn.data_ptr(), An.data_ptr(), Mn.data_ptr(), ue_g.data_ptr(), Au_g.data_ptr(),
                                                 cm_g.data_ptr(), ci_g.data_ptr(), row_group.data_ptr(), c_n0.data_ptr(), out_n.data_ptr(),
                                                 out_u.data_ptr(), B, G, N, H, ws.data_ptr(), ws.numel(), S()),
                   "digat_encoder_fwd_grouped")
        return
    M = Xn.shape[0] if news_index is not None else 0
    _lib.check(L().digat_encoder_fwd_grouped_cached(_params(params), Xn.data_ptr(), An.data_ptr(), Mn.data_ptr(), ue_g.data_ptr(),
                                                    Au_g.data_ptr(), cm_g.data_ptr(), ci_g.data_ptr(), row_group.data_ptr(), c_n0.data_ptr(),
                                                    ptr(news_hpq0), ptr(hist_hpq0), ptr(topic_hpq0), ptr(ctxq0), ptr(news_index), M,
                                                    out_n.data_ptr(),
                                                    out_u.data_ptr(), B, G, N, H, ws.data_ptr(), ws.numel(), S()),
               "digat_encoder_fwd_grouped_cached")


def row_logits(news_ctx, user_ctx, logits):
    B, d = news_ctx.shape
    _lib.check(L().digat_row_logits(news_ctx.data_ptr(), user_ctx.data_ptr(), logits.data_ptr(), B, d, S()),
               "digat_row_logits")


def user_row_runs(ue, Au, cm, ci, row_group, leaders, n_runs, ws):
    B, H, d = ue.shape
    U, C1 = Au.shape[1], cm.shape[1]
    _lib.check(L().digat_user_row_runs(ue.data_ptr(), Au.data_ptr(), cm.data_ptr(), ci.data_ptr(), B, H, U, C1, d,
                                       row_group.data_ptr(), leaders.data_ptr(), n_runs.data_ptr(), ws.data_ptr(), ws.numel(),
                                       S()), "digat_user_row_runs")


# ---- training: one call per function and direction.  Output, ``save`` and gradient tensors are allocated here, the scratch buffer is
# ---- _lib.workspace's per (device, stream); the save / workspace byte counts are the library's own, asked again in the backward
def xattn_fwd_train(Xd, A, cvec, W, bW, F1, F2, F3, b3, a, p, seed, p_in, seed_in, image, xattn_mode):
    B, n, d = Xd.shape
    dev = Xd.device
    out = torch.empty_like(Xd)
    nsave, nws = L().digat_xattn_train_save_bytes(B, n, d), L().digat_xattn_train_workspace_bytes(B, n, d)
    save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "train")
    _lib.check(L().digat_xattn_fwd_train(Xd.data_ptr(), A.data_ptr(), cvec.data_ptr(), W.data_ptr(), bW.data_ptr(), F1.data_ptr(),
                                         F2.data_ptr(), F3.data_ptr(), b3.data_ptr(), a.data_ptr(), out.data_ptr(), p,
                                         seed, p_in, seed_in, B, n, d, save.data_ptr(), nsave, ws.data_ptr(), nws, ptr(image), xattn_mode, S()),
               "digat_xattn_fwd_train")
    return out, save


def xattn_bwd(dOut, out, Xd, A, cvec, W, F1, F2, F3, a, p, p_in, save, image, xattn_mode):
    """-> [dX, dctx, dW3 ([3,d,d]: dW, dF1, dF2), dbW, dF3, db3, da]"""
    B, n, d = Xd.shape
    dev = Xd.device
    nsave, nws = L().digat_xattn_train_save_bytes(B, n, d), L().digat_xattn_train_workspace_bytes(B, n, d)
    ws = _lib.workspace(nws, dev, "train")
    dX, dc = torch.empty_like(Xd), torch.empty_like(cvec)
    # dW, dF1, dF2 as the three blocks of one [3 d, d] buffer: the library writes its single [3 d, d] weight-gradient product in place
    dW3 = torch.empty((3,) + tuple(W.shape), dtype=torch.float32, device=dev)
    dW, dF1, dF2 = dW3[0], dW3[1], dW3[2]
    dF3 = torch.empty_like(W)
    dbW, db3, da = (torch.empty(d, dtype=torch.float32, device=dev) for _ in range(3))
    _lib.check(L().digat_xattn_bwd(dOut.data_ptr(), out.data_ptr(), Xd.data_ptr(), A.data_ptr(), cvec.data_ptr(), W.data_ptr(),
                                   F1.data_ptr(), F2.data_ptr(), F3.data_ptr(), a.data_ptr(), p, p_in, save.data_ptr(), nsave,
                                   dX.data_ptr(), dc.data_ptr(), dW.data_ptr(), dbW.data_ptr(), dF1.data_ptr(), dF2.data_ptr(),
                                   dF3.data_ptr(), db3.data_ptr(), da.data_ptr(), B, n, d, ws.data_ptr(), nws, ptr(image), xattn_mode, S()),
               "digat_xattn_bwd")
    return [dX, dc, dW3, dbW, dF3, db3, da]


def news_ctx_fwd_train(X, mask, Kc, Qc, bQc, Wg, bg, p, seed, prev):
    B, N, d = X.shape
    dev = X.device
    out = torch.empty((B, d), dtype=torch.float32, device=dev)
    nsave, nws = L().digat_news_ctx_train_save_bytes(B, N, d), L().digat_news_ctx_train_workspace_bytes(B, N, d)
    save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "train")
    _lib.check(L().digat_news_ctx_fwd_train(X.data_ptr(), mask.data_ptr(), Kc.data_ptr(), Qc.data_ptr(), bQc.data_ptr(),
                                            Wg.data_ptr(), bg.data_ptr(), out.data_ptr(), p, seed, B, N, d,
                                            save.data_ptr(), nsave, ws.data_ptr(), nws, ptr(prev), S()), "digat_news_ctx_fwd_train")
    return out, save


def news_ctx_bwd(dout, X, mask, Kc, Qc, Wg, p, save, grads, accumulate):
    """grads: dKc, dQc, dbQc, dWg, dbg (the caller's: written, or added to when accumulate); -> dX"""
    dKc, dQc, dbQc, dWg, dbg = grads
    B, N, d = X.shape
    nsave, nws = L().digat_news_ctx_train_save_bytes(B, N, d), L().digat_news_ctx_train_workspace_bytes(B, N, d)
    ws = _lib.workspace(nws, X.device, "train")
    dX = torch.empty_like(X)
    _lib.check(L().digat_news_ctx_bwd(dout.data_ptr(), X.data_ptr(), mask.data_ptr(), Kc.data_ptr(), Qc.data_ptr(), Wg.data_ptr(),
                                      p, save.data_ptr(), nsave, dX.data_ptr(), dKc.data_ptr(), dQc.data_ptr(), dbQc.data_ptr(),
                                      dWg.data_ptr(), dbg.data_ptr(), B, N, d, accumulate, ws.data_ptr(), nws, S()), "digat_news_ctx_bwd")
    return dX


def user_ctx_fwd_train(Xu, cat_mask, cat_idx, c_n, Ku, Qu, bQu, Fa, bFa, Kua, Qua, bQua, H, C1, p, seed, image, prev):
    B, U, d = Xu.shape
    dev = Xu.device
    out = torch.empty((B, d), dtype=torch.float32, device=dev)
    nsave = L().digat_user_ctx_train_save_bytes(B, U, H, C1, d)
    nws = L().digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)
    save, ws = _lib.save_buffer(nsave, dev), _lib.workspace(nws, dev, "train")
    _lib.check(L().digat_user_ctx_fwd_train(Xu.data_ptr(), cat_mask.data_ptr(), cat_idx.data_ptr(), c_n.data_ptr(), Ku.data_ptr(),
                                            Qu.data_ptr(), bQu.data_ptr(), Fa.data_ptr(), bFa.data_ptr(), Kua.data_ptr(),
                                            Qua.data_ptr(), bQua.data_ptr(), out.data_ptr(), p, seed,
                                            B, U, H, C1, d, save.data_ptr(), nsave, ws.data_ptr(), nws, ptr(image), ptr(prev), S()),
               "digat_user_ctx_fwd_train")
    return out, save


def user_ctx_bwd(dout, Xu, cat_mask, cat_idx, c_n, Ku, Qu, Fa, Kua, Qua, p, save, grads, accumulate, H, C1, image):
    """grads: dKu, dQu, dFa, dKua, dQua, dbQu, dbFa, dbQua (the caller's; the C entry takes each bias after its weight); -> dXu, dc_n"""
    dKu, dQu, dFa, dKua, dQua, dbQu, dbFa, dbQua = grads
    B, U, d = Xu.shape
    nsave = L().digat_user_ctx_train_save_bytes(B, U, H, C1, d)
    nws = L().digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)
    ws = _lib.workspace(nws, Xu.device, "train")
    dXu, dc = torch.empty_like(Xu), torch.empty_like(c_n)
    _lib.check(L().digat_user_ctx_bwd(dout.data_ptr(), Xu.data_ptr(), cat_mask.data_ptr(), cat_idx.data_ptr(), c_n.data_ptr(),
                                      Ku.data_ptr(), Qu.data_ptr(), Fa.data_ptr(), Kua.data_ptr(), Qua.data_ptr(), p,
                                      save.data_ptr(), nsave, dXu.data_ptr(), dc.data_ptr(), dKu.data_ptr(), dQu.data_ptr(),
                                      dbQu.data_ptr(), dFa.data_ptr(), dbFa.data_ptr(), dKua.data_ptr(), dQua.data_ptr(),
                                      dbQua.data_ptr(), B, U, H, C1, d, accumulate, ws.data_ptr(), nws, ptr(image), S()), "digat_user_ctx_bwd")
    return dXu, dc


def dropout_fwd(x, p, seed):
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(L().digat_dropout_fwd(x.data_ptr(), y.data_ptr(), mask.data_ptr(), x.numel(), p, seed, S()),
               "digat_dropout_fwd")
    return y, mask


def dropout_bwd(dy, mask, p):
    dx = torch.empty_like(dy)
    _lib.check(L().digat_dropout_bwd(dy.data_ptr(), mask.data_ptr(), dx.data_ptr(), dy.numel(), p, S()),
               "digat_dropout_bwd")
    return dx
