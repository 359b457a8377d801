"""CPU suite for the training entries' C ABI (the Eq. 8 layer, the news and user contexts, the vanilla-GAT layer, the pairwise
backward): the ten size queries pinned per shape, and the status of a call whose save or workspace buffer is one byte short.  No
device: a size query is host arithmetic and every status case fails before anything is read or launched."""
import ctypes

import pytest


def align256(v):
    return (v + 255) // 256 * 256


# (B, n, d) -> (xattn save, xattn workspace WITH its dead regions, pairwise backward workspace, gat save, gat train workspace, gat
# workspace).  The byte counts are ABI: Python and the torch extension size their buffers with them.  The second figure is the Eq. 8
# workspace while its backward layout still held `wcat` ([3 d, d] fp32) and `db3g` ([3 d] fp32), two regions no launch had read
# since the stacked weights are split from their three homes and the reduction writes dbW in place: the query returns that figure
# minus align256(3 d d 4) + align256(3 d 4), and the test below spells the subtraction out.
GRAPH_SIZES = {
    (320, 67, 400): (159232768, 259628544, 60914688, 47232512, 122200320, 40221440),
    (320, 10, 400): (22560256, 60770048, 7352320, 5408000, 25492992, 5273600),
    (32, 67, 80): (4219648, 5874176, 2597888, 1979392, 2431232, 1278208),
    (3, 10, 80): (45824, 633856, 18176, 12800, 279296, 11520),
    (2, 128, 32): (434688, 767488, 434944, 327680, 292352, 165888),
    (1, 1, 4): (2560, 34048, 1792, 1024, 16640, 1024),
}
# (B, N, d) -> (news-context save, news-context workspace WITH `wsplit`): the backward carved a split scratch of
# digat_split_weights_bytes(3 d, 2 d) bytes that no product of this entry splits into
NEWS_SIZES = {
    (320, 10, 400): (2700800, 33968384),
    (5, 10, 400): (43008, 8366080),
    (2100, 3, 80): (3553536, 4521216),
    (1, 1, 4): (1536, 17152),
}
# (B, U, H, C1, d) -> (user-context save, user-context workspace): the forward's dead T2 was the smaller side of the buffer
USER_SIZES = {
    (320, 67, 50, 18, 400): (32087040, 75877376),
    (5, 67, 50, 18, 400): (502784, 10717184),
    (64, 101, 70, 32, 80): (2237952, 2693632),
    (1, 2, 1, 2, 4): (2560, 18432),
}


def _lib_built():
    from digat_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


@pytest.mark.parametrize("shape", list(GRAPH_SIZES))
def test_graph_layer_size_queries_are_pinned(shape):
    _, L = _lib_built()
    B, n, d = shape
    xsave, xws_with_dead, pairwise, gsave, gtrain, gfwd = GRAPH_SIZES[shape]
    dead = align256(3 * d * d * 4) + align256(3 * d * 4)                    # wcat + db3g: 1 924 864 bytes at d = 400
    got = (L.digat_xattn_train_save_bytes(*shape), L.digat_xattn_train_workspace_bytes(*shape), L.digat_xattn_pairwise_bwd_workspace(*shape),
           L.digat_gat_train_save_bytes(*shape), L.digat_gat_train_workspace_bytes(*shape), L.digat_gat_workspace_bytes(*shape))
    assert got == (xsave, xws_with_dead - dead, pairwise, gsave, gtrain, gfwd), shape


@pytest.mark.parametrize("shape", list(NEWS_SIZES))
def test_news_context_size_queries_are_pinned(shape):
    _, L = _lib_built()
    B, N, d = shape
    save, ws_with_wsplit = NEWS_SIZES[shape]
    dead = align256(L.digat_split_weights_bytes(3 * d, 2 * d))              # 5 760 000 bytes at d = 400
    got = (L.digat_news_ctx_train_save_bytes(*shape), L.digat_news_ctx_train_workspace_bytes(*shape))
    assert got == (save, ws_with_wsplit - dead), shape


@pytest.mark.parametrize("shape", list(USER_SIZES))
def test_user_context_size_queries_are_pinned(shape):
    _, L = _lib_built()
    got = (L.digat_user_ctx_train_save_bytes(*shape), L.digat_user_ctx_train_workspace_bytes(*shape))
    assert got == USER_SIZES[shape], shape


WORKSPACE = 3
BIG = 1 << 30


def short_buffer_cases(L):
    """[(what, returned status)]: every training entry with its save buffer, then its workspace, one byte below the published query;
    digat_gat_fwd and digat_xattn_pairwise_bwd with a short workspace.  Non-null HOST addresses and B > 0: each call must end before
    anything is read or launched.  (B == 0 is left out on purpose: the Eq. 8 and GAT backwards then zero-fill their gradients,
    hipMemsetAsync, which host addresses and a machine without a device cannot serve.)"""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    B, n, d = 3, 10, 80
    U, H, C1 = 12, 5, 4
    xs, xw = L.digat_xattn_train_save_bytes(B, n, d), L.digat_xattn_train_workspace_bytes(B, n, d)
    ns, nw = L.digat_news_ctx_train_save_bytes(B, n, d), L.digat_news_ctx_train_workspace_bytes(B, n, d)
    us, uw = L.digat_user_ctx_train_save_bytes(B, U, H, C1, d), L.digat_user_ctx_train_workspace_bytes(B, U, H, C1, d)
    gs, gw = L.digat_gat_train_save_bytes(B, n, d), L.digat_gat_train_workspace_bytes(B, n, d)
    assert min(xs, xw, ns, nw, us, uw, gs, gw) > 1

    entries = {
        "xattn_fwd_train": (xs, xw, lambda nsave, nws: L.digat_xattn_fwd_train(*[a] * 11, 0.2, 1, 0.25, 2, B, n, d, a, nsave, a, nws, None, 0, None)),
        "xattn_bwd": (xs, xw, lambda nsave, nws: L.digat_xattn_bwd(*[a] * 10, 0.2, 0.25, a, nsave, *[a] * 9, B, n, d, a, nws, None, 0, None)),
        "news_ctx_fwd_train": (ns, nw, lambda nsave, nws: L.digat_news_ctx_fwd_train(*[a] * 8, 0.1, 1, B, n, d, a, nsave, a, nws, None, None)),
        "news_ctx_bwd": (ns, nw, lambda nsave, nws: L.digat_news_ctx_bwd(*[a] * 6, 0.1, a, nsave, *[a] * 6, B, n, d, 0, a, nws, None)),
        "user_ctx_fwd_train": (us, uw, lambda nsave, nws: L.digat_user_ctx_fwd_train(*[a] * 13, 0.2, 1, B, U, H, C1, d, a, nsave, a, nws, None, None,
                                                                                     None)),
        "user_ctx_bwd": (us, uw, lambda nsave, nws: L.digat_user_ctx_bwd(*[a] * 10, 0.2, a, nsave, *[a] * 10, B, U, H, C1, d, 0, a, nws, None, None)),
        "gat_fwd_train": (gs, gw, lambda nsave, nws: L.digat_gat_fwd_train(*[a] * 7, 0.2, 1, B, n, d, a, nsave, a, nws, None)),
        "gat_bwd": (gs, gw, lambda nsave, nws: L.digat_gat_bwd(*[a] * 7, 0.2, a, nsave, *[a] * 5, B, n, d, a, nws, None)),
    }
    cases = []
    for name, (nsave, nws, call) in entries.items():
        cases += [(name + " short save", call(nsave - 1, BIG)), (name + " short workspace", call(BIG, nws - 1))]
    cases += [("gat_fwd short workspace", L.digat_gat_fwd(*[a] * 7, B, n, d, a, L.digat_gat_workspace_bytes(B, n, d) - 1, None)),
              ("xattn_pairwise_bwd short workspace",
               L.digat_xattn_pairwise_bwd(*[a] * 11, 0.2, *[a] * 4, 0, B, n, d, a, L.digat_xattn_pairwise_bwd_workspace(B, n, d) - 1, None))]
    return cases


def test_training_entries_refuse_a_buffer_one_byte_short_without_a_device():
    _lib, L = _lib_built()
    for q in ("digat_xattn_train_save_bytes", "digat_xattn_train_workspace_bytes", "digat_xattn_pairwise_bwd_workspace", "digat_gat_train_save_bytes",
              "digat_gat_train_workspace_bytes", "digat_gat_workspace_bytes", "digat_news_ctx_train_save_bytes",
              "digat_news_ctx_train_workspace_bytes", "digat_user_ctx_train_save_bytes", "digat_user_ctx_train_workspace_bytes"):
        assert hasattr(L, q) and q in _lib.EXPORTED, q
    cases = short_buffer_cases(L)
    assert len(cases) == 18
    assert dict(cases) == {what: WORKSPACE for what, _ in cases}
