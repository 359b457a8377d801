"""CPU suite for the news encoders' C ABI (digat_msa_* / digat_cnn_*): the six size queries pinned per shape, and the status a bad
digat_msa_* call returns, in the order the entry points check (tests/test_cnn_cpu.py pins the same for digat_cnn_*).  No device: a
size query is host arithmetic and every status case fails before anything is read or launched."""
import ctypes

import pytest

# (T, Lw, dm, heads, dk, att) -> (workspace, train_save, train_workspace WITH `wcat`).  The byte counts are ABI: Python sizes its
# buffers with them.  The third figure is the training workspace while its layout still held `wcat`, a [3 hd, dm] fp32 scratch that
# no launch had read since the stacked weights are split from their three homes: the query returns that figure minus
# align_up(3 * hd * dm * 4, 256), and the test below spells the subtraction out.
MSA_SIZES = {
    (6400, 32, 300, 16, 25, 256): (1818624000, 1880883200, 1680923904),
    (65238, 32, 300, 16, 25, 256): (18538030080, 19172665344, 16202142976),
    (300, 32, 300, 16, 25, 256): (85248000, 88166400, 137879552),
    (140, 20, 64, 5, 16, 100): (6092800, 6283264, 6612480),
    (1, 1, 16, 1, 4, 4): (1280, 1792, 65792),
    (0, 16, 32, 2, 8, 12): (0, 0, 95744),
}
# (T, Lw, dm, Kc, taps, att) -> (workspace, train_save, train_workspace)
CNN_SIZES = {
    (6400, 32, 300, 400, 3, 256): (589824000, 590643200, 1245260032),
    (4099, 32, 300, 400, 3, 256): (377763840, 378288640, 811752960),
    (72, 32, 300, 396, 5, 256): (6598656, 6607872, 32632064),
    (1, 1, 16, 8, 1, 4): (768, 1024, 82944),
    (0, 32, 300, 400, 3, 256): (0, 0, 0),
}


def _lib_built():
    from digat_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


@pytest.mark.parametrize("shape", list(MSA_SIZES))
def test_msa_size_queries_are_pinned(shape):
    _, L = _lib_built()
    T, Lw, dm, heads, dk, att = shape
    workspace, save, train_ws_with_wcat = MSA_SIZES[shape]
    wcat = (3 * heads * dk * dm * 4 + 255) // 256 * 256                       # 1 440 000 bytes at 16 x 25 heads, dm 300
    got = (L.digat_msa_workspace_bytes(*shape), L.digat_msa_train_save_bytes(*shape), L.digat_msa_train_workspace_bytes(*shape))
    assert got == (workspace, save, train_ws_with_wcat - wcat), shape


@pytest.mark.parametrize("shape", list(CNN_SIZES))
def test_cnn_size_queries_are_pinned(shape):
    _, L = _lib_built()
    got = (L.digat_cnn_workspace_bytes(*shape), L.digat_cnn_train_save_bytes(*shape), L.digat_cnn_train_workspace_bytes(*shape))
    assert got == CNN_SIZES[shape], shape


OK, ARG, SHAPE, WORKSPACE = 0, 1, 2, 3
BIG = 1 << 30


def msa_status_cases(_lib, L):
    """[(what, returned status)] of digat_msa_fwd / digat_msa_fwd_train / digat_msa_bwd on calls that end before any launch."""
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)                                      # a non-null HOST address: every check below fails before it is read

    def params(dm=300, heads=16, dk=25, att=256):
        P = _lib.MsaParams(word_embedding_dim=dm, head_num=heads, head_dim=dk, attention_dim=att)
        for k in ("word_embedding", "W_Q", "b_Q", "W_K", "W_V", "b_V", "A1", "b1", "a2"):
            setattr(P, k, a)
        return P

    def fwd(P="default", text=a, T=4, Lw=32, ws=a, nws=BIG):
        return L.digat_msa_fwd(params() if P == "default" else P, text, a, a, T, Lw, ws, nws, None)

    def fwd_train(P="default", out=a, p=0.2, T=4, Lw=32, nsave=BIG, nws=BIG):
        return L.digat_msa_fwd_train(params() if P == "default" else P, a, a, out, p, 1, T, Lw, a, nsave, a, nws, None)

    def bwd(P="default", dout=a, T=4, Lw=32, nsave=BIG, ld=300, da2=a, nws=BIG):
        return L.digat_msa_bwd(params() if P == "default" else P, a, a, dout, 0.2, a, nsave, a, ld, a, a, a, a, a, a, a, da2, T, Lw, a, nws, None)

    # inference takes att = 6 and Lw = 33: those two calls carry a 16-byte workspace, so that they too end before a launch.
    # digat_msa_bwd at T = 0 is left out on purpose: it zero-fills the gradient buffers (hipMemsetAsync), which host addresses and
    # a machine without a device cannot serve; tests/test_hip_news.py asserts it on the GPU.
    cases = [("fwd NULL params", fwd(P=None)), ("fwd NULL tokens", fwd(text=None)), ("fwd NULL workspace", fwd(ws=None)), ("fwd T < 0", fwd(T=-1)),
             ("fwd Lw = 0", fwd(Lw=0)), ("fwd dm = 30", fwd(P=params(dm=30))), ("fwd dk = 33", fwd(P=params(dk=33))),
             ("fwd att = 0", fwd(P=params(att=0))), ("fwd Lw = 65", fwd(Lw=65)), ("fwd att = 6, 16-byte workspace", fwd(P=params(att=6), nws=16)),
             ("fwd Lw = 33, 16-byte workspace", fwd(Lw=33, nws=16)), ("fwd 16-byte workspace", fwd(nws=16)), ("fwd T = 0", fwd(T=0, nws=0))]
    for name, fn in (("fwd_train", fwd_train), ("bwd", bwd)):
        cases += [(name + " NULL params", fn(P=None)), (name + " T < 0", fn(T=-1)), (name + " Lw = 0", fn(Lw=0)),
                  (name + " dm = 30", fn(P=params(dm=30))), (name + " dk = 33", fn(P=params(dk=33))), (name + " att = 0", fn(P=params(att=0))),
                  (name + " att = 6", fn(P=params(att=6))), (name + " Lw = 33", fn(Lw=33)), (name + " 16-byte workspace", fn(nws=16)),
                  (name + " 16-byte save", fn(nsave=16)), (name + " 16-byte save and workspace", fn(nsave=16, nws=16))]
    cases += [("fwd_train NULL out", fwd_train(out=None)), ("fwd_train p_drop = 1", fwd_train(p=1.0)), ("fwd_train p_drop < 0", fwd_train(p=-0.1)),
              ("fwd_train p_drop = 1, dm = 30", fwd_train(p=1.0, P=params(dm=30))), ("fwd_train T = 0", fwd_train(T=0, nsave=0, nws=0)),
              ("fwd_train T = 0, Lw = 33", fwd_train(T=0, Lw=33)),
              ("bwd NULL dout", bwd(dout=None)), ("bwd NULL da2", bwd(da2=None)), ("bwd ld = 304", bwd(ld=304)),
              ("bwd ld = 320, 16-byte workspace", bwd(ld=320, nws=16)), ("bwd ld = 304, Lw = 33", bwd(ld=304, Lw=33)),
              ("bwd ld = 304, 16-byte save", bwd(ld=304, nsave=16))]
    return cases


# what each call returned before the news encoders' host code was brought to one carve per entry (recorded from that build, not
# reasoned): inference takes Lw <= 64 and any att > 0, the training pair Lw <= 32 and att % 4 == 0; a bad leading dimension of
# row_grad is an argument error found after the shape; the save buffer is checked before the workspace.
MSA_STATUS = {
    "fwd NULL params": ARG, "fwd NULL tokens": ARG, "fwd NULL workspace": ARG, "fwd T < 0": ARG, "fwd Lw = 0": ARG,
    "fwd dm = 30": SHAPE, "fwd dk = 33": SHAPE, "fwd att = 0": SHAPE, "fwd Lw = 65": SHAPE,
    "fwd att = 6, 16-byte workspace": WORKSPACE, "fwd Lw = 33, 16-byte workspace": WORKSPACE, "fwd 16-byte workspace": WORKSPACE,
    "fwd T = 0": OK,                                                 # no title: nothing is launched
    "fwd_train NULL params": ARG, "fwd_train NULL out": ARG, "fwd_train T < 0": ARG, "fwd_train Lw = 0": ARG,
    "fwd_train p_drop = 1": ARG, "fwd_train p_drop < 0": ARG, "fwd_train p_drop = 1, dm = 30": ARG,
    "fwd_train dm = 30": SHAPE, "fwd_train dk = 33": SHAPE, "fwd_train att = 0": SHAPE, "fwd_train att = 6": SHAPE, "fwd_train Lw = 33": SHAPE,
    "fwd_train 16-byte workspace": WORKSPACE, "fwd_train 16-byte save": WORKSPACE, "fwd_train 16-byte save and workspace": WORKSPACE,
    "fwd_train T = 0": OK, "fwd_train T = 0, Lw = 33": SHAPE,
    "bwd NULL params": ARG, "bwd NULL dout": ARG, "bwd NULL da2": ARG, "bwd T < 0": ARG, "bwd Lw = 0": ARG,
    "bwd dm = 30": SHAPE, "bwd dk = 33": SHAPE, "bwd att = 0": SHAPE, "bwd att = 6": SHAPE, "bwd Lw = 33": SHAPE,
    "bwd ld = 304": ARG, "bwd ld = 304, Lw = 33": SHAPE, "bwd ld = 304, 16-byte save": ARG,
    "bwd ld = 320, 16-byte workspace": WORKSPACE,                    # the padded leading dimension (digat_msa_row_grad_ld) is accepted
    "bwd 16-byte workspace": WORKSPACE, "bwd 16-byte save": WORKSPACE, "bwd 16-byte save and workspace": WORKSPACE,
}


def test_msa_abi_without_a_device():
    _lib, L = _lib_built()
    for n in ("digat_msa_split_bytes", "digat_split_msa_weights", "digat_msa_workspace_bytes", "digat_msa_fwd", "digat_msa_train_save_bytes",
              "digat_msa_train_workspace_bytes", "digat_msa_fwd_train", "digat_msa_bwd", "digat_msa_row_grad_ld"):
        assert hasattr(L, n) and n in _lib.EXPORTED, n
    got = dict(msa_status_cases(_lib, L))
    assert got == MSA_STATUS
    assert L.digat_msa_row_grad_ld(64, 32, 300) == 320 and L.digat_msa_row_grad_ld(63, 32, 300) == 300
