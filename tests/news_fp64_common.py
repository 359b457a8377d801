"""Shared by tests/test_news_fp64_cpu.py and tests/test_hip_news_fp64.py: the fp64 references of the two DIGAT news encoders (MSA:
oracle/news_oracle.py on double parameters; CNN: the stock module cast to double), the case lists both files run, the inputs of a
case, and the comparison of this pipeline.  The CPU file pins the references to the golden fixtures and holds the stock fp32 modules
to a quarter of the tolerance on every case listed here; the GPU file holds the HIP kernels to the whole of it."""
import copy
import types
import zlib
from typing import NamedTuple

import numpy as np
import torch

from test_cnn_cpu import cnn_encoder
from test_hip_nrms import MASKS, make_mask  # noqa: F401  (the mask kinds of the NRMS sweep: live, prefix, holes, one, none, mixed)

OUT_TOL = dict(rtol=1e-5, atol=2e-6)      # the project's figures for this pipeline (tests/test_hip_news.py): the news representation ...
GRAD_TOL = dict(rtol=2e-4, atol=2e-6)     # ... and every gradient of a training step


def close(got, want, what, rtol=1e-5, atol=2e-6):
    """tests/test_hip_news.py:_close: relative to the larger of |want| and 5 % of the tensor's scale.  Returns the worst err / tol."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    scale = max(float(np.abs(want).max()), 1e-12)
    err = np.abs(got - want)
    tol = atol + rtol * np.maximum(np.abs(want), 0.05 * scale)
    ratio = float((err / tol).max())
    assert not (err > tol).any(), f"{what}: max|diff| {err.max():.3e} (scale {scale:.3e}), worst err/tol {ratio:.3f}"
    return ratio


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class MsaCase(NamedTuple):
    T: int
    Lw: int
    heads: int
    dk: int
    dm: int
    att: int
    V: int
    kind: str = "mixed"


class CnnCase(NamedTuple):
    T: int
    Lw: int
    dm: int
    Kc: int
    att: int
    V: int
    method: str
    window: int
    kind: str = "mixed"


# One (heads, d_k) of every KS = ceil(d_k / 4) = 1..8 of msa_attention_mfma_kernel<KS>; head counts below, equal to and above the four
# waves of a workgroup (two in the backward) and no multiple of them; d_k = 3 and 25 are no multiple of 4.
HEADS_DK = [(4, 3), (1, 8), (5, 12), (4, 16), (4, 20), (2, 24), (4, 25), (5, 32), (16, 25)]

# MSA inference.  Lw: one word; 15 | 16 | 17 and 31 | 32 the edges of the 16-row tiles; 32 | 33 the switch from the matrix-core kernel to
# msa_attention_kernel; 43 | 44 the two sides of 64 KiB of dynamic LDS at d_k = 25 (16 (2 Lw d_k + Lw (Lw + 1)) = 64 672 | 66 880 B);
# 50; 64 the limit, where (1, 32) asks for 132 096 B, the largest request of the contract.
MSA_LW = [1, 15, 16, 17, 31, 32, 33, 43, 44, 50, 64]
MSA_INFER = [MsaCase(T, Lw, h, dk, 32, 12, 60) for Lw in MSA_LW for h, dk in HEADS_DK + ([(1, 32)] if Lw == 64 else []) for T in (1, 3, 37)]

# The projections' routes (digat_gemm_plan.h, gemm_plan's rules by number).  With T Lw >= 2048, hd % 80 == 0 and dm >= 32 the Q|K|V
# product takes the token ids as its row list: rule 6, three strips a tile, and a row list keeps 128-row tiles -> STRIP_3_BF16 for all
# four; affine1 on A1's image (no row list, fewer than 400 workgroups): rule 6 -> STRIP_1_BF16_64 for all four (att padded to 160, 80,
# 320, 80 columns).
MSA_ROWLIST = [MsaCase(129, 16, 4, 20, 64, 100, 60),     # 2 064 rows
               MsaCase(70, 32, 4, 20, 36, 20, 60),       # 2 240 rows, dm no multiple of 16
               MsaCase(48, 44, 16, 25, 32, 256, 60),     # 2 112 rows into msa_attention_kernel above 64 KiB of LDS
               MsaCase(33, 64, 5, 32, 300, 12, 60)]      # 2 112 rows, the production dm
# The same shapes just below 2 048 rows: no kernel of rules 2-4 takes a row list, the embeddings are gathered first.  Q|K|V: dm = 64 and
# 32 (k0 % 16 == 0) rule 4 -> SKINNY_1 (192 tiles) and SKINNY_2 (960 tiles); dm = 36 and 300 rule 7 -> F32_64 (three segments of a
# multiple of 80 columns).  affine1: rule 3 would run on the image but takes no row list, so news_pool_fwd keeps the plain launch, whose
# att % 80 != 0 -> rule 7, F32_32, for all four.
MSA_GATHER = [c._replace(T=2047 // c.Lw) for c in MSA_ROWLIST]

# MSA training pair (Lw <= 32).  V = 20: tokens repeat inside and across titles, so the word table's gradient sums several rows.
MSA_TRAIN_LW = [1, 15, 16, 17, 31, 32]
MSA_TRAIN = [MsaCase(T, Lw, h, dk, 32, 12, 20) for Lw in MSA_TRAIN_LW for h, dk in HEADS_DK for T in (1, 9)]
# >= 2 048 token rows: the matrix-core products of the backward (row_grad padded to 80 columns; x3_ok for affine1 when att % 8 == 0)
MSA_TRAIN_BIG = [MsaCase(140, 16, 5, 16, 64, 100, 20), MsaCase(70, 32, 4, 20, 36, 20, 20)]
# a title masked throughout, alone in its batch
MSA_TRAIN_NONE = [MsaCase(1, 16, 4, 20, 32, 12, 20, "none"), MsaCase(1, 31, 5, 12, 32, 12, 20, "none")]

# CNN.  cnn_conv_tiled_kernel packs tpt = 128 / Lw titles a tile: Lw 16 -> 8, 17 18 -> 7, 21 -> 6, 22 25 -> 5, 26 31 32 -> 4, 33 42 -> 3,
# 43 63 64 -> 2: both sides of every change.  Lw = 1, 2, 3 are shorter than the 5 and 7 tap windows.  Lw = 16 with 7 taps fills
# CNN_MAX_AROWS = 176 rows exactly.
CNN_LW = [1, 2, 3, 15, 16, 17, 18, 21, 22, 25, 26, 31, 32, 33, 42, 43, 63, 64]
WINDOWS = [("naive", 1), ("naive", 3), ("naive", 5), ("naive", 7), ("group3", 3)]
CNN_SHAPES = [(32, 132), (36, 24)]        # (dm, Kc): Kc = 132 gives two 128-column tiles, the second ragged


def tiled_T(Lw):
    """The smallest T with T Lw >= 2048 whose last tile of 128 / Lw titles is ragged."""
    T, tpt = -(-2048 // Lw), 128 // Lw
    while T % tpt == 0:
        T += 1
    return T


def _cnn_infer_Ts(Lw):
    if Lw >= 16:
        return (5, tiled_T(Lw))           # the plain kernel, the tiled one
    return (5, 140) if Lw == 15 else (5,)  # 2 100 rows of 15 words stay on the plain kernel (Lw < 16); their affine1 runs on the image


CNN_INFER = [CnnCase(T, Lw, dm, Kc, 12, 60, m, w) for Lw in CNN_LW for m, w in WINDOWS for dm, Kc in CNN_SHAPES for T in _cnn_infer_Ts(Lw)]
CNN_TRAIN_LW = [1, 3, 15, 16, 17, 22, 31, 32]
CNN_TRAIN = [CnnCase(T, Lw, dm, Kc, 12, 20, m, w) for Lw in CNN_TRAIN_LW for m, w in WINDOWS for dm, Kc in CNN_SHAPES for T in (1, 9)]
# >= 2 048 rows, one per window: the forward and the flipped-weight input gradient (K = Kc >= 32) both run tiled, last tile ragged
CNN_TRAIN_BIG = [CnnCase(tiled_T(Lw), Lw, 36, 132, 12, 20, m, w) for (m, w), Lw in zip(WINDOWS, (32, 22, 17, 16, 31))]

# Permutation and poisoned scratch: per encoder one case on the tiled / row-list route and one on the plain one, att = 100 and 12 (`pre`
# has 60 and 68 padded columns); Lw <= 32 so that the training pair runs them too.  The permutation check adds the long-title kernels.
MSA_PAIR = [MsaCase(129, 16, 4, 20, 64, 100, 60), MsaCase(9, 17, 5, 12, 32, 12, 60)]
MSA_PERM = MSA_PAIR + [MsaCase(48, 44, 16, 25, 32, 256, 60), MsaCase(7, 33, 4, 3, 32, 12, 60)]
CNN_PAIR = [CnnCase(129, 16, 36, 132, 100, 60, "naive", 7), CnnCase(9, 17, 32, 24, 12, 60, "group3", 3)]
CNN_PERM = CNN_PAIR + [CnnCase(tiled_T(43), 43, 32, 132, 12, 60, "naive", 3)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _rng(case):
    return np.random.default_rng(zlib.crc32(repr(tuple(case)).encode()))


def _titles(case, out_dim, rng):
    """Token ids over the whole of [0, V), under padding too (MSA attends over padding; both encoders convolve / project it), the mask
    and a cotangent for the training checks."""
    text = torch.from_numpy(rng.integers(0, case.V, size=(case.T, case.Lw)).astype(np.int64))
    mask = torch.from_numpy(make_mask(case.kind, case.T, case.Lw, rng))
    R = torch.from_numpy(rng.standard_normal((case.T, out_dim)).astype(np.float32))
    return text, mask, R


def msa_inputs(case):
    """(state as numpy, text int64 [T, Lw], mask uint8 [T, Lw], cotangent fp32 [T, heads d_k]) of an MsaCase."""
    from digat_amd import synthetic
    rng = _rng(case)
    state = synthetic.make_msa_state(case.V, case.dm, case.heads, case.dk, case.att, seed=int(rng.integers(1 << 30)))
    return (state, *_titles(case, case.heads * case.dk, rng))


def msa_encoder(case, state, dropout=0.0):
    """newsEncoders.MSA on the CPU with the case's weights."""
    from digat_amd import newsEncoders
    cfg = types.SimpleNamespace(vocabulary_size=case.V, word_embedding_dim=case.dm, max_title_length=case.Lw, dropout_rate=dropout,
                                MSA_head_num=case.heads, MSA_head_dim=case.dk, attention_dim=case.att)
    enc = newsEncoders.MSA(cfg)
    res = enc.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return enc


def cnn_inputs(case):
    """(CPU encoder fp32 with dropout 0, text, mask, cotangent fp32 [T, Kc]) of a CnnCase."""
    from digat_amd import synthetic
    rng = _rng(case)
    state = synthetic.make_cnn_state(case.V, case.dm, case.Kc, case.att, case.method, case.window, seed=int(rng.integers(1 << 30)))
    enc = cnn_encoder(case.V, case.dm, case.Kc, case.att, case.Lw, case.method, case.window, state, dropout=0.0)
    return (enc, *_titles(case, case.Kc, rng))


# ---- references ------------------------------------------------------------------------------------------------------------------
def fp64_params(state):
    """A state dict (numpy or tensors) as double leaves that require a gradient: what msa_fp64 differentiates."""
    return {k: torch.as_tensor(v).detach().double().clone().requires_grad_(True) for k, v in state.items()}


def msa_fp64(state, text, mask, heads):
    """oracle.news_oracle.msa_forward on the parameters cast to double (the oracle is dtype-agnostic).  Double leaves (fp64_params) pass
    through the cast unchanged, so their .grad is the fp64 gradient."""
    from oracle import news_oracle
    p = {k: torch.as_tensor(v).double() for k, v in state.items()}
    return news_oracle.msa_forward(p, torch.as_tensor(text).long(), torch.as_tensor(mask), heads)


def msa_h_fp64(state, text, heads):
    """relu(softmax(Q K^T / sqrt(d_k)) V) [T, Lw, heads d_k] in fp64, written out independently of the oracle (einsum per head): what
    an all-masked title's representation is the plain mean of."""
    p = {k: torch.as_tensor(v).double() for k, v in state.items()}
    x = p["word_embedding.weight"][torch.as_tensor(text).long()]
    T, Lw, _ = x.shape
    q = (x @ p["multiheadSelfattention.W_Q.weight"].T + p["multiheadSelfattention.W_Q.bias"]).view(T, Lw, heads, -1)
    k = (x @ p["multiheadSelfattention.W_K.weight"].T).view(T, Lw, heads, -1)
    v = (x @ p["multiheadSelfattention.W_V.weight"].T + p["multiheadSelfattention.W_V.bias"]).view(T, Lw, heads, -1)
    s = torch.einsum("tihc,tjhc->thij", q, k) / float(q.shape[-1]) ** 0.5
    return torch.relu(torch.einsum("thij,tjhc->tihc", torch.softmax(s, dim=3), v)).reshape(T, Lw, -1)


def cnn_fp64_module(encoder):
    """A double copy of a CPU encoder built by test_cnn_cpu.cnn_encoder, in ``encoder``'s mode."""
    return copy.deepcopy(encoder).cpu().double()


def cnn_fp64(encoder, text, mask):
    """copy.deepcopy(encoder).double().forward_stock(...) on text / mask [T, Lw] -> [T, Kc].  An encoder that is double already (a
    cnn_fp64_module the caller keeps for its parameters' .grad) is used as it is."""
    ref = encoder if next(encoder.parameters()).dtype == torch.float64 else cnn_fp64_module(encoder)
    return ref.forward_stock(torch.as_tensor(text).long().unsqueeze(0), torch.as_tensor(mask).unsqueeze(0)).squeeze(0)
