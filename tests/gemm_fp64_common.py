"""Shared by tests/test_gemm_fp64_cpu.py and tests/test_gemm_fp64_gpu.py: every GEMM kernel launch_gemm can launch, alone, against a
float64 product.

The pieces: a ctypes mirror of GemmArgs (digat_amd/csrc/digat_gemm_plan.h), a table of launches (CASES) that names the kernel
each is to run, operands drawn as the other GEMM tests draw them (standard normal x, w / sqrt(K)), a float64 reference of what the
kernels' epilogues state, decoders for the two reduced output formats, float64 emulations of the reduced product sets, and the
bound every output element is held to.  The CPU file proves on the launch plan that the table reaches every kernel and that the
bounds separate the product sets; the GPU file runs the table through digat_gemm_launch.

Bounds (check_segment), none fitted to a measurement:

  full   full-precision products (fp32 MFMA, skinny, bf16x6 with six products, fp16x3 with three): the rule of
         tests/test_hip_parity.py (test_linear_mfma_f32, test_linear_bf16x6_is_fp32_grade), T = 2e-6 sqrt(K) + 1e-5 |pre|, on the
         value `pre` in front of the epilogue.  relu, the adds and the dropout mask are applied to both sides and do not enlarge
         it.  EPI_GATE: out = s(pre) e0 + (1 - s(pre)) e1 with |s'| <= 1/4, so |d out| <= |e0 - e1| / 4 |d pre| <= max(|e0|, |e1|)
         |d pre| / 2: the bound is T max(|e0|, |e1|) (the gate cases draw |e0|, |e1| >= 1/2, so that the fp32 rounding of e2 + out
         stays far below it).
  x3     bf16x6 with x3_segs: x = x1 + x2 + x3 and w = w1 + w2 + w3 exactly, every piece the 8 leading bits of what the pieces in
         front of it left, by TRUNCATION (split3f): |x - x1| < 2^-7 |x|, |x2| < 2^-7 |x|, |x3| < 2^-14 |x|, |x1 + x2| <= |x|, the
         same for w.  The kernel keeps x1 w1 + x2 w1 + x1 w2; what it drops is x w - kept = x3 w + x2 w2 + (x1 + x2) w3, each
         below 2^-14 |x| |w|: |dropped| < 3 2^-14 sum_k |x_k| |w_k| (c = 3, p = 14).  fp16x3 computes hi hi + lo hi + hi lo with
         x3_segs set or clear (the kernel's `lite < 2` branch): its x3 is its full product, held to `full`.
  x1     bf16x6 with x1_segs keeps x1 w1: dropped = (x - x1) w + x1 (w - w1), < 2 2^-7 sum_k |x_k| |w_k| (c = 2, p = 7).  fp16x3
         keeps hi hi: x_hi is 2^4 x truncated to fp16's 11 bits (|x - x_hi| < 2^-10 |x|), w_hi is 2^10 w rounded to nearest
         (|w - w_hi| <= 2^-11 |w|), |x_hi| <= |x|: dropped < 3 2^-11 sum_k |x_k| |w_k| (c = 3, p = 11; operands whose scaled
         value is an fp16 subnormal, |x| < 3.8e-6, add at most 2^-24 / 16 |w| each: nothing at these sizes).
         x3 and x1 stand on top of `full`; the sums are taken in float64.
  bf16   a bf16_segs output is the round-to-nearest-even of a value within the segment's bound: half a bf16 ulp, 2^-8 |want|, more.
  e4m3   a fp8_segs output is rows of [nseg codes | nseg / 80 fp32 scales | pad].  The scale of a (row, 80-column strip) block is
         its absmax / 448: held to the largest bound of the block's elements, / 448.  A decoded element, code x stored scale, lies
         within half an e4m3 ulp at its magnitude: 2^-4 |want| for normals (3 mantissa bits), and half the subnormal step 2^-9,
         2^-10, times the scale, below the smallest normal 2^-6; plus the segment's bound.
  f8c    the fp16-fp8c kernel: the bounds of tests/test_hip_fp8c.py (test_f16f8c_linear_against_its_quantiser_and_fp64):
         |err| <= 2^-12 sum_k |x_k w_k| + 1e-6 of the row's largest |pre| against fp64, and 1e-6 of the row's largest |pre| against
         the restated quantiser (emulate_f16f8c), which leaves the kernel the accumulation order only; the fp32 store of an
         epilogue that adds (relu + e0, + e0, + y) rounds once more: 2^-24 |want| on top of the second.
"""
import ctypes as C
import functools
import math
import os
import re
import zlib

import numpy as np
import torch

from conftest import REPO

PLAN_H = os.path.join(REPO, "digat_amd", "csrc", "digat_gemm_plan.h")
_p, _l, _i = C.c_void_p, C.c_long, C.c_int


class GemmArgs(C.Structure):
    """GemmArgs of digat_amd/csrc/digat_gemm_plan.h, field for field (tests/test_gemm_fp64_cpu.py holds it to the header's layout)."""
    _fields_ = [("a0", _p), ("lda0", _l), ("k0", _i), ("a1", _p), ("lda1", _l),
                ("w", _p * 3), ("bias", _p * 3), ("y", _p * 3), ("ldy", _l),
                ("nseg", _i), ("nsegs", _i), ("M", _i), ("K", _i), ("transW", _i), ("epi", _i),
                ("e0", _p), ("lde0", _l), ("e1", _p), ("lde1", _l), ("e2", _p), ("lde2", _l),
                ("mtiles", _i), ("ntiles", _i), ("wsplit", _p),
                ("radd", _p), ("radd_seg", _i), ("rows_per_b", _i), ("exec_rows", _p),
                ("rowidx", _p), ("nrows_dev", _p), ("gather_only", _i), ("m_dispatch", _i),
                ("x3_segs", _i), ("x1_segs", _i), ("bf16_segs", _i), ("fp8_segs", _i), ("ldy8", _l),
                ("format", _i), ("range_flag", _p), ("dmask", _p), ("lddm", _l), ("dscale", C.c_float), ("dmask_cols", _i),
                ("ragged", _i), ("strips", _i)]


FIELDS = [f[0] for f in GemmArgs._fields_]
EPI = {None: 0, "relu": 1, "gate": 2, "gate_e2": 2, "accum": 3, "add_e0": 4}
KIND = {None: 1, "proj": 0}                    # DIGAT_KERNEL_LINEAR, DIGAT_KERNEL_PROJ (include/digat_hip.h)
BF16X6, F16X3, F16F8C = 0, 1, 2
DSCALE = 1.25                                  # 1 / (1 - 0.2): the dropout of the layers
BIG = 1 << 30                                  # m_dispatch: the kernels of a launch of 2 048 rows and more


@functools.lru_cache(maxsize=None)
def kernel_ids():
    """GemmKernel by name: GEMM_NONE, GEMM_PER_SEGMENT, then DIGAT_GEMM_KERNELS in the header's order."""
    text = open(PLAN_H).read()
    block = text[text.index("#define DIGAT_GEMM_KERNELS(X)"):text.index("enum GemmKernel")]
    names = ["NONE", "PER_SEGMENT"] + re.findall(r"X\((\w+),", block)
    return {n: i for i, n in enumerate(names)}


def kernel_name(kid):
    return {v: k for k, v in kernel_ids().items()}[kid]


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# name -> fields.  kernel: the GemmKernel the launch is to run; ragged_plan: GemmPlan::ragged (the ragged instantiation and its tile
# order).  M, nseg, nsegs, K as in GemmArgs.  Optional: fmt (a split image in that format), kind, k0 (two-operand A: [a0 | a1]),
# transW, epi, bias (False: NULL), radd (rows_per_b; on segment min(1, nsegs - 1)), rows ("subset": sorted, "perm", "empty", "all":
# sorted, every row), gather (gather_only: the list indexes A alone), bf16_segs / fp8_segs / x3_segs / x1_segs (segment masks),
# dmask (dmask_cols), m_dispatch, ragged, big (an activation of 5000: beyond fp16x3's 4094).
CASES = {}


def _add(name, kernel, M, nseg, nsegs, K, **f):
    assert name not in CASES, name
    CASES[name] = dict(kernel=kernel, M=M, nseg=nseg, nsegs=nsegs, K=K, **f)


def _epis(prefix, kernel, M, nseg, nsegs, K, epis, **f):
    for e in epis:
        _add(f"{prefix}_{e}", kernel, M, nseg, nsegs, K, epi=e, **f)


def _fp32_mfma():
    # (kernel, fields that reach it, row counts: 1 / a tile / a tile and a tail, (nseg, nsegs), wider (nseg, nsegs))
    fam = (("F32_32", {}, (1, 32, 40), (100, 1), (128, 2)),
           ("F32_64", {"radd": 7}, (1, 64, 100), (80, 2), (160, 3)),            # below 2 048 rows the skinny kernel takes what has no radd
           ("F32_128", {"m_dispatch": BIG}, (1, 128, 200), (100, 1), (80, 3)),
           ("F32_128_PROJ", {"m_dispatch": BIG, "kind": "proj"}, (1, 128, 200), (100, 1), (80, 3)))
    for kern, f, Ms, (n, s), (n2, s2) in fam:
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, n, s, 36, **f)
        for K in (4, 32, 48):
            _add(f"{p}_k{K}", kern, Ms[2], n, s, K, **f)
        _add(f"{p}_wide", kern, Ms[2], n2, s2, 36, **f)
        _add(f"{p}_nobias", kern, Ms[2], n, s, 36, bias=False, **f)
        _add(f"{p}_two_operand", kern, Ms[2], n, s, 36, k0=16, **f)
        _add(f"{p}_two_operand_k4", kern, Ms[2], n, s, 8, k0=4, **f)
        _epis(p, kern, Ms[2], n, s, 36, ("relu", "gate", "gate_e2", "accum"), **f)
        if "radd" not in f:
            _add(f"{p}_radd", kern, Ms[2], n, s, 36, radd=7, **f)
    _add("f32_32_n17", "F32_32", 40, 17, 1, 36)
    _add("f32_32_transW", "F32_32", 40, 100, 1, 36, transW=1)
    _add("f32_32_transW_relu", "F32_32", 40, 17, 1, 48, transW=1, epi="relu")
    _add("f32_64_transW", "F32_64", 100, 80, 2, 48, transW=1)                  # two segments: not the skinny transpose kernel
    _add("f32_128_transW", "F32_128", 200, 100, 1, 36, transW=1, m_dispatch=BIG)
    _add("f32_128_proj_transW", "F32_128_PROJ", 200, 80, 1, 48, transW=1, m_dispatch=BIG, kind="proj")
    _add("f32_128_short_k_image", "F32_128", 200, 80, 3, 16, fmt=F16X3, m_dispatch=BIG)      # K < 32: not the strip kernel
    _add("f32_128_gate_image", "F32_128", 200, 80, 1, 64, fmt=F16X3, m_dispatch=BIG, epi="gate", k0=32)
    for tiles, M in ((1, 32), (7, 200), (8, 256), (9, 260)):                   # the grid is rounded to 8, the tiles dealt over 8 XCDs
        _add(f"f32_32_tiles{tiles}", "F32_32", M, 64, 1, 32)
    _add("per_segment", "PER_SEGMENT", 40, 100, 2, 36)
    _add("per_segment_radd_big", "PER_SEGMENT", 200, 100, 3, 36, radd=7, m_dispatch=BIG, kind="proj")
    _add("per_segment_gate_e2", "PER_SEGMENT", 40, 17, 3, 36, epi="gate_e2", k0=16)


def _skinny():
    for kern, Ms, K in (("SKINNY_1", (1, 16, 17), 48), ("SKINNY_2", (1, 32, 40), 800)):
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, 80, 1, K)
        _add(f"{p}_three_strips", kern, Ms[2], 240, 1, K)
        _add(f"{p}_two_segments", kern, Ms[2], 160, 2, K)
        _add(f"{p}_three_segments", kern, Ms[2], 80, 3, K)
        _add(f"{p}_five_strips", kern, Ms[2], 400, 1, K)
        _add(f"{p}_nobias", kern, Ms[2], 80, 1, K, bias=False)
        _add(f"{p}_two_operand", kern, Ms[2], 80, 1, K, k0=K - 16)
        _epis(p, kern, Ms[2], 80, 2, K, ("relu", "gate", "gate_e2", "accum"))
    for K in (16, 32):
        _add(f"skinny_1_k{K}", "SKINNY_1", 17, 80, 1, K)
    _add("skinny_2_k816", "SKINNY_2", 40, 80, 1, 816)
    _add("skinny_2_wide", "SKINNY_2", 40, 19200, 1, 16)                        # 2 x 240 workgroups: 32-row tiles without a long K
    for kern, Ms, k0s in (("SKINNY_1_KTAIL", (1, 16, 17), (16, 32)), ("SKINNY_2_KTAIL", (1, 32, 40), (800,))):
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, 80, 1, k0s[0] + 4, k0=k0s[0])
        for k0 in k0s[1:]:
            _add(f"{p}_k{k0 + 4}", kern, Ms[2], 80, 1, k0 + 4, k0=k0)
        _add(f"{p}_three_segments", kern, Ms[2], 80, 3, k0s[0] + 4, k0=k0s[0])
        _add(f"{p}_five_strips_nobias", kern, Ms[2], 400, 1, k0s[0] + 4, k0=k0s[0], bias=False)
        _epis(p, kern, Ms[2], 80, 2, k0s[0] + 4, ("relu", "gate", "gate_e2", "accum"), k0=k0s[0])
    _add("skinny_2_ktail_wide", "SKINNY_2_KTAIL", 40, 19200, 1, 20, k0=16)
    for kern, Ms, Ks in (("SKINNY_TW_1", (1, 16, 17), (48, 16, 32)), ("SKINNY_TW_2", (1, 32, 40), (800, 816))):
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, 80, 1, Ks[0], transW=1)
        for K in Ks[1:]:
            _add(f"{p}_k{K}", kern, Ms[2], 80, 1, K, transW=1)
        _add(f"{p}_three_strips", kern, Ms[2], 240, 1, Ks[0], transW=1)
        _add(f"{p}_five_strips_nobias", kern, Ms[2], 400, 1, Ks[0], transW=1, bias=False)
        _epis(p, kern, Ms[2], 80, 1, Ks[0], ("relu", "gate", "gate_e2", "accum"), transW=1)
    _add("skinny_tw_2_wide", "SKINNY_TW_2", 40, 19200, 1, 16, transW=1)


def _skinny_split():
    for fname, fmt in (("F16", F16X3), ("BF16", BF16X6)):
        kern, Ms = f"SKINNY_SPLIT_{fname}_1", (1, 16, 17)
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, 80, 1, 40, fmt=fmt)
        for K in (8, 32, 48):
            _add(f"{p}_k{K}", kern, Ms[2], 80, 1, K, fmt=fmt)
        _add(f"{p}_three_strips", kern, Ms[2], 240, 1, 40, fmt=fmt)
        _add(f"{p}_two_segments", kern, Ms[2], 160, 2, 40, fmt=fmt)
        _add(f"{p}_three_segments", kern, Ms[2], 80, 3, 40, fmt=fmt)
        _add(f"{p}_five_strips", kern, Ms[2], 400, 1, 40, fmt=fmt)
        _add(f"{p}_nobias", kern, Ms[2], 80, 1, 40, fmt=fmt, bias=False)
        _add(f"{p}_two_operand", kern, Ms[2], 80, 1, 40, fmt=fmt, k0=32)
        _add(f"{p}_two_operand_k16", kern, Ms[2], 80, 1, 16, fmt=fmt, k0=8)
        _add(f"{p}_m_dispatch_1", kern, 100, 80, 1, 40, fmt=fmt, m_dispatch=1)
        _epis(p, kern, Ms[2], 80, 2, 40, ("relu", "gate", "gate_e2", "accum"), fmt=fmt)
        # 32-row tiles from ceil(M / 32) N / 80 = 320 workgroups: a wide N with a short K
        kern, Ms = f"SKINNY_SPLIT_{fname}_2", (1, 32, 40)
        p = kern.lower()
        for M in Ms:
            _add(f"{p}_m{M}", kern, M, 25600 if M <= 32 else 12800, 1, 8, fmt=fmt)
        _add(f"{p}_k40", kern, 40, 12800, 1, 40, fmt=fmt)
        _add(f"{p}_two_segments_nobias", kern, 40, 6400, 2, 8, fmt=fmt, bias=False)
        _add(f"{p}_two_operand", kern, 40, 12800, 1, 16, fmt=fmt, k0=8)
        _epis(p, kern, 40, 6400, 2, 8, ("relu", "gate", "gate_e2", "accum"), fmt=fmt)
    _add("skinny_split_f16_1_big", "SKINNY_SPLIT_F16_1", 17, 80, 1, 40, fmt=F16X3, big=True)
    _add("skinny_split_f16_2_big", "SKINNY_SPLIT_F16_2", 40, 12800, 1, 8, fmt=F16X3, big=True)


def _strip():
    D = {"m_dispatch": BIG}
    # 64-row tiles: few rows, no request for ragged tiles (bf16x6: no row list either)
    for fname, fmt in (("F16", F16X3), ("BF16", BF16X6)):
        for nsub, n1 in ((3, 240), (1, 80)):
            kern = f"STRIP_{nsub}_{fname}_64"
            p, f = kern.lower(), dict(fmt=fmt, **D)
            for M in (1, 64, 100):
                _add(f"{p}_m{M}", kern, M, n1, 1, 36, **f)
            for K in (32, 48):
                _add(f"{p}_k{K}", kern, 100, n1, 1, K, **f)
            if nsub == 3:
                _add(f"{p}_two_tiles_span_segments", kern, 100, 160, 3, 36, **f)
                _add(f"{p}_three_segments", kern, 100, 80, 3, 36, **f)
                _add(f"{p}_reduced", kern, 100, 80, 3, 48, x3_segs=2, x1_segs=4, **f)
                _add(f"{p}_outputs", kern, 100, 80, 3, 36, bf16_segs=2, fp8_segs=4, **f)
                _add(f"{p}_outputs_radd_reduced", kern, 100, 160, 3, 36, bf16_segs=2, fp8_segs=4, x3_segs=2, x1_segs=4, radd=7, **f)
            else:
                _add(f"{p}_two_strips", kern, 100, 160, 1, 36, **f)
                _add(f"{p}_four_strips", kern, 100, 320, 1, 36, **f)
                _add(f"{p}_five_strips", kern, 100, 400, 1, 36, **f)
                _add(f"{p}_two_segments", kern, 100, 80, 2, 36, **f)
                _add(f"{p}_reduced", kern, 100, 80, 2, 48, x3_segs=1, x1_segs=2, **f)
                _add(f"{p}_outputs", kern, 100, 80, 2, 36, bf16_segs=1, fp8_segs=2, **f)
                _add(f"{p}_fp8_five_strips_x1", kern, 100, 400, 1, 36, fp8_segs=1, x1_segs=1, **f)
            _add(f"{p}_nobias", kern, 100, n1, 1, 36, bias=False, **f)
            _epis(p, kern, 100, n1, 1, 36, ("relu", "accum", "add_e0"), **f)
            _add(f"{p}_radd", kern, 100, 80, nsub if nsub == 3 else 2, 36, radd=7, **f)
            if fmt == F16X3:
                for rows in ("subset", "perm", "empty", "all"):
                    _add(f"{p}_rows_{rows}", kern, 100, n1, 1, 36, rows=rows, epi="relu", **f)
                _add(f"{p}_gather", kern, 100, n1, 1, 36, rows="perm", gather=True, epi="add_e0", **f)
                _add(f"{p}_big", kern, 100, n1, 1, 36, big=True, **f)
            else:
                _add(f"{p}_dmask", kern, 100, n1, 1, 36, dmask=0, epi="add_e0", **f)
                _add(f"{p}_dmask_cols", kern, 100, n1, 1, 36, dmask=n1 - 60, **f)
    for tiles, M in ((1, 64), (7, 400), (8, 512), (9, 520)):
        _add(f"strip_3_f16_64_tiles{tiles}", "STRIP_3_F16_64", M, 240, 1, 32, fmt=F16X3, **D)
    # 128-row tiles: a bf16x6 launch with a row list; any launch that asks for ragged tiles and counts its workgroups at m_dispatch
    R = {"ragged": 1, **D}
    fam = (("STRIP_3_F16_FULL", F16X3, 3, R, {}), ("STRIP_3_F16", F16X3, 3, R, {"x3_segs": 2, "x1_segs": 4}), ("STRIP_1_F16", F16X3, 1, R, {}),
           ("STRIP_3_BF16", BF16X6, 3, {"rows": "all", **D}, {}), ("STRIP_1_BF16", BF16X6, 1, {"rows": "all", **D}, {}))
    for kern, fmt, nsub, reach, red in fam:
        p = kern.lower()
        shape = (80, 3) if nsub == 3 else (80, 1)
        f = dict(fmt=fmt, **reach, **red)
        for M in (1, 128, 200):
            _add(f"{p}_m{M}", kern, M, *shape, 36, **f)
        for K in (32, 48):
            _add(f"{p}_k{K}", kern, 200, *shape, K, **f)
        _add(f"{p}_nobias", kern, 200, *shape, 36, bias=False, **f)
        _epis(p, kern, 200, *shape, 36, ("relu", "accum", "add_e0"), **f)
        _add(f"{p}_radd", kern, 200, 80, 3 if nsub == 3 else 2, 36, radd=7, **f)
        if nsub == 3:
            _add(f"{p}_two_tiles_span_segments", kern, 200, 160, 3, 36, **f)
            _add(f"{p}_outputs", kern, 200, 80, 3, 36, bf16_segs=2, fp8_segs=4, **f)
        else:
            _add(f"{p}_two_strips", kern, 200, 160, 1, 36, **f)
            _add(f"{p}_two_segments_outputs", kern, 200, 80, 2, 36, bf16_segs=1, fp8_segs=2, **f)
            _add(f"{p}_reduced", kern, 200, 80, 2, 48, x3_segs=1, x1_segs=2, **f)
        g = {k: v for k, v in f.items() if k != "rows"}
        if fmt == BF16X6:
            if nsub == 3:
                _add(f"{p}_reduced", kern, 200, 80, 3, 48, x3_segs=2, x1_segs=4, **f)
            else:
                _add(f"{p}_four_strips", kern, 200, 320, 1, 36, **f)
                _add(f"{p}_five_strips", kern, 200, 400, 1, 36, **f)
            _add(f"{p}_by_ragged_request", kern, 200, *shape, 36, fmt=fmt, ragged=2, **D)
            _add(f"{p}_dmask", kern, 200, *shape, 36, dmask=0, epi="add_e0", **f)
            _add(f"{p}_dmask_cols", kern, 200, *shape, 36, dmask=20, **f)
        for rows in ("subset", "perm", "empty"):
            _add(f"{p}_rows_{rows}", kern, 200, *shape, 36, rows=rows, epi="relu", **g)
        _add(f"{p}_gather", kern, 200, *shape, 36, rows="perm", gather=True, epi="add_e0", **g)
        if fmt == F16X3:
            _add(f"{p}_rows_all", kern, 200, *shape, 36, rows="all", **g)
            _add(f"{p}_big", kern, 200, *shape, 36, big=True, **f)
    # ragged 240-column tiles: more than three strips, no multiple of three; both tile orders
    for kern, fmt, red in (("STRIP_3_F16_FULL", F16X3, {}), ("STRIP_3_F16", F16X3, {"x3_segs": 1, "x1_segs": 2}), ("STRIP_3_BF16", BF16X6, {})):
        for order in (1, 2):
            p = f"{kern.lower()}_ragged{order}"
            f = dict(fmt=fmt, ragged=order, ragged_plan=order, **D)
            for M in (1, 128, 200):
                _add(f"{p}_m{M}", kern, M, 320, 1, 36, **f, **({"x1_segs": 1} if red else {}))
            _add(f"{p}_five_strips", kern, 200, 400, 1, 48, **f, **({"x3_segs": 1} if red else {}))
            _add(f"{p}_ten_strips_two_segments", kern, 200, 400, 2, 32, radd=7, **f, **red)
            _add(f"{p}_nine_row_tiles", kern, 1100, 320, 1, 32, bias=False, **f, **({"x1_segs": 1} if red else {}))
            _add(f"{p}_relu_rows", kern, 200, 400, 1, 36, epi="relu", rows="subset", **f, **({"x3_segs": 1} if red else {}))
            _add(f"{p}_rows_empty", kern, 200, 320, 1, 36, rows="empty", **f, **({"x1_segs": 1} if red else {}))
            _add(f"{p}_outputs", kern, 200, 160, 2, 36, bf16_segs=1, fp8_segs=2, **f, **red)
            if fmt == BF16X6:
                _add(f"{p}_dmask_cols", kern, 200, 400, 1, 36, dmask=260, epi="add_e0", **f)


def _f16f8c():
    for kern, shape, wide in (("F16F8C_3", (240, 1), (160, 3)), ("F16F8C_1", (80, 1), (400, 1))):
        p, f = kern.lower(), {"fmt": F16F8C}
        for M in (1, 128, 200):
            _add(f"{p}_m{M}", kern, M, *shape, 132, **f)
        for K in (4, 128, 400):
            _add(f"{p}_k{K}", kern, 200, *shape, K, **f)
        _add(f"{p}_wide", kern, 200, *wide, 132, **f)
        _add(f"{p}_segments", kern, 200, 80, 3 if kern == "F16F8C_3" else 2, 132, **f)
        _add(f"{p}_nobias", kern, 200, *shape, 132, bias=False, **f)
        _epis(p, kern, 200, *shape, 132, ("relu", "accum", "add_e0"), **f)
        _add(f"{p}_radd", kern, 200, 80, 3 if kern == "F16F8C_3" else 2, 132, radd=7, **f)
        for rows in ("subset", "perm", "empty", "all"):
            _add(f"{p}_rows_{rows}", kern, 200, *shape, 132, rows=rows, epi="relu", **f)
        _add(f"{p}_gather", kern, 200, *shape, 132, rows="perm", gather=True, epi="add_e0", **f)
        _add(f"{p}_big", kern, 200, *shape, 132, big=True, **f)
    for tiles, M in ((7, 800), (9, 1100)):
        _add(f"f16f8c_1_tiles{tiles}", "F16F8C_1", M, 80, 1, 4, fmt=F16F8C)


_fp32_mfma()
_skinny()
_skinny_split()
_strip()
_f16f8c()

# launches the plan refuses: name -> (fields, the status the plan gives)
REFUSED = {
    "row_list_on_the_skinny_kernel": (dict(kernel="SKINNY_1", M=17, nseg=80, nsegs=1, K=48, rows="all"), 1),
    "gate_on_the_strip_formats": (dict(kernel="NONE", M=200, nseg=240, nsegs=1, K=36, fmt=F16F8C, epi="gate"), 1),
    "image_of_another_format": (dict(kernel="STRIP_3_F16_64", M=100, nseg=240, nsegs=1, K=36, fmt=F16X3, m_dispatch=BIG, image_fmt=BF16X6), 1),
}


# ---- operands, layout, arguments ---------------------------------------------------------------------------------------------------
def seg_mask(case, key, s):
    return (case.get(key, 0) >> s) & 1


def strip_kernel(case):
    return case["kernel"].startswith("STRIP") or case["kernel"].startswith("F16F8C")


def layout(case):
    """Row strides of a case, the same on the CPU (plan) and on the GPU: every operand is a column block of a wider matrix."""
    K, nseg = case["K"], case["nseg"]
    k0 = case.get("k0", K)
    dcols = case["dmask"] if case.get("dmask") else nseg
    return dict(lda0=k0 + 8, lda1=K - k0 + 12, ldy=nseg + 8, lde0=nseg + 12, lde1=nseg + 4, lde2=nseg + 8, lddm=dcols + 4,
                ldy8=16 + nseg + 4 * (nseg // 80) + 12)


def radd_seg(case):
    return min(1, case["nsegs"] - 1)


def draw(name, case):
    """The operands of a case as numpy arrays (fp32 unless stated), by the case's name."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    M, K, nseg, nsegs = case["M"], case["K"], case["nseg"], case["nsegs"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    rows = case.get("rows")
    gather = bool(case.get("gather"))
    Msrc = M + 5 if gather else M
    o = {"x": f32(rng.standard_normal((Msrc, K)))}
    if case.get("big"):
        o["x"][min(3, Msrc - 1), K // 2] = 5000.0
    o["w"] = [f32(rng.standard_normal((nseg, K)) / np.sqrt(K)) for _ in range(nsegs)]
    o["bias"] = [f32(rng.standard_normal(nseg)) for _ in range(nsegs)] if case.get("bias", True) else None
    if case.get("radd"):
        o["radd"] = f32(rng.standard_normal((-(-M // case["radd"]), nseg)))
    epi = case.get("epi")
    if epi in ("relu", "add_e0"):
        o["e0"] = f32(rng.standard_normal((M, nseg)))
    if epi in ("gate", "gate_e2"):
        for k in ("e0", "e1"):      # |e| >= 1/2: see the module docstring
            v = rng.standard_normal((M, nseg))
            o[k] = f32(np.sign(v) * (0.5 + np.abs(v)))
    if epi == "gate_e2":
        o["e2"] = f32(rng.standard_normal((M, nseg)))
    if epi == "accum":
        o["y_before"] = [f32(rng.standard_normal((M, nseg))) for _ in range(nsegs)]
    if case.get("dmask") is not None:
        dcols = case["dmask"] if case["dmask"] else nseg
        o["dmask"] = (rng.random((M, dcols)) < 0.8).astype(np.uint8)
    if rows:
        if gather:
            n = max(1, M - 3)
            o["rowidx"] = rng.integers(0, Msrc, size=M).astype(np.int32)
        else:
            perm = rng.permutation(M).astype(np.int32)
            n = {"subset": max(1, (3 * M) // 5), "perm": M, "empty": 0, "all": M}[rows]
            o["rowidx"] = perm if rows in ("perm", "empty") else np.sort(perm[:n]).astype(np.int32)
            if rows in ("subset", "all"):      # the list is as long as the launch has rows; entries past the live count are never read
                o["rowidx"] = np.concatenate([o["rowidx"], np.full(M - n, M - 1, dtype=np.int32)])
        o["nrows"] = n
    return o


def written_rows(case, o):
    """Boolean [M]: the output rows the launch writes."""
    M = case["M"]
    w = np.zeros(M, dtype=bool)
    if not case.get("rows"):
        w[:] = True
    elif case.get("gather"):
        w[:o["nrows"]] = True
    else:
        w[o["rowidx"][:o["nrows"]]] = True
    return w


def fill_args(case, ptr):
    """GemmArgs of a case; ptr: operand name -> address ("w0", "bias1", "y2", "a0", "a1", "e0" ...)."""
    g = GemmArgs()
    ld = layout(case)
    K, nsegs = case["K"], case["nsegs"]
    k0 = case.get("k0", K)
    g.a0, g.lda0, g.k0 = ptr["a0"], ld["lda0"], k0
    if k0 < K:
        g.a1, g.lda1 = ptr["a1"], ld["lda1"]
    for s in range(nsegs):
        g.w[s], g.y[s] = ptr[f"w{s}"], ptr[f"y{s}"]
        if case.get("bias", True):
            g.bias[s] = ptr[f"bias{s}"]
    g.ldy, g.nseg, g.nsegs, g.M, g.K = ld["ldy"], case["nseg"], nsegs, case["M"], K
    g.transW, g.epi = case.get("transW", 0), EPI[case.get("epi")]
    for k in ("e0", "e1", "e2"):
        if k in ptr:
            setattr(g, k, ptr[k])
            setattr(g, "ld" + k, ld["ld" + k])
    if case.get("radd"):
        g.radd, g.radd_seg, g.rows_per_b = ptr["radd"], radd_seg(case), case["radd"]
    if case.get("rows"):
        g.rowidx, g.nrows_dev, g.gather_only = ptr["rowidx"], ptr["nrows"], int(bool(case.get("gather")))
    g.m_dispatch = case.get("m_dispatch", 0)
    for k in ("x3_segs", "x1_segs", "bf16_segs", "fp8_segs", "ragged"):
        setattr(g, k, case.get(k, 0))
    g.ldy8 = ld["ldy8"]
    g.format = case.get("fmt") or 0
    if "wsplit" in ptr:
        g.wsplit = ptr["wsplit"]
    if "range_flag" in ptr:
        g.range_flag = ptr["range_flag"]
    if case.get("dmask") is not None:
        g.dmask, g.lddm, g.dscale, g.dmask_cols = ptr["dmask"], ld["lddm"], DSCALE, case["dmask"]
    return g


def fake_pointers(case):
    """16-byte aligned stand-ins for the device addresses: what the plan looks at on the CPU."""
    names = ["a0", "a1", "radd", "rowidx", "nrows", "dmask", "range_flag"] + [f"{k}{s}" for k in ("w", "bias", "y") for s in range(3)]
    ptr = {n: 0x10000 * (i + 1) for i, n in enumerate(names)}
    epi = case.get("epi")
    for k, on in (("e0", epi in ("relu", "add_e0", "gate", "gate_e2")), ("e1", epi in ("gate", "gate_e2")), ("e2", epi == "gate_e2")):
        if on:
            ptr[k] = 0x900000 + 0x10000 * int(k[1])
    if case.get("fmt") is not None:
        ptr["wsplit"] = 0xA00000
    return ptr


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def activations(case, o, dtype=np.float64):
    """[M, K]: row r of A as output row r meets it (through the row list when the launch gathers)."""
    x = o["x"].astype(dtype)
    if case.get("gather"):
        return x[o["rowidx"][:case["M"]].astype(np.int64)]
    return x


def reference(case, o, dtype=np.float64, product=None):
    """Per segment (pre, want): the value in front of the epilogue and the stored value, for all M rows, in `dtype`, in the kernels'
    order: A w^T (A w with transW: the same numbers, the weight is only stored the other way), + bias, + radd[row // rows_per_b];
    relu + e0 | gate of e0 and e1, + e2 | + y_before | + e0; the mask x dscale on columns < dmask_cols.  A bf16 or e4m3 segment is
    stored in front of the epilogue (the strip kernel's `continue`).  product(s, A, w): another product than A w^T in `dtype`
    (the emulations of the reduced sets), from the fp32 operands."""
    M = case["M"]
    A = activations(case, o, dtype)
    epi = case.get("epi")
    out = []
    for s in range(case["nsegs"]):
        v = product(s, activations(case, o, np.float32), o["w"][s]).astype(dtype) if product else A @ o["w"][s].astype(dtype).T
        if o["bias"] is not None:
            v = v + o["bias"][s].astype(dtype)
        if case.get("radd") and s == radd_seg(case):
            v = o["radd"].astype(dtype)[np.arange(M) // case["radd"]] + v
        pre = v
        if seg_mask(case, "bf16_segs", s) or seg_mask(case, "fp8_segs", s):
            out.append((pre, pre))
            continue
        if epi == "relu":
            v = np.maximum(v, 0) + o["e0"].astype(dtype)
        elif epi in ("gate", "gate_e2"):
            gate = 1 / (1 + np.exp(-v))
            v = gate * o["e0"].astype(dtype) + (1 - gate) * o["e1"].astype(dtype)
            if epi == "gate_e2":
                v = o["e2"].astype(dtype) + v
        elif epi == "accum":
            v = o["y_before"][s].astype(dtype) + v
        elif epi == "add_e0":
            v = o["e0"].astype(dtype) + v
        if case.get("dmask") is not None:
            dc = o["dmask"].shape[1]
            v = v.copy()
            v[:, :dc] = np.where(o["dmask"] != 0, v[:, :dc] * dtype(DSCALE), dtype(0))
        out.append((pre, v))
    return out


# ---- the reduced product sets, in float64 ------------------------------------------------------------------------------------------
def split_bf16(v):
    """fp32 -> its three bf16 pieces by truncation (split3f), as float64."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    top = lambda a: (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    a = top(v)
    r1 = v - a
    b = top(r1)
    c = r1 - b
    assert np.array_equal(a.astype(np.float64) + b.astype(np.float64) + c.astype(np.float64), v.astype(np.float64))
    return a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)


def fp16_rtz(v):
    """fp32 -> the fp16 value nearest zero (v_cvt_pkrtz_f16_f32), |v| < 65504 (tests/test_hip_fp8c.py:_fp16_rtz)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    bits = v.view(np.uint32)
    normal = (bits & np.uint32(0x7FFFFFFF)) >= np.uint32(0x38800000)
    trunc = (bits & np.uint32(0xFFFFE000)).view(np.float32)
    sub = (np.trunc(v.astype(np.float64) * 2.0 ** 24) * 2.0 ** -24).astype(np.float32)
    return np.where(normal, trunc, sub)


def split_f16(x, w):
    """fp16x3's pieces as float64: activations x 2^4 (hi truncated, lo = the remainder rounded to nearest), weights x 2^10 (both
    pieces rounded to nearest).  Products of the pieces carry 2^14."""
    xs = np.asarray(x, dtype=np.float32) * np.float32(16)
    xh = fp16_rtz(xs)
    xl = (xs - xh).astype(np.float16).astype(np.float32)
    ws = np.asarray(w, dtype=np.float32) * np.float32(1024)
    wh = ws.astype(np.float16).astype(np.float32)
    wl = (ws - wh).astype(np.float16).astype(np.float32)
    return tuple(a.astype(np.float64) for a in (xh, xl, wh, wl))


def emulated_product(fmt, products, x, w):
    """x w^T as the strip kernel forms it in `fmt` with `products` in ("full", "x3", "x1"): sums in float64."""
    if fmt == BF16X6:
        x1, x2, x3 = split_bf16(x)
        w1, w2, w3 = split_bf16(w)
        y = x1 @ w1.T
        if products != "x1":
            y = y + x2 @ w1.T + x1 @ w2.T
        if products == "full":
            y = y + x3 @ w1.T + x2 @ w2.T + x1 @ w3.T
        return y
    xh, xl, wh, wl = split_f16(x, w)
    y = xh @ wh.T
    if products != "x1":      # fp16x3: three products with x3_segs set or clear
        y = y + xl @ wh.T + xh @ wl.T
    return y / 16384.0


def mx_e4m3(v):
    """[..., K] (K % 32 == 0) -> OCP e4m3 with one E8M0 scale per 32 values, dequantised (tests/test_hip_fp8c.py:_mx_e4m3)."""
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    shp = v.shape
    vb = v.reshape(*shp[:-1], shp[-1] // 32, 32)
    amax = vb.abs().amax(-1, keepdim=True)
    u = amax.view(torch.int32)
    x = ((u >> 23) - 8 + ((u & 0x7FFFFF) > 0x600000).to(torch.int32)).clamp(0, 253)
    inv = ((254 - x) << 23).view(torch.float32)
    scale = torch.pow(2.0, (x - 127).to(torch.float64))
    q = (vb * inv).to(torch.float8_e4m3fn).to(torch.float64) * scale
    return q.reshape(shp).numpy()


def emulate_f16f8c(x, w):
    """x w^T as DIGAT_GEMM_F16F8C computes it, sums in float64 (tests/test_hip_fp8c.py:emulate_f16f8c without the bias)."""
    M, K = x.shape
    Kp = -(-K // 128) * 128
    xp = np.zeros((M, Kp), dtype=np.float32)
    wp = np.zeros((w.shape[0], Kp), dtype=np.float32)
    xp[:, :K], wp[:, :K] = x, w
    xs = xp * np.float32(16)
    xh = fp16_rtz(xs)
    xl = xs - xh
    ws = wp * np.float32(1024)
    wh = ws.astype(np.float16).astype(np.float32)
    wl = ws - wh
    return (xh.astype(np.float64) @ wh.astype(np.float64).T + mx_e4m3(xh) @ mx_e4m3(wl).T + mx_e4m3(xl) @ mx_e4m3(wh).T) / 16384.0


# ---- decoders ---------------------------------------------------------------------------------------------------------------------
def decode_bf16(u16):
    return (np.asarray(u16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


_E4M3 = np.array([(-1.0 if c & 0x80 else 1.0) * (float("nan") if c & 0x7F == 0x7F else
                                                  ((c & 7) * 2.0 ** -9 if (c >> 3) & 15 == 0 else (1 + (c & 7) / 8) * 2.0 ** (((c >> 3) & 15) - 7)))
                  for c in range(256)])


def decode_e4m3_rows(rows, nseg):
    """uint8 [M, >= nseg + 4 nseg / 80] block-scaled rows -> (decoded float64 [M, nseg], scales float64 [M, nseg / 80])."""
    rows = np.ascontiguousarray(rows)
    strips = nseg // 80
    scales = np.ascontiguousarray(rows[:, nseg:nseg + 4 * strips]).view(np.float32).astype(np.float64)
    return _E4M3[rows[:, :nseg]] * np.repeat(scales, 80, axis=1), scales


def encode_bf16(v):
    """fp32 -> bf16 bits, round to nearest even (pack_bf16_rne)."""
    a = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((a + 0x7FFF + ((a >> 16) & 1)) >> 16).astype(np.uint16)


def encode_e4m3_rows(v, nseg):
    """fp32 [M, nseg] -> the block-scaled rows the strip kernel's epilogue writes (scale = the strip's absmax / 448)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    M, strips = v.shape[0], nseg // 80
    amax = np.abs(v).reshape(M, strips, 80).max(-1)
    scale = np.where(amax > 0, amax * np.float32(1.0 / 448.0), np.float32(1)).astype(np.float32)
    q = v * np.repeat(np.float32(1) / scale, 80, axis=1)
    codes = torch.from_numpy(np.clip(q, -448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return np.concatenate([codes, scale.view(np.uint8).reshape(M, 4 * strips)], axis=1)


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
REDUCED = {(BF16X6, "x3"): 3 * 2.0 ** -14, (BF16X6, "x1"): 2 * 2.0 ** -7, (F16X3, "x3"): 0.0, (F16X3, "x1"): 3 * 2.0 ** -11}


def products_of(case, s):
    if strip_kernel(case) and not case["kernel"].startswith("F16F8C"):
        return "x1" if seg_mask(case, "x1_segs", s) else ("x3" if seg_mask(case, "x3_segs", s) else "full")
    return "full"


def full_tolerance(case, pre):
    return 2e-6 * math.sqrt(case["K"]) + 1e-5 * np.abs(pre)


def tolerances(case, o, ref, products=None):
    """Per segment the float64 bound [M, nseg] on the value in front of the output format's rounding (module docstring); products:
    the product set to bound each segment for (default: the one the case asks for)."""
    A = np.abs(activations(case, o))
    f8c = case["kernel"].startswith("F16F8C")
    rowmax = np.max(np.abs(np.concatenate([pre for pre, _ in ref], axis=1)), axis=1, keepdims=True)
    tol = []
    for s, (pre, want) in enumerate(ref):
        l1 = None
        if f8c:
            l1 = A @ np.abs(o["w"][s].astype(np.float64)).T
            tol.append(2.0 ** -12 * l1 + 1e-6 * rowmax)
            continue
        t = full_tolerance(case, pre)
        if case.get("epi") in ("gate", "gate_e2") and not (seg_mask(case, "bf16_segs", s) or seg_mask(case, "fp8_segs", s)):
            t = t * np.maximum(np.abs(o["e0"].astype(np.float64)), np.abs(o["e1"].astype(np.float64)))
        ps = products or products_of(case, s)
        if ps != "full" and REDUCED[(case["fmt"], ps)]:
            t = t + REDUCED[(case["fmt"], ps)] * (A @ np.abs(o["w"][s].astype(np.float64)).T)
        tol.append(t)
    return tol


def output_kind(case, s):
    return "e4m3" if seg_mask(case, "fp8_segs", s) else ("bf16" if seg_mask(case, "bf16_segs", s) else "fp32")


def check_segment(case, s, got, want, tol, rows, what, stats=None):
    """Hold segment s of a launch — `got`: fp32 [M, nseg], bf16 bits [M, nseg] or e4m3 rows [M, bytes] — to `want` within `tol` on the
    rows `rows` (boolean [M]); returns the worst err / bound (stats["scale"]: the same of an e4m3 segment's block scales)."""
    nseg = case["nseg"]
    want, tol = want[rows], tol[rows]
    if want.size == 0:
        return 0.0
    if seg_mask(case, "fp8_segs", s):
        dec, scales = decode_e4m3_rows(got[rows], nseg)
        R = want.shape[0]
        amax = np.abs(want).reshape(R, nseg // 80, 80).max(-1)
        tmax = tol.reshape(R, nseg // 80, 80).max(-1)
        assert np.isfinite(scales).all() and (scales > 0).all(), f"{what}: scales"
        r_scale = float((np.abs(scales * 448.0 - amax) / tmax).max())
        assert r_scale <= 1.0, f"{what}: a block scale is not its absmax / 448 (worst err/tol {r_scale:.3f})"
        if stats is not None:
            stats["scale"] = max(stats.get("scale", 0.0), r_scale)
        sc = np.repeat(scales, 80, axis=1)
        half_ulp = np.where(np.abs(want) >= 2.0 ** -6 * sc, 2.0 ** -4 * np.abs(want), 2.0 ** -10 * sc)
        got, tol = dec, half_ulp + tol
    elif seg_mask(case, "bf16_segs", s):
        got, tol = decode_bf16(got[rows]), 2.0 ** -8 * np.abs(want) + tol
    else:
        got = got[rows].astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    err = np.abs(got - want)
    ratio = float((err / tol).max())
    if ratio > 1.0:
        idx = np.unravel_index(np.argmax(err / tol), err.shape)
        raise AssertionError(f"{what}: {int((err > tol).sum())}/{err.size} out of bound, worst err/tol {ratio:.3f} at (listed row, column) {idx}: "
                             f"got {got[idx]:.9g} want {want[idx]:.9g} (bound {tol[idx]:.3e})")
    return ratio
