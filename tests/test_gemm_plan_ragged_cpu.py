"""CPU suite: the launch plan of ragged 240-column tiles (GemmArgs::ragged, digat_amd/csrc/digat_gemm_plan.h).

A launch asks for them; gemm_plan grants them only to the strip-mined kernel at 128-row tiles when N is more than three strips
and no multiple of three.  The rows below pin (a) that a launch which does not ask keeps the plan it had before the field
existed — recorded from that dispatch — and (b) what asking yields: the kernel, ceil(strips / 3) column tiles, and a grid of
8 x (ceil(full-width tiles / 8) + ceil(short tiles / 8)) workgroups, an XCD's full-width tiles in front of its short ones.
"""
import shutil
import subprocess

from conftest import REPO

A = "(const float*)0x10000"
P = "(const float*)0x20000"
R = "(const int*)0x30000"
F16 = {"wsplit": "IMG", "format": "1"}
BF16 = {"wsplit": "IMG", "format": "0"}
ROWS = {"rowidx": R, "nrows_dev": R}
RELU = {"epi": "EPI_RELU_RES", "e0": P, "lde0": "400"}
ASK = {"ragged": "DIGAT_GEMM_RAGGED"}
BIG = 1 << 30
USER = 4096 * 34         # the user nodes of a 4 096-row pass

# name: (M, nseg, nsegs, K, fields), expected "kernel ragged grid mt nt"
CASES = {
    # the field clear: the plans of before
    "fa_clear": ((40960, 400, 1, 400, {**F16, **ROWS, **RELU}), "gemm_bf16x6s_kernel<1, true, 2, false> ragged=0 grid=1600 mt=320 nt=5"),
    "bd_clear": ((4096, 400, 1, 400, F16), "gemm_bf16x6s_kernel<1, true, 1, false> ragged=0 grid=320 mt=64 nt=5"),
    "proj_clear": ((USER, 400, 3, 400, {**F16, **ROWS}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=0 grid=5440 mt=1088 nt=5"),
    "two_segments_clear": ((USER, 400, 2, 400, {**F16, **ROWS}), "gemm_bf16x6s_kernel<1, true, 2, false> ragged=0 grid=10880 mt=1088 nt=10"),
    "bf16_clear": ((40960, 400, 1, 400, {**BF16, **ROWS}), "gemm_bf16x6s_kernel<1, false, 2, false> ragged=0 grid=1600 mt=320 nt=5"),
    "small_clear": ((384, 400, 1, 400, {**F16, "m_dispatch": str(BIG)}), "gemm_bf16x6s_kernel<1, true, 1, false> ragged=0 grid=32 mt=6 nt=5"),
    # the field set, granted: 3 + 2 strips, 3 + 3 + 3 + 1 strips
    "fa_ask": ((40960, 400, 1, 400, {**F16, **ROWS, **RELU, **ASK}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=1 grid=640 mt=320 nt=2"),
    "fa_ask_rowmajor": ((40960, 400, 1, 400, {**F16, **ROWS, **RELU, "ragged": "DIGAT_GEMM_RAGGED_ROWMAJOR"}),
                        "gemm_bf16x6s_kernel<3, true, 2, true> ragged=2 grid=640 mt=320 nt=2"),
    "two_segments_ask": ((USER, 400, 2, 400, {**F16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=1 grid=4352 mt=1088 nt=4"),
    "user_nodes_ask": ((USER, 400, 1, 400, {**F16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=1 grid=2176 mt=1088 nt=2"),
    "bf16_ask": ((40960, 400, 1, 400, {**BF16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<3, false, 2, false> ragged=1 grid=640 mt=320 nt=2"),
    "x3_ask": ((40960, 400, 2, 400, {**F16, **ASK, "x3_segs": "2"}), "gemm_bf16x6s_kernel<3, true, 2, false> ragged=1 grid=1280 mt=320 nt=4"),
    "odd_ask": ((4100, 560, 1, 48, {**BF16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<3, false, 2, false> ragged=1 grid=112 mt=33 nt=3"),
    # ... at m_dispatch, like the choice of the kernel itself: a small launch gets the tiles of the large one
    "small_ask": ((384, 400, 1, 400, {**F16, **ASK, "m_dispatch": str(BIG)}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=1 grid=16 mt=3 nt=2"),
    "small_ask2": ((384, 400, 2, 48, {**F16, **ROWS, **ASK, "m_dispatch": str(BIG)}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=1 grid=24 mt=3 nt=4"),
    # the field set, ignored: N a multiple of 240, N of at most three strips, 64-row tiles, the other kernels
    "proj_ask": ((USER, 400, 3, 400, {**F16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<3, true, 2, true> ragged=0 grid=5440 mt=1088 nt=5"),
    "two_strips_ask": ((40960, 160, 1, 400, {**F16, **ROWS, **ASK}), "gemm_bf16x6s_kernel<1, true, 2, false> ragged=0 grid=640 mt=320 nt=2"),
    "small_two_strips_ask": ((384, 160, 1, 400, {**F16, **ASK, "m_dispatch": str(BIG)}), "gemm_bf16x6s_kernel<1, true, 2, false> ragged=0 grid=8 mt=3 nt=2"),
    "bd_ask": ((4096, 400, 1, 400, {**F16, **ASK}), "gemm_bf16x6s_kernel<1, true, 1, false> ragged=0 grid=320 mt=64 nt=5"),
    "skinny_ask": ((1024, 400, 1, 400, {**F16, **ASK}), "gemm_skinny_split_kernel<1, true> ragged=0 grid=320 mt=64 nt=5"),
    "f8c_ask": ((40960, 400, 1, 400, {"wsplit": "IMG", "format": "2", **ASK}), "gemm_f16f8c_kernel<1> ragged=0 grid=1600 mt=320 nt=5"),
    "f32_ask": ((40960, 400, 1, 400, ASK), "gemm_f32_kernel<128, 80, 4, 1, 1, 0> ragged=0 grid=1600 mt=320 nt=5"),
}

HARNESS = r"""
#include <stdio.h>
#include <string.h>
#include "digat_amd/csrc/digat_gemm_plan.h"
static const unsigned short* const IMG = (const unsigned short*)0x1000;
static void run(const char* name, const GemmArgs& g) {
    const GemmPlan p = gemm_plan(g, DIGAT_KERNEL_LINEAR);
    if (p.status) printf("%s|error %d\n", name, p.status);
    else printf("%s|%s ragged=%d grid=%u mt=%d nt=%d\n", name, gemm_kernel_name(p.kernel), p.ragged, p.grid, p.mtiles, p.ntiles);
}
int main() {
"""


def _case_source(name, M, N, nsegs, K, fields):
    s = ["{ GemmArgs g; memset(&g, 0, sizeof(g));",
         f"g.a0 = {A}; g.lda0 = {K}; g.k0 = {K}; g.K = {K}; g.M = {M}; g.nseg = {N}; g.nsegs = {nsegs}; g.ldy = {N};"]
    s += [f"g.w[{i}] = {P}; g.y[{i}] = (float*){P};" for i in range(nsegs)]
    s += [f"g.{k} = {v};" for k, v in fields.items()]
    s.append(f'run("{name}", g); }}')
    return " ".join(s)


def test_ragged_tiles_are_granted_only_where_asked_and_possible(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS + "\n".join(_case_source(n, *args) for n, (args, _) in CASES.items()) + "\nreturn 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}", str(src), "-o", str(exe)], check=True)
    got = dict(l.split("|") for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert got.keys() == CASES.keys()
    for name, (_, want) in CASES.items():
        assert got[name] == want, (name, got[name])


def test_the_grid_of_a_ragged_launch_holds_every_tile():
    """The kernel's long-first map, replayed on the host: with any live row count up to M, the workgroups of the plan's grid reach
    every (row tile, column tile) exactly once, an XCD's full-width tiles before its short ones."""
    def tiles(grid, mlive, ntiles):
        nfw = ntiles - 1
        nfull, cf, cs = mlive * nfw, (mlive * nfw + 7) // 8, (mlive + 7) // 8
        seen, per_xcd = [], {}
        for wg in range(grid):
            xcd, j = wg & 7, wg >> 3
            if j < cf:
                t = xcd * cf + j
                if t >= nfull:
                    continue
                tile = (t // nfw, t % nfw)
            else:
                t = xcd * cs + (j - cf)
                if j - cf >= cs or t >= mlive:
                    continue
                tile = (t, nfw)
            seen.append(tile)
            per_xcd.setdefault(xcd, []).append(tile[1] == nfw)
        return seen, per_xcd

    for mtiles, ntiles in ((3, 2), (3, 4), (320, 2), (33, 3), (1, 2), (9, 4)):
        grid = 8 * ((mtiles * (ntiles - 1) + 7) // 8 + (mtiles + 7) // 8)         # gemm_plan's
        for mlive in {0, 1, 2, mtiles // 2, mtiles - 1, mtiles}:
            if mlive > mtiles:
                continue
            seen, per_xcd = tiles(grid, mlive, ntiles)
            assert sorted(seen) == [(m, n) for m in range(mlive) for n in range(ntiles)], (mtiles, ntiles, mlive)
            for short in per_xcd.values():
                assert short == sorted(short)          # False (full width) before True (short)
