"""CPU suite: which GEMM kernel instantiation runs a launch, on which grid, and what a launch returns.

digat_amd/csrc/digat_gemm_plan.h holds the whole dispatch of launch_gemm (gemm_plan) in plain C++; this test builds it with the
host compiler and pins its answer for a table of GemmArgs that reaches every branch, every instantiation and every refusal.
The expected rows were recorded from the previous dispatch (the chain of branches in launch_gemm / launch_gemm_f16f8c, run with
hipLaunchKernelGGL recording kernel, grid, block and tile counts): a shape that moves to another kernel fails here even when
the other kernel's results would match within tolerance.
"""
import os
import re
import shutil
import subprocess

from conftest import REPO

A = "(const float*)0x10000"
P = "(const float*)0x20000"
R = "(const int*)0x30000"
BIG = 68608
PROJ = "DIGAT_KERNEL_PROJ"
F32_128 = "gemm_f32_kernel<128, 80, 4, 1, 1, 0>"
F32_128P = "gemm_f32_kernel<128, 80, 4, 1, 1, 1>"
F32_64 = "gemm_f32_kernel<64, 80, 4, 1, 2, 0>"
F32_32 = "gemm_f32_kernel<32, 64, 1, 4, 2, 0>"
# images: IMG<f> was split in format f, IMGU by nobody the library knows (no format to check against)
F8C = {"wsplit": "IMG2", "format": "2"}
F16 = {"wsplit": "IMG1", "format": "1"}
BF16 = {"wsplit": "IMG0", "format": "0"}
ROWS = {"rowidx": R, "nrows_dev": R}
GATE = {"epi": "EPI_GATE", "k0": "400", "a1": P, "lda1": "400", "e0": P, "e1": P, "lde0": "400", "lde1": "400"}
KTAIL = {"k0": "400", "a1": P, "lda1": "4"}
RADD = {"radd": P, "radd_seg": "1", "rows_per_b": "64"}
GB4 = 1 << 20          # rows of 1024 floats: a row-list operand of 4 GB

# name: (M, nseg, nsegs, K, kind, fields), (takes a row list, expected launch)
CASES = {
    # 1. fp16-fp8c: its own kernel at every row count; without an image the launch runs as fp16x3's
    "f8c_3": ((4096, 400, 3, 400, PROJ, F8C), (1, "gemm_f16f8c_kernel<3> grid=160 block=512 mt=32 nt=5")),
    "f8c_1": ((100, 80, 1, 400, PROJ, F8C), (1, "gemm_f16f8c_kernel<1> grid=8 block=512 mt=1 nt=1")),
    "f8c_rows": ((4096, 400, 3, 400, PROJ, {**F8C, **ROWS}), (1, "gemm_f16f8c_kernel<3> grid=160 block=512 mt=32 nt=5")),
    "f8c_unnoted": ((4096, 400, 3, 400, PROJ, {**F8C, "wsplit": "IMGU"}), (1, "gemm_f16f8c_kernel<3> grid=160 block=512 mt=32 nt=5")),
    "f8c_wrong_image": ((4096, 400, 3, 400, PROJ, {**F8C, "wsplit": "IMG1"}), (1, "error 1")),
    "f8c_gate": ((4096, 400, 1, 400, None, {**F8C, "epi": "EPI_GATE"}), (0, "error 1")),
    "f8c_bf16_segs": ((4096, 400, 3, 400, PROJ, {**F8C, "bf16_segs": "6"}), (0, "error 1")),
    "f8c_x3_segs": ((4096, 400, 3, 400, PROJ, {**F8C, "x3_segs": "6"}), (0, "error 1")),
    "f8c_unaligned_a0": ((4096, 400, 3, 400, PROJ, {**F8C, "a0": "(const float*)0x10004"}), (0, "error 1")),
    "f8c_no_image": ((4096, 400, 3, 400, PROJ, {"format": "2"}), (0, f"{F32_128P} grid=480 block=256 mt=32 nt=15")),
    "f8c_no_image_small": ((100, 400, 3, 400, None, {"format": "2"}), (0, "gemm_skinny_kernel<1, false, false> grid=105 block=256 mt=7 nt=15")),
    "f8c_no_image_rows": ((4096, 400, 3, 400, PROJ, {"format": "2", "rowidx": R}), (0, "error 1")),
    # 2. skinny, weights read as their transpose
    "tw_k800": ((1000, 400, 1, 800, None, {"transW": "1"}), (0, "gemm_skinny_kernel<2, false, true> grid=160 block=256 mt=32 nt=5")),
    "tw_mt1": ((1000, 400, 1, 400, None, {"transW": "1"}), (0, "gemm_skinny_kernel<1, false, true> grid=315 block=256 mt=63 nt=5")),
    "tw_wide": ((2000, 2000, 1, 400, None, {"transW": "1"}), (0, "gemm_skinny_kernel<2, false, true> grid=1575 block=256 mt=63 nt=25")),
    "tw_rows": ((1000, 400, 1, 400, None, {"transW": "1", "rowidx": R}), (0, "error 1")),
    "tw_two_segs": ((1000, 400, 2, 400, None, {"transW": "1"}), (0, f"{F32_64} grid=160 block=256 mt=16 nt=10")),
    "tw_big": ((4096, 400, 1, 400, None, {"transW": "1"}), (0, f"{F32_128} grid=160 block=256 mt=32 nt=5")),
    # 3. skinny, split operands
    "ss_f16_mt2": ((1024, 400, 3, 400, None, F16), (0, "gemm_skinny_split_kernel<2, true> grid=480 block=256 mt=32 nt=15")),
    "ss_f16_mt1": ((100, 400, 1, 400, None, F16), (0, "gemm_skinny_split_kernel<1, true> grid=35 block=256 mt=7 nt=5")),
    "ss_bf16_mt2": ((1024, 400, 3, 400, None, BF16), (0, "gemm_skinny_split_kernel<2, false> grid=480 block=256 mt=32 nt=15")),
    "ss_bf16_mt1": ((100, 400, 1, 400, None, BF16), (0, "gemm_skinny_split_kernel<1, false> grid=35 block=256 mt=7 nt=5")),
    "ss_gate": ((1024, 400, 1, 800, None, {**F16, **GATE}), (0, "gemm_skinny_split_kernel<1, true> grid=320 block=256 mt=64 nt=5")),
    "ss_unnoted": ((1024, 400, 3, 400, None, {**BF16, "wsplit": "IMGU"}), (0, "gemm_skinny_split_kernel<2, false> grid=480 block=256 mt=32 nt=15")),
    "ss_bad_format": ((1024, 400, 3, 400, None, {"wsplit": "IMGU", "format": "5"}), (0, "error 1")),
    "ss_wrong_image": ((1024, 400, 3, 400, None, {**F16, "wsplit": "IMG0"}), (0, "error 1")),
    "ss_m_dispatch": ((4096, 400, 3, 400, None, {**F16, "m_dispatch": "1"}), (0, "gemm_skinny_split_kernel<2, true> grid=1920 block=256 mt=128 nt=15")),
    "ss_rows": ((1024, 400, 3, 400, None, {**F16, "rowidx": R}), (0, "error 1")),
    "ss_radd": ((1024, 400, 3, 400, PROJ, {**F16, **RADD}), (0, f"{F32_64} grid=240 block=256 mt=16 nt=15")),
    "ss_add_e0": ((1024, 400, 1, 400, None, {**F16, "epi": "EPI_ADD_E0", "e0": P, "lde0": "400"}),
                  (0, "gemm_skinny_kernel<1, false, false> grid=320 block=256 mt=64 nt=5")),
    # 4. skinny fp32
    "sk_mt2_ktail": ((1024, 400, 3, 404, None, KTAIL), (0, "gemm_skinny_kernel<2, true, false> grid=480 block=256 mt=32 nt=15")),
    "sk_mt2": ((1024, 400, 3, 400, None, {}), (0, "gemm_skinny_kernel<2, false, false> grid=480 block=256 mt=32 nt=15")),
    "sk_mt1_ktail": ((100, 80, 1, 404, None, KTAIL), (0, "gemm_skinny_kernel<1, true, false> grid=7 block=256 mt=7 nt=1")),
    "sk_mt1": ((100, 80, 1, 400, None, {}), (0, "gemm_skinny_kernel<1, false, false> grid=7 block=256 mt=7 nt=1")),
    "sk_k800": ((100, 80, 1, 800, None, {}), (0, "gemm_skinny_kernel<2, false, false> grid=4 block=256 mt=4 nt=1")),
    "sk_rows": ((100, 80, 1, 400, None, {"rowidx": R}), (0, "error 1")),
    "sk_split_k_odd": ((1024, 400, 1, 404, None, {**BF16, **KTAIL}), (0, "gemm_skinny_kernel<1, true, false> grid=320 block=256 mt=64 nt=5")),
    # 5. one launch per segment (the expected launch is every segment's)
    "perseg_small": ((100, 100, 2, 64, None, {}), (0, f"per segment: {F32_32} grid=8 block=256 mt=4 nt=2")),
    "perseg_big_radd": ((4096, 100, 3, 64, PROJ, RADD), (0, f"per segment: {F32_128P} grid=64 block=256 mt=32 nt=2")),
    "perseg_rows": ((4096, 100, 3, 64, None, {"rowidx": R}), (0, "error 1")),
    "perseg_not_needed": ((100, 128, 2, 64, None, {}), (0, f"{F32_32} grid=16 block=256 mt=4 nt=4")),
    # 6. strip-mined: 64-row tiles below 400 workgroups, 240-column tiles, FULL
    "st_f16_64_3": ((4096, 400, 3, 400, PROJ, F16), (1, "gemm_bf16x6s_kernel<3, true, 1, false> grid=320 block=256 mt=64 nt=5")),
    "st_f16_64_1": ((4096, 400, 1, 400, None, F16), (1, "gemm_bf16x6s_kernel<1, true, 1, false> grid=320 block=256 mt=64 nt=5")),
    "st_bf16_64_3": ((4096, 400, 3, 400, None, BF16), (1, "gemm_bf16x6s_kernel<3, false, 1, false> grid=320 block=256 mt=64 nt=5")),
    "st_bf16_64_1": ((4096, 400, 1, 400, None, BF16), (1, "gemm_bf16x6s_kernel<1, false, 1, false> grid=320 block=256 mt=64 nt=5")),
    "st_bf16_rows_small": ((4096, 400, 3, 400, None, {**BF16, **ROWS}), (1, "gemm_bf16x6s_kernel<3, false, 2, false> grid=160 block=256 mt=32 nt=5")),
    "st_f16_rows_small": ((4096, 400, 3, 400, PROJ, {**F16, **ROWS}), (1, "gemm_bf16x6s_kernel<3, true, 1, false> grid=320 block=256 mt=64 nt=5")),
    "st_f16_full": ((BIG, 400, 3, 400, PROJ, F16), (1, "gemm_bf16x6s_kernel<3, true, 2, true> grid=2680 block=256 mt=536 nt=5")),
    "st_f16_x3": ((BIG, 400, 3, 400, PROJ, {**F16, "x3_segs": "6"}), (1, "gemm_bf16x6s_kernel<3, true, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_f16_x1": ((BIG, 400, 3, 400, PROJ, {**F16, "x1_segs": "6", "bf16_segs": "6"}),
                  (1, "gemm_bf16x6s_kernel<3, true, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_f16_fp8_segs": ((BIG, 400, 3, 400, PROJ, {**F16, "fp8_segs": "6", "ldy8": "512"}),
                        (1, "gemm_bf16x6s_kernel<3, true, 2, true> grid=2680 block=256 mt=536 nt=5")),
    "st_bf16_big": ((BIG, 400, 3, 400, None, BF16), (1, "gemm_bf16x6s_kernel<3, false, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_bf16_x1": ((BIG, 400, 3, 400, None, {**BF16, "x1_segs": "7"}), (1, "gemm_bf16x6s_kernel<3, false, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_f16_big_1": ((BIG, 400, 1, 400, None, F16), (1, "gemm_bf16x6s_kernel<1, true, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_bf16_big_1": ((BIG, 400, 1, 400, None, BF16), (1, "gemm_bf16x6s_kernel<1, false, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_f16_rows": ((BIG, 400, 3, 400, PROJ, {**F16, **ROWS}), (1, "gemm_bf16x6s_kernel<3, true, 2, true> grid=2680 block=256 mt=536 nt=5")),
    "st_bf16_gather": ((20000, 400, 3, 300, None, {**BF16, "rowidx": R, "gather_only": "1"}),
                       (1, "gemm_bf16x6s_kernel<3, false, 2, false> grid=792 block=256 mt=157 nt=5")),
    "st_bf16_dmask": ((BIG, 400, 1, 1200, None, {**BF16, "dmask": "(const uint8_t*)0x40000", "lddm": "400"}),
                      (1, "gemm_bf16x6s_kernel<1, false, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_unnoted": ((BIG, 400, 3, 400, None, {**BF16, "wsplit": "IMGU"}), (1, "gemm_bf16x6s_kernel<3, false, 2, false> grid=2680 block=256 mt=536 nt=5")),
    "st_m_dispatch": ((100, 400, 3, 400, PROJ, {**F16, "m_dispatch": "1 << 30"}), (1, "gemm_bf16x6s_kernel<3, true, 1, false> grid=16 block=256 mt=2 nt=5")),
    "st_rows_4g": ((GB4, 400, 3, 1024, None, {**F16, "rowidx": R}), (1, "error 2")),
    "st_rows_below_4g": ((GB4 - 1, 400, 3, 1024, None, {**F16, "rowidx": R}), (1, "gemm_bf16x6s_kernel<3, true, 2, true> grid=40960 block=256 mt=8192 nt=5")),
    "st_bad_format": ((BIG, 400, 3, 400, None, {"wsplit": "IMGU", "format": "5"}), (1, "error 1")),
    "st_bad_format_4g": ((GB4, 400, 3, 1024, None, {"wsplit": "IMGU", "format": "5", "rowidx": R}), (1, "error 1")),
    "st_wrong_image": ((BIG, 400, 3, 400, None, {**F16, "wsplit": "IMG0"}), (1, "error 1")),
    "st_wrong_image_4g": ((GB4, 400, 3, 1024, None, {**F16, "wsplit": "IMG0", "rowidx": R}), (1, "error 2")),
    "st_f8c_image_as_f16": ((BIG, 400, 3, 400, None, {**F16, "wsplit": "IMG2"}), (1, "error 1")),
    # 7. fp32 MFMA
    "f32_proj": ((4096, 400, 3, 400, PROJ, {}), (0, f"{F32_128P} grid=480 block=256 mt=32 nt=15")),
    "f32_linear": ((4096, 400, 3, 400, None, {}), (0, f"{F32_128} grid=480 block=256 mt=32 nt=15")),
    "f32_mid": ((1024, 400, 3, 400, None, RADD), (0, f"{F32_64} grid=240 block=256 mt=16 nt=15")),
    "f32_small": ((100, 100, 1, 64, None, {}), (0, f"{F32_32} grid=8 block=256 mt=4 nt=2")),
    "f32_gate_split": ((BIG, 400, 1, 800, None, {**F16, **GATE}), (0, f"{F32_128} grid=2680 block=256 mt=536 nt=5")),
    "f32_short_k": ((BIG, 400, 3, 16, None, F16), (0, f"{F32_128} grid=8040 block=256 mt=536 nt=15")),
    "f32_transW_big": ((4096, 400, 1, 400, PROJ, {"transW": "1"}), (0, f"{F32_128P} grid=160 block=256 mt=32 nt=5")),
    "f32_rows": ((4096, 400, 3, 400, None, {"rowidx": R}), (0, "error 1")),
    # the thresholds, from both sides
    "edge_wg395": ((10112, 400, 3, 400, PROJ, F16), (1, "gemm_bf16x6s_kernel<3, true, 1, false> grid=792 block=256 mt=158 nt=5")),
    "edge_wg400": ((10240, 400, 3, 400, PROJ, F16), (1, "gemm_bf16x6s_kernel<3, true, 2, true> grid=400 block=256 mt=80 nt=5")),
    "edge_m2047": ((2047, 400, 3, 400, PROJ, F16), (0, "gemm_skinny_split_kernel<2, true> grid=960 block=256 mt=64 nt=15")),
    "edge_m2048": ((2048, 400, 3, 400, PROJ, F16), (1, "gemm_bf16x6s_kernel<3, true, 1, false> grid=160 block=256 mt=32 nt=5")),
    "edge_ss315": ((672, 400, 3, 400, None, F16), (0, "gemm_skinny_split_kernel<1, true> grid=630 block=256 mt=42 nt=15")),
    "edge_ss330": ((673, 400, 3, 400, None, F16), (0, "gemm_skinny_split_kernel<2, true> grid=330 block=256 mt=22 nt=15")),
    "edge_sk465": ((992, 400, 3, 400, None, {}), (0, "gemm_skinny_kernel<1, false, false> grid=930 block=256 mt=62 nt=15")),
    "edge_sk480": ((993, 400, 3, 400, None, {}), (0, "gemm_skinny_kernel<2, false, false> grid=480 block=256 mt=32 nt=15")),
}

HARNESS = r"""
#include <stdio.h>
#include <string.h>
#include "digat_amd/csrc/digat_gemm_plan.h"
static const unsigned short* const IMG0 = (const unsigned short*)0x1000;
static const unsigned short* const IMG1 = (const unsigned short*)0x2000;
static const unsigned short* const IMG2 = (const unsigned short*)0x3000;
static const unsigned short* const IMGU = (const unsigned short*)0x4000;
// the format the library recorded for an image (wsplit_format_of): -1 = not one it has split
static int made_as(const void* img) { return img == IMG0 ? 0 : img == IMG1 ? 1 : img == IMG2 ? 2 : -1; }
static void launch(const GemmPlan& p, char* out) {
    sprintf(out, "%s grid=%u block=%u mt=%d nt=%d", gemm_kernel_name(p.kernel), p.grid, p.block, p.mtiles, p.ntiles);
}
static void run(const char* name, const GemmArgs& g, int kind) {
    const GemmPlan p = gemm_plan(g, kind);
    char out[256];
    const int m = made_as(g.wsplit);
    if (p.status) sprintf(out, "error %d", p.status);
    else if (p.image_format >= 0 && m >= 0 && m != p.image_format) sprintf(out, "error %d", DIGAT_ERR_ARG);
    else if (p.kernel == GEMM_PER_SEGMENT) {
        GemmArgs one = g;              // the segments of these launches are alike
        one.nsegs = 1; one.radd = nullptr;
        char seg[200];
        launch(gemm_plan(one, kind), seg);
        sprintf(out, "per segment: %s", seg);
    } else launch(p, out);
    printf("%s|%d|%s\n", name, (int)gemm_takes_row_list(g), out);
}
int main() {
#define PRINT_NAME(id, ...) printf("kernel|%s\n", #__VA_ARGS__);
    DIGAT_GEMM_KERNELS(PRINT_NAME)
"""


def _case_source(name, M, N, nsegs, K, kind, fields):
    s = [f"{{ GemmArgs g; memset(&g, 0, sizeof(g));",
         f"g.a0 = {A}; g.lda0 = {K}; g.k0 = {K}; g.K = {K}; g.M = {M}; g.nseg = {N}; g.nsegs = {nsegs}; g.ldy = {N};"]
    s += [f"g.w[{i}] = {P}; g.y[{i}] = (float*){P};" for i in range(nsegs)]
    s += [f"g.{k} = {v};" for k, v in fields.items()]
    s.append(f'run("{name}", g, {kind or "DIGAT_KERNEL_LINEAR"}); }}')
    return " ".join(s)


def test_gemm_plan_pins_every_launch(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS + "\n".join(_case_source(n, *args) for n, (args, _) in CASES.items()) + "\nreturn 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}", str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()

    kernels = [l.split("|", 1)[1] for l in lines if l.startswith("kernel|")]
    got = {}
    for l in lines:
        if not l.startswith("kernel|"):
            name, rows, launch = l.split("|")
            got[name] = (int(rows), launch)
    assert got.keys() == CASES.keys()
    for name, (_, want) in CASES.items():
        assert got[name] == want, name

    # the table reaches every instantiation the library launches, each under the name profiles list it by
    reached = {re.match(r"(?:per segment: )?(\S+(?: \S+)*?) grid=", launch).group(1)
               for _, launch in got.values() if "grid=" in launch}
    assert reached == set(kernels)
    assert len(kernels) == len(set(kernels)) == 25
    assert any(k.startswith("gemm_bf16x6s_kernel<3") for k in kernels)                    # bench.py's symbols
    assert "gemm_f32_kernel<128, 80, 4, 1, 1, 1>" in kernels
    assert any(k.startswith("gemm_skinny_split") for k in kernels) and any(k.startswith("gemm_f16f8c_kernel") for k in kernels)
    # every launch in the library goes through the plan: no kernel of the list is launched anywhere else
    csrc = os.path.join(REPO, "digat_amd", "csrc")
    for f in os.listdir(csrc):
        text = open(os.path.join(csrc, f)).read()
        for k in ("gemm_f16f8c_kernel<", "gemm_skinny_kernel<", "gemm_skinny_split_kernel<", "gemm_bf16x6s_kernel<", "gemm_f32_kernel<"):
            assert not re.search(r"hipLaunchKernelGGL\(\(?" + re.escape(k), text), (f, k)
