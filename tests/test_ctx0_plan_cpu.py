"""CPU suite: when the folded pass's first user context is the GEMM + ``user_ctx0_kernel`` pair (csrc/digat_encoder_plan.h:
``ctx0_fits``, ``encoder_plan_ctx0``), pinned with the host compiler like the rest of the plan; and the new export's signature."""
import shutil
import subprocess

from conftest import REPO

HARNESS = r"""
#include <stdio.h>
#include "digat_amd/csrc/digat_encoder_plan.h"
static int bit(int variant, int N, int H, int C, int d, bool folded) {
    EncoderPlanIn in = {};
    in.flags = 2; in.B = 4096; in.N = N; in.H = H; in.C = C; in.d = d; in.L = 3; in.G = variant == ENC_GROUPED ? 110 : 0; in.variant = variant;
    in.folded = folded;
    return encoder_plan_ctx0(in) ? 1 : 0;
}
int main() {
    const int variants[3] = {ENC_PLAIN, ENC_GROUPED, ENC_SHARED};
    const int Ns[3] = {10, 26, 65}, Cs[2] = {17, 18};
    for (int v = 0; v < 3; ++v) for (int n = 0; n < 3; ++n) for (int c = 0; c < 2; ++c)
        printf("bench %d %d %d %d\n", variants[v], Ns[n], Cs[c], bit(variants[v], Ns[n], 50, Cs[c], 400, true));
    printf("unfolded %d\n", bit(ENC_PLAIN, 10, 50, 17, 400, false));
    printf("H65 %d\n", bit(ENC_PLAIN, 10, 65, 17, 400, true));
    printf("H64 %d\n", bit(ENC_PLAIN, 10, 64, 17, 400, true));
    printf("H53d516 %d\n", bit(ENC_PLAIN, 10, 53, 17, 516, true));
    printf("H52d1024 %d\n", bit(ENC_PLAIN, 10, 52, 7, 1024, true));
    printf("d1028 %d\n", bit(ENC_PLAIN, 10, 50, 7, 1028, true));
    printf("d402 %d\n", bit(ENC_PLAIN, 10, 50, 17, 402, true));
    printf("C64 %d\n", bit(ENC_PLAIN, 10, 50, 64, 64, true));
    printf("lds_over %d\n", bit(ENC_PLAIN, 10, 50, 40, 400, true));       /* 41 x 400 floats = 65.6 KB of pooled topics alone */
    printf("lds_under %d\n", bit(ENC_PLAIN, 10, 50, 31, 400, true));
    printf("bytes %zu %zu\n", ctx0_lds_bytes(50, 18, 400), ctx0_lds_bytes(52, 64, 1024));
    return 0;
}
"""


def test_ctx0_plan_bit(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    src = tmp_path / "ctx0.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "ctx0"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}", str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, _, val = line.rpartition(" ") if not line.startswith("bytes") else ("bytes", "", line.split(" ", 1)[1])
        got[key] = val
    bench = {k: v for k, v in got.items() if k.startswith("bench")}
    assert len(bench) == 18 and set(bench.values()) == {"1"}, bench          # N = 10 / 26 / 65, C = 17 / 18, all three variants
    assert got["unfolded"] == "0"                                             # the training-shaped path keeps its entries
    assert got["H65"] == "0" and got["H64"] == "1"
    assert got["H53d516"] == "0" and got["H52d1024"] == "1"                   # the 16-step instantiation runs at most 512 threads
    assert got["d1028"] == "0" and got["d402"] == "0"
    assert got["C64"] == "0"                                                  # C + 1 = 65 buckets: more than a wave's lanes
    assert got["lds_over"] == "0" and got["lds_under"] == "1"
    # the bench shape's image: M 2 x 16 x 51, seven waves of score scratch, the tables, [18, 400] pooled topics; two fit a CU with room
    a, b = (int(x) for x in got["bytes"].split())
    assert a == (2 * 16 * 51 + 7 * 64 + 3 * 64 + 68 + 16 + 18 * 400) * 4 and a <= 64 * 1024 < b


def test_ctx0_export_is_declared_and_bound():
    from digat_amd import _lib
    assert "digat_user_ctx0_fwd" in _lib.EXPORTED
    res, args = _lib._SIGNATURES["digat_user_ctx0_fwd"]
    assert len(args) == 20
    header = open(f"{REPO}/include/digat_hip.h").read()
    decl = header.split("int digat_user_ctx0_fwd(")[1].split(");")[0]
    assert decl.count(",") + 1 == len(args)
    assert "#define DIGAT_ABI_VERSION 4" in header.replace("  ", " ")
