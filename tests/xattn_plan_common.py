"""Shared by tests/test_xattn_plan_cpu.py and tests/test_eq8_fp64_cpu.py: digat_amd/csrc/digat_xattn_plan.h built with the host
compiler into one small program that reads a route and its inputs per line and prints the route's whole result on one line.

A request is (route, {input field: value}); fields left out are 0 / false.  A result line is "status=.. field=.. ..", a launch
(Eq8Launch) printed as launch=kernel:U:pq16:... in the order of LAUNCH, a tile plan (XattnTile) as tile=... in the order of TILE.
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

from conftest import REPO

HEADER = os.path.join(REPO, "digat_amd", "csrc", "digat_xattn_plan.h")
KERNELS = ("NONE", "SMALL_LDS", "SMALL", "TILE", "AGG", "SPARSE", "TWIN", "L0", "SPARSE_BWD", "PAIR_BWD")            # Eq8Kernel, in order
LAUNCH = ("kernel", "U", "pq16", "R", "maxt", "ch", "radd", "train", "grid", "grid_y", "block", "lds", "raise_lds", "xcd_group", "guard")
TILE = ("status", "B", "n", "d", "d4", "NT", "SN", "CC4", "nchunks", "RB", "img_slots", "ring_slots", "ninstr", "am_off", "a_off", "tl_off",
        "ld_off", "pm_off", "threads", "lds", "blocks")
# the inputs of each route (the members of its input struct, or its arguments), and the members of what it returns
ROUTES = {
    "tile": (("B", "n", "d"), None),
    "agg": (("B", "n", "d", "upto_1024", "guard"), "Eq8AggRoute"),
    "pair": (("B", "n", "d", "alpha_wanted", "live", "group", "radd", "bindex", "guarded"), "Eq8PairRoute"),
    "sparse": (("B", "n", "d4", "train", "radd", "group", "xgroup", "live", "run_if", "fill_flags", "rowidx", "nrows_dev", "twin", "pq16",
                "centre_limit", "ld8"), "Eq8SparseRoute"),
    "l0": (("B", "n", "d4", "train", "radd", "group", "xgroup", "live", "run_if", "fill_flags", "rowidx", "nrows_dev", "twin", "pq16",
            "centre_limit", "ld8", "G"), "Eq8L0Route"),
    "train_fwd": (("B", "n", "d", "mode", "flag", "dr"), "Eq8TrainFwdRoute"),
    "train_bwd": (("B", "n", "d", "mode", "flag", "dr"), "Eq8TrainBwdRoute"),
}
# the members of every struct a route returns, as the harness prints them (test_xattn_plan_cpu.py holds the header to these lists)
MEMBERS = {
    "Eq8Launch": LAUNCH, "XattnTile": TILE,
    "Eq8AggRoute": ("status", "groups", "sa", "launch"),
    "Eq8PairRoute": ("status", "fused", "tile", "score", "agg"),
    "Eq8SparseRoute": ("status", "launch"),
    "Eq8L0Route": ("eligible", "launch"),
    "Eq8TrainFwdRoute": ("status", "path", "tile", "sparse", "score", "agg"),
    "Eq8TrainBwdRoute": ("only_sparse", "guard", "sparse", "pair"),
}
INPUTS = {"Eq8PairIn": ROUTES["pair"][0], "Eq8SparseIn": ROUTES["sparse"][0], "Eq8TrainIn": ROUTES["train_fwd"][0]}

HARNESS = r"""
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <map>
#include <string>
#include "digat_amd/csrc/digat_xattn_plan.h"
typedef std::map<std::string, long> In;
static void launch(const char* tag, const Eq8Launch& l) {
    printf(" %s=""" + ":".join("%ld" for _ in LAUNCH) + r"""", tag, """ + ", ".join(f"(long)l.{m}" for m in LAUNCH) + r""");
}
static void tile(const XattnTile& t) {
    printf(" tile=""" + ":".join("%ld" for _ in TILE) + r"""", """ + ", ".join(f"(long)t.{m}" for m in TILE) + r""");
}
static void agg(const char* tag, const Eq8AggRoute& r) { printf(" %s.status=%d %s.groups=%d %s.sa=%d", tag, r.status, tag, r.groups, tag, r.sa); launch(tag, r.launch); }
static Eq8SparseIn sparse_in(In& v) {
    Eq8SparseIn in = {};
""" + "\n".join(f'    in.{m} = v["{m}"];' for m in ROUTES["sparse"][0]) + r"""
    return in;
}
static Eq8TrainIn train_in(In& v) {
    Eq8TrainIn in = {};
""" + "\n".join(f'    in.{m} = v["{m}"];' for m in ROUTES["train_fwd"][0]) + r"""
    return in;
}
// the tile plan at every n, every d up to 4096 and three batch sizes: the conditions the tile kernel's code relies on
static void sweep() {
    long plans = 0, missing = 0, bad = 0, over64k = 0, maxlds = 0;
    const int Bs[3] = {1, 3, 4096};
    for (int n = 1; n <= 128; ++n) for (int d = 4; d <= 4096; d += 4) for (int B : Bs) {
        const XattnTile t = xattn_tile_plan(B, n, d);
        if (t.status) { ++missing; continue; }
        ++plans;
        const long ringb = (long)XA_RING * t.ring_slots * 16;
        const char* why = nullptr;
        if ((long)t.lds > 160 * 1024) why = "total LDS above 160 KiB";
        else if (ringb > 60 * 1024) why = "the DMA ring above 60 KiB";
        else if (t.ninstr > XA_KMAX * (t.threads / 64)) why = "more DMA instructions per chunk than XA_KMAX per wave";
        else if (t.RB * t.NT * t.NT > t.threads) why = "fewer threads than tile flags";
        else if (2 * t.RB * 4 * t.NT > t.threads) why = "fewer threads than image rows";
        else if (t.threads % 64 || t.threads > 1024 || t.threads <= 0) why = "threads";
        else if (t.CC4 < 1 || t.CC4 * t.nchunks != t.d4 || t.d4 * 4 != d) why = "chunks do not tile the row";
        else if ((long)t.RB * n * n + 32 > t.am_off) why = "the byte image of phase 0 reaches the adjacency bit rows";
        else if ((long)t.RB * n * t.SN * 4 > t.am_off) why = "the score area reaches the adjacency bit rows";
        else if (ringb > t.am_off) why = "the ring reaches the adjacency bit rows";
        else if (t.am_off % 16 || t.a_off % 16) why = "am_off / a_off not 16-byte aligned";
        else if (t.RB < 1 || t.RB > B) why = "RB outside 1 .. B";
        else if (t.blocks != (B + t.RB - 1) / t.RB) why = "blocks != ceil(B / RB)";
        else if (t.NT != (n + 3) / 4 || t.SN != 4 * t.NT || t.img_slots != t.RB * 4 * t.NT * t.CC4 || t.ring_slots % 64 || t.ring_slots < 2 * t.img_slots ||
                 t.ninstr * 64 != t.ring_slots) why = "image geometry";
        else if (!(t.am_off < t.a_off && t.a_off + 4 * d == t.tl_off && t.tl_off < t.ld_off && t.ld_off < t.pm_off && (size_t)t.pm_off < t.lds)) why = "LDS areas out of order";
        if (why) { if (++bad <= 5) printf(" [n=%d d=%d B=%d: %s]", n, d, B, why); }
        if (t.lds > 64 * 1024) ++over64k;
        if ((long)t.lds > maxlds) maxlds = (long)t.lds;
    }
    printf(" plans=%ld missing=%ld violations=%ld over64k=%ld maxlds=%ld", plans, missing, bad, over64k, maxlds);
}
int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        In v;
        char* route = strtok(line, " \n");
        if (!route) continue;
        for (char* t = strtok(nullptr, " \n"); t; t = strtok(nullptr, " \n")) { char* eq = strchr(t, '='); *eq = 0; v[t] = atol(eq + 1); }
        const std::string r = route;
        printf("%s", route);
        if (r == "tile") tile(xattn_tile_plan(v["B"], v["n"], v["d"]));
        else if (r == "agg") agg("agg", eq8_agg_route(v["B"], v["n"], v["d"], v["upto_1024"], v["guard"]));
        else if (r == "pair") {
            Eq8PairIn in = {};
""" + "\n".join(f'            in.{m} = v["{m}"];' for m in ROUTES["pair"][0]) + r"""
            const Eq8PairRoute p = eq8_pair_route(in);
            printf(" status=%d fused=%d", p.status, p.fused); tile(p.tile); launch("score", p.score); agg("agg", p.agg);
        } else if (r == "sparse") {
            const Eq8SparseRoute p = eq8_sparse_route(sparse_in(v));
            printf(" status=%d", p.status); launch("launch", p.launch);
        } else if (r == "l0") {
            const Eq8L0Route p = eq8_l0_route(sparse_in(v), v["G"]);
            printf(" eligible=%d", p.eligible); launch("launch", p.launch);
        } else if (r == "train_fwd") {
            const Eq8TrainFwdRoute p = eq8_train_fwd_route(train_in(v));
            printf(" status=%d path=%d", p.status, p.path); tile(p.tile); launch("sparse", p.sparse); launch("score", p.score); agg("agg", p.agg);
        } else if (r == "train_bwd") {
            const Eq8TrainBwdRoute p = eq8_train_bwd_route(train_in(v));
            printf(" only_sparse=%d guard=%d", p.only_sparse, p.guard); launch("sparse", p.sparse); launch("pair", p.pair);
        } else if (r == "sweep") sweep();
        else return 2;
        printf("\n");
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def harness():
    """The compiled harness (once per session)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    tmp = tempfile.mkdtemp(prefix="xattn_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    src = os.path.join(tmp, "plan.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{REPO}", src, "-o", os.path.join(tmp, "plan")], check=True)
    return os.path.join(tmp, "plan")


def request_line(route, fields):
    assert set(fields) <= set(ROUTES[route][0]) if route in ROUTES else not fields, (route, fields)
    return " ".join([route] + [f"{k}={int(v)}" for k, v in fields.items()])


def run(requests, exe=None):
    """[(route, fields)] -> the result line of each, without the route's name."""
    text = "".join(request_line(r, f) + "\n" for r, f in requests)
    out = subprocess.run([exe or harness()], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(requests)
    return [line.split(" ", 1)[1] if " " in line else "" for line in out]


def parse(line):
    """A result line as {field: int, or [ints] for a launch / tile}."""
    res = {}
    for kv in line.split():
        k, v = kv.split("=")
        res[k] = [int(x) for x in v.split(":")] if ":" in v else int(v)
    return res


def launch_of(fields):
    return dict(zip(LAUNCH, fields))


def kernel_name(fields):
    """A launch as the kernel instantiation it stands for, e.g. 'SPARSE<2,0,0,0>'."""
    l = launch_of(fields)
    k = KERNELS[l["kernel"]]
    params = {"SMALL_LDS": ("U",), "SMALL": ("U",), "AGG": ("maxt",), "SPARSE": ("U", "pq16", "radd", "train"), "TWIN": ("U", "R"),
              "L0": ("U", "R"), "SPARSE_BWD": ("U",), "PAIR_BWD": ("ch",)}.get(k, ())
    return k + ("<" + ",".join(str(l[p]) for p in params) + ">" if params else "")
