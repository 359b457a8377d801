"""CPU suite: every decision of an encoder call, and what a refused call returns.

digat_amd/csrc/digat_encoder_plan.h holds the decisions of one encoder call (encoder_plan) in plain C++; this test builds it with the
host compiler and pins the whole EncoderPlan, or the refusal status, for the inputs of tests/golden/encoder_plan_table.json.
The expected rows were recorded from the previous code: the predicate lines of encoder_fwd_impl / encoder_fwd_folded (and the
checks of the public entries), copied into a stand-alone program with every pointer turned into "was it passed", evaluated on the
same inputs.  A call that takes another path fails here even where the other path's results would match.

A row's `in` holds what differs from DEFAULT; `want` is "status" for a call refused before the carve, else
"0|status after the carve|the mode fields|the boolean fields that are set".
"""
import json
import os
import shutil
import subprocess

from conftest import REPO

DEFAULT = dict(flags=2, B=64, N=10, H=50, C=17, d=400, L=2, G=0, variant=0, folded=1, c_n0=0, news_hpq0=0, hist_hpq0=0, topic_hpq0=0,
               ctxq0=0, news_index=0, news_rows=0, fsplit=0, ctx_fused_fits=1)
INTS = ("flags", "B", "N", "H", "C", "d", "L", "G", "variant")
BOOLS_IN = ("folded", "c_n0", "news_hpq0", "hist_hpq0", "topic_hpq0", "ctxq0", "news_index", "fsplit", "ctx_fused_fits")
MODES = {"sparse_mode": {0, 1, 2}, "pq_x3": {0, 1}, "pq_mode": set(range(8)), "fmt": {0, 1}, "lfmt": {0, 1, 2}, "bd_disp": {1, 1 << 30},
         "news_sparse_mode": {1, 2}, "side_mode": {0, 1, 2}}
BOOLS = ("folded", "shared", "by_group", "xu0_grouped", "xu0_shared", "c_n0_in_place", "ctxq0", "want_live", "want_scan", "l0_chunked", "twins",
         "l0_sparse", "l0_dense", "group_tables", "news_early", "news_lists", "news_cached0", "news_indexed0", "user_ctx_fused", "side_wanted")

HARNESS = r"""
#include <stdio.h>
#include "digat_amd/csrc/digat_encoder_plan.h"
static void run(const char* name, const EncoderPlanIn& in) {
    const EncoderPlan p = encoder_plan(in);
    if (p.status) { printf("%s|%d\n", name, p.status); return; }
    printf("%s|0|%d|""" + " ".join(f"{m}=%d" for m in MODES) + r"""|", name, p.status_after_carve, """ + ", ".join(f"p.{m}" for m in MODES) + r""");
""" + "\n".join(f'    if (p.{b}) printf(" {b}");' for b in BOOLS) + r"""
    printf("\n");
}
int main() {
"""


def _case_source(name, fields):
    v = {**DEFAULT, **fields}
    s = ["{ EncoderPlanIn in = {};"]
    s += [f"in.{k} = {v[k]};" for k in INTS]
    s += [f"in.{k} = {'true' if v[k] else 'false'};" for k in BOOLS_IN]
    s.append(f'in.news_rows = {v["news_rows"]}LL; run("{name}", in); }}')
    return " ".join(s)


def test_encoder_plan_pins_every_decision(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the torch extension is built with g++ too)"
    table = json.load(open(os.path.join(REPO, "tests", "golden", "encoder_plan_table.json")))
    src = tmp_path / "plan.cpp"
    src.write_text(HARNESS + "\n".join(_case_source(r["name"], r["in"]) for r in table) + "\nreturn 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}", str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(l.split("|", 1) for l in lines)
    assert len(lines) == len(table) == len(got)
    for r in table:
        assert got[r["name"]].strip() == r["want"], r["name"]

    # the table reaches every refusal, both states of every boolean field and every value of every mode field
    whole = [r["want"].split("|") for r in table if "|" in r["want"]]
    assert {r["want"] for r in table if "|" not in r["want"]} == {"1", "2"}          # DIGAT_ERR_ARG, DIGAT_ERR_SHAPE before the carve
    assert {w[1] for w in whole} == {"0", "1"}                                        # news_index admitted and refused
    for b in BOOLS:
        assert {b in w[3].split() for w in whole} == {False, True}, b
    for m, values in MODES.items():
        seen = {int(kv.split("=")[1]) for w in whole for kv in w[2].split() if kv.split("=")[0] == m}
        assert seen == values, (m, seen)
    # every field of the plan is pinned: the struct has no member the harness does not print
    text = open(os.path.join(REPO, "digat_amd", "csrc", "digat_encoder_plan.h")).read()
    body = text.split("struct EncoderPlan {")[1].split("};")[0]
    members = set()
    for line in body.splitlines():
        decl = line.split("//")[0].strip()
        for part in decl.split(";"):
            words = part.replace(",", " ").split()
            members.update(words[1:])
    assert members == set(BOOLS) | set(MODES) | {"status", "status_after_carve"}, members ^ (set(BOOLS) | set(MODES))
