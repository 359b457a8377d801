"""CPU suite: every launch decision of Eq. 8, and what a refused call returns.

digat_amd/csrc/digat_xattn_plan.h holds the limits of the Eq. 8 kernels, the tile plan of the all-pairs score kernel and one route
per entry that chooses kernels, in plain C++; tests/xattn_plan_common.py builds it with the host compiler, and this test pins the
whole result of every route for the inputs of tests/golden/xattn_plan_table.json.

The expected rows were recorded from the code before the header existed: the decision lines of plan_xattn, launch_score,
launch_xattn_pairwise, launch_agg / launch_agg_1024, launch_sparse, launch_sparse_train, sparse_l0_ok / launch_sparse_l0,
xattn_pairwise_fwd_train_flag and xattn_pairwise_bwd_ld, copied verbatim into a stand-alone program with every pointer turned into
"was it passed" and every launch into a record of its instantiation, grid, block and LDS bytes, evaluated on the table's inputs (and,
against the header, on 200 000 random ones: no difference).  One difference is deliberate and is not in the rows: the training forward
of an all-pairs launch with d > 1024 used to launch the score kernel before its aggregation refused the shape; the route refuses it
before anything is launched (same status).

A row is {"name", "route", "in": the inputs that were given (the others are 0), "want": the route's result line}; see xattn_plan_common.py for the format.
"""
import json
import os
import re

import xattn_plan_common as X
from conftest import REPO

ARG, SHAPE = 1, 2                                   # DIGAT_ERR_ARG, DIGAT_ERR_SHAPE
TABLE = json.load(open(os.path.join(REPO, "tests", "golden", "xattn_plan_table.json")))
# every instantiation of an Eq. 8 kernel the library launches
INSTANTIATED = ({f"{k}<{U}>" for k in ("SMALL_LDS", "SMALL") for U in (1, 2, 4)} | {"TILE", "AGG<512>", "AGG<1024>"} |
                {f"SPARSE<{U},{v}>" for U in (1, 2, 4) for v in ("0,0,0", "0,1,0", "1,0,0", "2,0,0", "0,0,1")} |
                {"TWIN<1,2>", "TWIN<2,2>", "L0<1,4>", "L0<2,4>", "SPARSE_BWD<1>", "SPARSE_BWD<2>", "PAIR_BWD<64>", "PAIR_BWD<32>"})


def test_routes_pin_every_decision():
    got = X.run([(r["route"], r["in"]) for r in TABLE])
    assert len({r["name"] for r in TABLE}) == len(TABLE)
    for r, g in zip(TABLE, got):
        assert g == r["want"], r["name"]


def test_table_reaches_every_kernel_refusal_and_threshold():
    rows = [(r["route"], r["in"], X.parse(r["want"])) for r in TABLE]
    of = lambda route: [(i, w) for r, i, w in rows if r == route]
    has = lambda route, **f: any(all(i.get(k, 0) == v for k, v in f.items()) for i, _ in of(route))

    # every kernel family and every template-parameter combination the library instantiates, and nothing else
    names = {X.kernel_name(v) for _, _, w in rows for k, v in w.items() if isinstance(v, list) and k != "tile"}
    assert names - {"NONE"} == INSTANTIATED, names ^ INSTANTIATED
    guards = {(X.KERNELS[X.launch_of(v)["kernel"]], X.launch_of(v)["guard"]) for _, _, w in rows for k, v in w.items() if isinstance(v, list) and k != "tile"}
    assert {("TILE", 1), ("SMALL", 1), ("SMALL_LDS", 1), ("AGG", 1), ("SPARSE", 2), ("SPARSE_BWD", 2), ("PAIR_BWD", 1)} <= guards
    assert all((k, 0) in guards for k in X.KERNELS[1:]) and not {("TWIN", 1), ("TWIN", 2), ("L0", 1), ("L0", 2)} & guards

    # every refusal of every route
    assert {w["tile"][0] for _, w in of("tile")} == {0, ARG, SHAPE}
    assert {w["status"] for _, w in of("pair")} == {0, ARG, SHAPE} and {w["status"] for _, w in of("train_fwd")} == {0, ARG, SHAPE}
    assert {w["agg.status"] for _, w in of("agg")} == {0, SHAPE} and {w["eligible"] for _, w in of("l0")} == {0, 1}
    refused = lambda route, **f: [w["status"] for i, w in of(route) if all(i.get(k, 0) == v for k, v in f.items())]
    assert set(refused("pair", B=3, bindex=1, alpha_wanted=1)) == {SHAPE} and set(refused("pair", bindex=1, live=1)) == {SHAPE}
    assert set(refused("pair", bindex=1, group=1)) == {SHAPE} and set(refused("pair", n=17, d=36, radd=1)) == {SHAPE}       # radd, bindex: small graphs only
    assert refused("pair", n=10, d=36, radd=1, bindex=1, alpha_wanted=0) == [0] and refused("pair", B=0, bindex=1, alpha_wanted=1) == [0]
    assert set(refused("sparse", n=129)) == {SHAPE} and set(refused("sparse", d4=257)) == {SHAPE} and set(refused("sparse", n=128, d4=100)) == {0}
    assert refused("sparse", pq16=1, radd=1) == [SHAPE] and refused("sparse", pq16=2, radd=1) == [SHAPE]                    # low-precision rows carry K3 already
    assert refused("sparse", pq16=1, d4=41) == [SHAPE] and refused("sparse", pq16=1, d4=40) == [0]                            # bf16 rows: whole 16-byte pieces
    assert refused("sparse", pq16=2, d4=30) == [SHAPE] and refused("sparse", pq16=2, d4=40) == [0]                            # e4m3 rows: whole 80-channel strips
    assert refused("sparse", pq16=2, ld8=419) == [SHAPE] and set(refused("sparse", pq16=2, ld8=428)) == {SHAPE} and refused("sparse", pq16=2, ld8=424) == [0]
    assert SHAPE in refused("train_fwd", n=67, d=1028) and SHAPE in refused("train_fwd", n=16, d=1028)                        # the aggregation's 1024 channels
    assert all(w["agg.status"] == (SHAPE if i["upto_1024"] and i["d"] > 1024 else 0) for i, w in of("agg") if "upto_1024" in i)

    # both sides of every threshold
    for route in ("pair", "train_fwd", "train_bwd"):
        for n in (16, 17, 44, 45, 128):
            assert has(route, n=n) or route != "pair" and n in (44, 45), (route, n)
        for d in (256, 260, 512, 516, 1024, 1028):
            assert has(route, d=d), (route, d)
    assert has("tile", n=44) and has("tile", n=45) and has("tile", n=128) and has("tile", n=129) and has("pair", n=129) and has("train_fwd", n=129)
    rb = lambda n: {w["tile"][X.TILE.index("RB")] for i, w in of("tile") if i["n"] == n and i["B"] > 1}
    assert rb(44) == {1, 2} and rb(45) == {1}                                          # one graph per workgroup from 128 tiles
    assert has("train_bwd", n=112) and has("train_bwd", n=113)
    assert {X.launch_of(w["pair"])["ch"] for i, w in of("train_bwd") if i["n"] in (112, 113) and w["pair"][0]} == {64, 32}
    lds_rows = {(i["n"] * i["d"] // 4 <= 2048, X.KERNELS[w["score"][0]]) for i, w in of("pair") if i["n"] <= 16 and i["d"] <= 1024 and w["fused"]}
    assert has("pair", n=16, d=512) and has("pair", n=16, d=516) and lds_rows == {(True, "SMALL_LDS"), (False, "SMALL")}         # n d / 4 = 2048
    assert {w["agg.groups"] for _, w in of("agg")} >= {8, 9, 16, 17}
    assert {(i["d4"] % 20 == 0, i["d4"] % 2 == 0) for i, _ in of("sparse") if i.get("pq16")} == {(True, True), (False, True), (False, False)}
    # guarded and unguarded grids on both sides of their caps: 2048 workgroups (inference), 8192 (training), 8192 (twins)
    for train, cap in ((0, 2048), (1, 8192)):
        g = {(i.get("run_if", 0), (i["B"] * i["n"] + 3) // 4 > cap, X.launch_of(w["launch"])["grid"] > cap) for i, w in of("sparse")
             if i.get("train", 0) == train and not i.get("twin") and w["status"] == 0}
        assert {(1, False, False), (1, True, False), (0, False, False), (0, True, True)} <= g, (train, g)
    tw = {((i["B"] * i["n"] + 3) // 4 > 8192, X.launch_of(w["launch"])["grid"]) for i, w in of("sparse") if X.KERNELS[w["launch"][0]] == "TWIN"}
    assert {c for c, _ in tw} == {False, True} and max(g for _, g in tw) == 8192
    # the twin route with each of its preconditions switched off in turn, the layer-0 route likewise
    twin_on = dict(twin=1, rowidx=1, live=1, nrows_dev=1)
    kern = lambda **f: [X.KERNELS[w["launch"][0]] for i, w in of("sparse") if i == {**dict(B=64, n=67, d4=100), **f}]
    assert kern(**twin_on) == ["TWIN"]
    for off in (dict(twin=0), dict(rowidx=0), dict(pq16=1), dict(radd=1), dict(group=1), dict(run_if=1), dict(fill_flags=1)):
        assert kern(**{**twin_on, **off}) == ["SPARSE"], off
    assert [X.KERNELS[w["launch"][0]] for i, w in of("sparse") if i.get("twin") and i["d4"] in (128, 129) and i["B"] == 64] == ["TWIN", "SPARSE"]
    l0_on = dict(group=1, xgroup=1, radd=1, rowidx=1, nrows_dev=1, live=1)
    elig = lambda **f: [w["eligible"] for i, w in of("l0") if i == {**dict(B=64, n=67, d4=100, G=8), **f}]
    for off in (dict(group=0), dict(xgroup=0), dict(radd=0), dict(rowidx=0), dict(nrows_dev=0), dict(live=0), dict(run_if=1), dict(pq16=1), dict(fill_flags=1),
                dict(centre_limit=50)):
        assert elig(**{**l0_on, **off}) == [0], off
    assert [w["eligible"] for i, w in of("l0") if i["d4"] in (128, 129) and i["n"] == 67] == [1, 0]
    assert [w["eligible"] for i, w in of("l0") if i["n"] in (128, 129)] == [1, 0]
    # training: modes 0, 1, 2, each with and without the flag and with and without dr; every path of the forward, every state of the backward
    for route in ("train_fwd", "train_bwd"):
        assert {(i.get("mode", 0), i.get("flag", 0), i.get("dr", 0)) for i, _ in of(route) if i.get("n") == 67 and i.get("d") == 400} == \
               {(m, f, r) for m in (0, 1, 2) for f in (0, 1) for r in (0, 1)}
    assert {w["path"] for _, w in of("train_fwd")} == {0, 1, 2, 3, 4}
    assert {(w["only_sparse"], w["guard"]) for _, w in of("train_bwd")} == {(0, 0), (1, 0), (0, 1)}
    # the known asymmetry: for 512 < d <= 1024 a forward that ran entry-wise is followed by the all-pairs backward
    fwd = {tuple(sorted(i.items())): w["path"] for i, w in of("train_fwd")}
    bwd = {tuple(sorted(i.items())): (w["only_sparse"], w["guard"]) for i, w in of("train_bwd")}
    key = tuple(sorted(dict(B=3, n=67, d=516, mode=1, flag=1, dr=1).items()))
    assert fwd[key] == 2 and bwd[key] == (0, 0) and bwd[tuple(sorted(dict(B=3, n=67, d=512, mode=1, flag=1, dr=1).items()))] == (1, 0)


def test_plan_structs_have_no_member_the_harness_does_not_print():
    text = open(X.HEADER).read()
    for name, want in {**X.MEMBERS, **X.INPUTS}.items():
        body = re.search(r"struct %s \{(.*?)\n?\};" % name, text, re.S).group(1)
        members = set()
        for line in body.splitlines():
            for part in line.split("//")[0].split(";"):
                members.update(part.replace(",", " ").split()[1:])
        assert members == set(want), (name, members ^ set(want))
    enum = re.search(r"enum Eq8Kernel \{(.*?)\};", text, re.S).group(1)
    assert tuple(re.findall(r"EQ8_(\w+),", enum)) == X.KERNELS


def test_tile_plan_sweep():
    """Every n in 1 .. 128, every d in 4 .. 4096 in steps of 4, B in {1, 3, 4096}: a plan exists, and it satisfies what
    xattn_score_kernel relies on (the conditions are written out in the harness's sweep(), none of them a tuned number): total LDS
    <= 160 KiB; the DMA ring <= 60 KiB (it is addressed through M0: the first 64 KiB); ninstr <= XA_KMAX x waves; a thread per tile
    flag and per image row; threads a multiple of 64, <= 1024; CC4 x nchunks == d / 4; the byte image (RB n^2 + 32), the score area
    and the ring end at or below am_off; am_off, a_off multiples of 16; 1 <= RB <= B; blocks == ceil(B / RB); the LDS areas in order."""
    line = X.run([("sweep", {})])[0]
    print(line)
    res = X.parse(re.sub(r"\[.*?\]", "", line))
    assert res["plans"] == 128 * 1024 * 3 and res["missing"] == 0 and res["violations"] == 0
    # the search is the one that was recorded: as many plans beyond 64 KiB (they raise the kernel's LDS attribute), the same largest one
    assert res["over64k"] == 52587 and res["maxlds"] == 90176
