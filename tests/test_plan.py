"""Traversal planning (qt-raytracer_amd/csrc/hippt_plan.h) from a host-compiled driver of
the product's own planner: tests/native/plan_check.cpp.  The yardstick is a recording of every scalar a
launch received at the commit before the planner existed (tests/golden/traversal_plan_parent.json: the
megakernel, wavefront, chained and query launch sites over a matrix of scenes and options on an MI355X):
the planner, fed a row's facts, options and call, returns the row's values exactly.  The chained run's
ring (chain_cap, ring_slots, ring_plan) has its own recording, tests/golden/ring_plan_parent.json.  No GPU.
"""
import json
import os
import subprocess

import pytest

from plan_rows import load_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "qt-raytracer_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "plan_check.cpp")

FACTS = ("numNodes", "numNodes4", "numTris", "numMats", "levels", "stackBound4", "full", "quantTree", "halfTree")
KNOBS = ("bvhWidth", "ldsScene", "stackCap", "bvhQuant", "ldsTopNodes", "cameraPool", "pathMode", "waveThreshold",
         "leafExit", "nodeExit", "chunk", "countTraversal", "fuseCombine", "chainBatches", "renderPad", "skyRect")
OUT = ("wide", "numNodes", "ldsScene", "stackCap", "stackDepth", "spills", "spillCap", "fmt", "poolWords", "topBytes",
       "poolOffset", "refBits", "waveThreshold", "leafExit", "nodeExit", "fuse", "mayChain", "trimWanted", "chunk0",
       "chunk1", "skyWanted0", "skyWanted1", "wantsHalf")
K_WIDE2, K_FLOAT, K_QUANT, K_HYBRID, K_HALF = range(5)
QUERY_KINDS = {(0, 0, 0): "hipptTraceRays", (1, 0, 0): "hipptOccluded", (0, 1, 0): "hipptTraceCamera",
               (0, 0, 1): "hipptTraceHits", (0, 1, 1): "hipptTraceCameraHits"}


def is_query(row):
    return row["site"] == "launch_query"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    path = str(d / "plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", path, SRC], check=True)
    return path


@pytest.fixture(scope="module")
def planned(exe, tmp_path_factory):
    """plans(cases): the planner's output for (row, knob overrides, profile) cases, as dicts."""
    d = tmp_path_factory.mktemp("plan_rows")
    count = [0]

    def plans(cases):
        path = str(d / ("cases%d.txt" % count[0]))
        count[0] += 1
        with open(path, "w") as f:
            for row, over, profile in cases:
                knobs = dict(row["knobs"], **over)
                c = row["ctx"]
                call = [profile, 0, 0, 2, 0] if is_query(row) else [profile, c["pinhole"], c["copy"], c["maxDepth"], c["total"]]
                vals = [row["facts"][k] for k in FACTS] + [knobs[k] for k in KNOBS] + \
                       [row["limits"]["scene"], row["limits"]["block"]] + call
                f.write(" ".join(str(int(v)) for v in vals) + "\n")
        r = subprocess.run([exe, "rows", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return [dict(zip(OUT, map(int, line.split()))) for line in lines]

    return plans


def test_the_header_compiles_with_gpp_alone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "hippt_plan.h"\nint main() { return hippt::plan::layout({}, {}, {}, false).stackDepth == 1 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "t"), str(src)], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_the_recording_covers_every_branch():
    rows = load_rows()
    render = [r for r in rows if not is_query(r)]
    out = [r["out"] for r in render]
    for fmt in (K_WIDE2, K_FLOAT, K_QUANT, K_HYBRID, K_HALF):
        assert any(o["wide"] == fmt for o in out), "node format %d" % fmt
    for v in (0, 1):
        assert any(o["ldsScene"] == v for o in out), "ldsScene %d" % v
        assert any(o["spills"] == v for o in out), "spills %d" % v
        assert any(r["ctx"]["chained"] == v for r in render), "chained %d" % v
        assert any(r["ctx"]["cnt"] == v for r in render), "cnt %d" % v
        assert any(r["knobs"]["pathMode"] == v for r in render), "pathMode %d" % v
    global_wide = [r for r in render if r["out"]["wide"] != K_WIDE2 and not r["out"]["ldsScene"]]
    assert any(r["out"]["topBytes"] == 0 for r in global_wide), "no top"
    assert any(r["out"]["topBytes"] > 0 and r["knobs"]["ldsTopNodes"] == -1 for r in global_wide), "automatic top"
    assert any(r["out"]["topBytes"] > 0 and r["knobs"]["ldsTopNodes"] > 0 for r in global_wide), "explicit top"
    # hybrid asked for, where the stack leaves none of the block budget for a top: 8-bit nodes
    assert any(r["knobs"]["bvhQuant"] == 2 and r["knobs"]["pathMode"] == 0 and r["knobs"]["ldsTopNodes"] == -1 and
               r["out"]["wide"] == K_QUANT and r["out"]["topBytes"] == 0 for r in global_wide), "hybrid -> quantized"
    for words in (0, 5, 8):
        assert any(o["poolWords"] == words for o in out), "poolWords %d" % words
    for site in ("launch_mesh", "run_wavefront", "chain_batch", "launch_query"):
        assert any(r["site"] == site for r in rows), site
    kinds = {(r["ctx"]["any"], r["ctx"]["camera"], r["ctx"]["records"]) for r in rows if is_query(r)}
    assert kinds == set(QUERY_KINDS), kinds
    # explicit loop parameters and claim size, and both automatic claim sizes
    assert any(r["knobs"]["waveThreshold"] >= 0 and r["knobs"]["leafExit"] >= 0 and r["knobs"]["nodeExit"] >= 0 and
               r["knobs"]["chunk"] > 0 for r in render)
    assert {256, 512} <= {o["chunk"] for o in out}


def test_the_planner_returns_every_recorded_row(planned):
    rows = load_rows()
    got = planned([(r, {}, 1 if is_query(r) else 0) for r in rows])
    for r, g in zip(rows, got):
        o, where = r["out"], (r["scene"], r["over"], r["site"])
        for key in ("numNodes", "ldsScene", "stackCap", "stackDepth", "topBytes", "waveThreshold", "leafExit", "nodeExit"):
            assert g[key] == o[key], (where, key)
        if is_query(r):
            # (hippt_api.cpp query_setup: the query kernel takes a spill area whenever the tree is 4-wide)
            assert g["wide"] == o["wide"] and g["fmt"] == (K_FLOAT if o["wide"] else K_WIDE2), where
            assert g["spillCap"] == o["spillCap"] and g["poolWords"] == 0, where
            assert o["chunk"] == (256 if r["ctx"]["numRays"] >= 1 << 20 else 64), where
            continue
        chained = r["ctx"]["chained"]
        assert g["fmt"] == o["wide"] and g["wide"] == (o["wide"] != K_WIDE2), where
        assert g["spills"] == o["spills"] and g["spillCap"] == (o["spillCapArg"] if o["wide"] != K_WIDE2 else 0), where
        if r["site"] != "run_wavefront":  # (the wavefront sets MeshParams::spillCap after its launch site)
            assert o["spillCap"] == (g["spillCap"] if g["spills"] else 0), where
        for key in ("poolWords", "poolOffset", "refBits", "mayChain", "trimWanted"):
            assert g[key] == o[key], (where, key)
        assert g["mayChain"] == chained, where  # (the recording's device had room for every ring)
        assert g["chunk%d" % chained] == o["chunk"] and g["skyWanted%d" % chained] == o["skyWanted"], where
        assert o["trimmed"] <= g["trimWanted"], where
        assert g["wantsHalf"] >= r["facts"]["halfTree"] or o["wide"] != K_HALF, where


def test_the_query_profile_is_the_wavefront_over_float_nodes_without_a_pool(planned):
    """query_knobs() against the render rules at PATH_MODE 1, BVH_QUANT 0, CAMERA_POOL 0, spelled out here."""
    rows = load_rows()
    query = planned([(r, {}, 1) for r in rows])
    render = planned([(r, {"pathMode": 1, "bvhQuant": 0, "cameraPool": 0}, 0) for r in rows])
    layout = OUT[:15]
    for r, q, g in zip(rows, query, render):
        for key in layout:
            assert q[key] == g[key], (r["scene"], r["over"], r["site"], key)


def ring_rows():
    """tests/golden/ring_plan_parent.json: chain_cap / ring_plan as they stood in hippt_api.cpp at the commit
    before they moved into hippt_plan.h, over total x HIPPT_OPT_CHAIN x ldsScene x scratch budget."""
    with open(os.path.join(REPO, "tests", "golden", "ring_plan_parent.json")) as f:
        doc = json.load(f)
    return [dict(zip(doc["columns"], row)) for row in doc["rows"]]


def test_the_ring_plan_returns_every_recorded_row(exe, tmp_path):
    rows = ring_rows()
    path = tmp_path / "ring.txt"
    path.write_text("".join("%d %d %d %d\n" % (r["total"], r["option"], r["ldsScene"], r["budget"]) for r in rows))
    out = subprocess.run([exe, "ring", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        got = dict(zip(("cap", "slots", "shift", "bytes"), map(int, line.split())))
        assert got == {k: r[k] for k in got}, r


def test_the_ring_recording_covers_every_branch():
    rows = ring_rows()
    auto = [r for r in rows if r["option"] <= 0]
    # both ceilings of the automatic cap: 8 for LDS-resident scenes, 16 for trees in global memory
    assert any(r["ldsScene"] and r["cap"] == 8 and r["total"] < 4e8 / 8.5 for r in auto)
    assert any(not r["ldsScene"] and r["cap"] == 16 and r["total"] < 4e8 / 16.5 for r in auto)
    # batches of more than a whole image's items: cap 8 whatever the scene
    assert any(not r["ldsScene"] and r["total"] > 1 << 26 and r["cap"] == 8 for r in auto)
    # a cap shrunk to the budget: below what the same case gets with the largest budget
    most = {(r["total"], r["option"], r["ldsScene"]): r["cap"] for r in rows if r["budget"] == 64 << 30}
    assert any(0 < r["cap"] < most[r["total"], r["option"], r["ldsScene"]] for r in rows)
    assert any(r["bytes"] == 0 and r["cap"] == 0 for r in rows), "unchained"
    assert any(r["slots"] == 32 for r in rows), "the 32-slot ring"
    # Recorded, not endorsed: 32 slots of 2^27 items use every bit of an item, so slot 31's last item
    # encodes as kNone (ADVICE.md's open finding).  The row keeps the parent's answer; the fix changes
    # behaviour and is its own change.
    assert any(r["total"] == 1 << 27 and r["option"] == 16 and r["budget"] == 64 << 30 and r["slots"] == 32 and
               r["shift"] == 27 for r in rows)


def test_no_plan_is_one_the_launchers_would_refuse(exe):
    lim = load_rows()[0]["limits"]
    r = subprocess.run([exe, "sweep", str(lim["scene"]), str(lim["block"])], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    head = dict(kv.split("=") for kv in r.stdout.splitlines()[-1].split())
    assert int(head["plans"]) > 10 ** 6 and int(head["violations"]) == 0
