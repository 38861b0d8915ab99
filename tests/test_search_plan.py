"""The search launch plan (libbicos_amd/csrc/search_plan.cpp) against tests/golden/search_plan.json.

tests/cpp/plan_dump links the host-only planning source alone and prints, for the table of
shapes in tests/cpp/plan_cases.hpp, every launch the search would issue: kernel family,
variant fields, grid, block, dynamic LDS and the patched chunk / tiles_per_row / tail fields.
The golden file was recorded from the launch ladders the plan replaced (their launchers made
to print their template arguments and launch shape in place of launching, on the same table),
so the plan must keep choosing what they chose. No GPU is involved.

search_plan.json: "launches" holds every distinct launch line (plan_dump.cpp has the format),
"plans" one entry per case in the table's order: the indices of its launches, -1 for
hipErrorInvalidValue, -2 where search_mx_agree_fusable says no and no fused launch is asked.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "plan_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_plan.json")


@pytest.fixture(scope="module")
def plan_dump():
    subprocess.run(["make", "-C", os.path.dirname(EXE), "plan_dump"], check=True, capture_output=True)
    return EXE


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        db = json.load(f)
    assert db["cases"] == len(db["plans"]) > 6000
    return db


def recorded(db, i):
    p = db["plans"][i]
    if isinstance(p, int):
        return {-1: "invalid", -2: "unfusable"}[p]
    return " ".join(db["launches"][k] + ";" for k in p)


def test_plan_matches_the_recorded_launches(plan_dump, golden):
    env = {k: v for k, v in os.environ.items() if k not in ("BICOS_PK128", "BICOS_LR_T")}
    got = subprocess.run([plan_dump], capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    assert len(got) == golden["cases"]
    bad = [(g, recorded(golden, i)) for i, g in enumerate(got)
           if g.split(":", 1)[1].strip() != recorded(golden, i)]
    assert not bad, "%d of %d cases differ, first: %s\n recorded: %s" % (
        len(bad), len(got), bad[0][0], bad[0][1])


def test_table_reaches_every_family_and_switch(golden):
    """the recorded table exercises what it is meant to: all three families, tails, compacted
    launches, the fused agree, streamed and pruned variants, lazy drops, invalid requests"""
    launches = [l.split() for l in golden["launches"]]
    assert {l[0] for l in launches} == {"mx", "pk", "lr"}
    # family words ksteps nodupes T keys tail list agree stream prune lazy
    for field in range(6, 12):
        assert {l[field] for l in launches} == {"0", "1"}, field
    assert {l[5] for l in launches if l[0] == "mx"} == {"0", "1", "2", "3"}
    assert -1 in golden["plans"] and -2 in golden["plans"]
    assert sum(len(p) == 2 for p in golden["plans"] if isinstance(p, list)) > 100  # main + tail


def test_fused_launch_rejects_a_width_that_is_no_fused_shape(plan_dump):
    """launch_search_mx_agree takes the descriptor width from its caller: a (words, n) pair
    outside the table of fused shapes is hipErrorInvalidValue, whatever the geometry says"""
    r = subprocess.run([plan_dump, "mismatch"], capture_output=True, text=True)
    lines = dict(l.split(": ") for l in r.stdout.splitlines())
    assert len(lines) == 8
    for key, verdict in lines.items():
        fused = key in ("words 1 n 8", "words 4 n 33")
        assert verdict == ("planned" if fused else "invalid"), key
    assert r.returncode == 0
