"""The planner of the routing sweep (wdpm_amd/csrc/wdpm_route_plan.h), a pure host function, through the stand-alone program
tests/route_plans_main.cpp: level sizes made up directly, and the properties of the returned plan - every level in exactly one
launch, in descending order; a wide level alone in a grid launch over exactly its ponds; runs of narrow levels no longer than the
cap; as many launches as the words of include/wdpm_pond_routing.h give (tests/pond_routing_model.plan_of)."""
import json
import os
import subprocess

import pytest

from conftest import ROOT
from pond_routing_model import BLOCK, RUN_LEVELS, plan_of


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("route_plans") / "route_plans")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "route_plans_main.cpp"), "-o", path])
    return path


def plan(exe, sizes, narrow=BLOCK, run_levels=RUN_LEVELS):
    """the plan of levels of `sizes` ponds, checked for what every plan must be; returns its launches"""
    words, i = [], 0
    while i < len(sizes):                                     # run-length encoded, for the long ones
        j = i
        while j < len(sizes) and sizes[j] == sizes[i]:
            j += 1
        words.append(f"{sizes[i]}x{j - i}")
        i = j
    p = json.loads(subprocess.check_output([exe, str(narrow), str(run_levels)] + words, text=True))
    assert p["levels"] == len(sizes)
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    covered = []
    for top, levels, wide, first, count in p["launches"]:
        assert levels >= 1
        if wide:
            assert levels == 1 and sizes[top] > narrow and (first, count) == (offsets[top], sizes[top])
        else:
            assert levels <= run_levels and all(sizes[top - j] <= narrow for j in range(levels))
        covered += [top - j for j in range(levels)]
    assert covered == list(range(len(sizes) - 1, -1, -1))     # every level once, the deepest first
    assert p["wide_levels"] == sum(s > narrow for s in sizes) == sum(l[2] for l in p["launches"])
    want = plan_of(sizes, narrow, run_levels)
    assert [("wide", l[0]) if l[2] else ("run", l[0], l[1]) for l in p["launches"]] == want
    return p["launches"]


def test_all_wide(exe):
    assert len(plan(exe, [1000, 257, 300, 70000])) == 4


def test_all_narrow(exe):
    assert plan(exe, [1, 256, 3, 255, 17]) == [[4, 5, 0, 0, 0]]


def test_alternating(exe):
    launches = plan(exe, [5, 300, 5, 300, 5, 300])
    assert [l[2] for l in launches] == [1, 0, 1, 0, 1, 0] and len(launches) == 6
    launches = plan(exe, [300, 5, 6, 300, 300, 7, 8, 9])
    assert [(l[0], l[1], l[2]) for l in launches] == [(7, 3, 0), (4, 1, 1), (3, 1, 1), (2, 2, 0), (0, 1, 1)]


def test_a_run_longer_than_the_cap(exe):
    launches = plan(exe, [1] * 65537)
    assert [(l[0], l[1]) for l in launches] == [(65536, 65536), (0, 1)]
    launches = plan(exe, [1] * 6667, run_levels=100)
    assert len(launches) == 67 and launches[-1][:2] == [66, 67] and all(l[1] == 100 for l in launches[:-1])
    assert len(plan(exe, [2] * 200 + [400] + [2] * 200, run_levels=100)) == 5
    assert len(plan(exe, [1] * 131072)) == 2 and len(plan(exe, [1] * 131073)) == 3


def test_one_level_and_no_level(exe):
    assert plan(exe, [1]) == [[0, 1, 0, 0, 0]] and plan(exe, [300]) == [[0, 1, 1, 0, 300]] and plan(exe, []) == []


def test_levels_of_exactly_one_workgroup_and_one_pond_more(exe):
    assert plan(exe, [256, 256]) == [[1, 2, 0, 0, 0]]
    assert plan(exe, [256, 257, 256]) == [[2, 1, 0, 0, 0], [1, 1, 1, 256, 257], [0, 1, 0, 0, 0]]
    assert [l[2] for l in plan(exe, [8, 9, 8], narrow=8)] == [0, 1, 0] and [l[2] for l in plan(exe, [1, 2], narrow=1)] == [1, 0]


def test_bounds_out_of_range_fall_back_to_the_defaults(exe):
    """a narrow bound above one workgroup would let a run skip ponds: the planner takes the default instead"""
    assert plan(exe, [300, 5], narrow=BLOCK) == json.loads(subprocess.check_output([exe, "1000", "0", "300", "5"], text=True))["launches"]
    bound = lambda *a: int(subprocess.check_output([exe, "bound"] + [str(v) for v in a], text=True))     # noqa: E731
    assert bound("8", 1, 256, 256) == 8 and bound("256", 1, 256, 256) == 256 and bound("1", 1, 256, 256) == 1
    assert bound("0", 1, 256, 256) == 256 and bound("257", 1, 256, 256) == 256 and bound("-", 1, 256, 256) == 256
    assert bound("", 1, 256, 256) == 256 and bound("x", 1, 256, 256) == 256 and bound("100", 1, 2 ** 31 - 1, 65536) == 100
