"""Two iterations per marching launch (wdpm_dispatch.h::plan_iter2, wdpm_march.hip::iter2_march): the planner offers it on the right
side of every condition, leaves plan_iteration() alone, and - forced onto small rasters with WDPM_ITER2=2 in child processes (the
switches are read once per process) - the launches are bit for bit the oracle's, group edges, raster edges, short last groups, every
row count mod 3 and every block length included.  The launch ledger says which launches ran two iterations.

The case where a bounded wait between waves gives up is not provoked on the GPU (it would be a deliberate fault on a shared card):
the kernel's wait loops and the host's check of the error word (wdpm_capi.hip::wdpm_iter2_verdict) are reviewed by reading."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LEDGER_ITER2, LEDGER_BALANCE = 16, 8

# one group stores 680 padded columns when it is the raster's first (kGroupIn - kGroupHaloR), 663 otherwise; a strip 171
BLOCKS = [("block", 2), ("block", 3), ("block", 4), ("block", 5)]
CASES = {
    # exactly one group; rows = 0 mod 3
    "one-group": dict(module="add", shape=(300, 678), level="codes16", tiles=0, script=BLOCKS + [("iter", 3), ("block", 20), ("block", 21)]),
    # one group and a half; rows = 1 mod 3; NODATA blocks and dry regions
    "group-and-a-half": dict(module="add", shape=(301, 1010), level="codes32", tiles=0, patches=True, script=BLOCKS + [("block", 21)]),
    # two groups and one strip; rows = 2 mod 3; the DEM as 16-bit offsets; subtract
    "two-groups-one-strip": dict(module="subtract", shape=(302, 1512), level="codes16", tiles=0, script=BLOCKS + [("block", 20)]),
    # the last strip stores one column (group 1, strip 1 begins at padded column 834 and stores from 842, the border)
    "one-column-last-strip": dict(module="add", shape=(120, 841), level="codes32", tiles=0, patches=True, script=BLOCKS),
    # depths above 3 m in places: steps of the unclamped neighbour step beside clamped ones
    "deep-water": dict(module="add", shape=(200, 1400), level="codes16", tiles=0, deep=True, script=[("block", 5), ("block", 4)]),
    # tall chunks: the ring wraps many times, producers wait for consumers
    "tall-chunks": dict(module="add", shape=(3000, 700), level="codes16", tiles=0, patches=True, script=[("block", 4), ("iter", 2)]),
}
for k in range(1, 6):       # wdpm_iterate(k) on fresh water: k = 1 is a single launch, 3 and 5 leave an odd one over
    CASES[f"iterate-{k}"] = dict(module="add", shape=(150, 900), level="codes32", tiles=0, script=[("iter", k), ("max_diff",), ("iter", k)])
FORCED = dict(WDPM_RELAY="0", WDPM_TRI="0", WDPM_ITER2="2")
PLAIN_KERNELS = ("fused_iteration_kernel<0, false, 1, false, false, true>", "fused_iteration_kernel<0, false, 2, false, false, true>")


def taint(rows, cols, k, bad):
    """tests/test_rowblock.py::taint: cell-level worst-case dependency simulation of k iterations in the reference's pass order"""
    nb = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    t = bad.copy()
    for _ in range(k):
        for oi in (1, 2, 3):
            for oj in (1, 2, 3):
                R, C = np.meshgrid(np.arange(oi, rows - 1, 3), np.arange(oj, cols - 1, 3), indexing="ij")
                acc = t[R, C].copy()
                for di, dj in nb:
                    tn = t[R + di, C + dj]
                    t[R + di, C + dj] = tn | acc
                    acc = acc | tn
                t[R, C] = acc
    return t


def test_group_halo_is_the_dependency_reach_of_two_iterations():
    """a group of 705 columns that begins on a block edge: after two iterations all but 17 columns on the left and 24 on the right
    are exact (wdpm_dispatch.h: kGroupHaloL = 17, kGroupHaloR = 25, so that the group pitch 663 is a multiple of 3)"""
    n, c0 = 1000, 99
    c1 = c0 + 704
    bad = np.zeros((300, n), bool)
    bad[:, :c0] = True
    bad[:, c1 + 1:] = True
    clean = np.nonzero(~taint(300, n, 2, bad)[100:-100].any(axis=0))[0]
    assert clean.min() - c0 == 17 and c1 - clean.max() == 24
    assert 705 - 17 - 25 == 663 and 663 % 3 == 0


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_plans") / "pair_plans")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(HERE, "pair_plans_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {d["case"]: d for d in map(json.loads, out.strip().splitlines())}


def test_plan_iter2_offers_and_refuses_on_the_right_side_of_every_condition(plans):
    assert len(plans) >= 25
    for name, p in plans.items():
        offered = name.startswith(("offered", "forced-4096", "ring-")) or name == "forced-small"
        assert p["iter2"] == int(offered), (name, p)
        # a refusal hands back plan_iteration()'s plan, field for field
        assert p["single_untouched"], name
        assert bool(p["ledger_sw"] & LEDGER_ITER2) == offered, (name, p)


def test_plan_iter2_geometry_at_16384(plans):
    p = plans["offered"]
    # 25 groups of 663 columns cover 16386 padded columns; one workgroup per CU in one round; chunks twice the single launch's
    assert p["groups"] == 25 and p["block"] == 512 and p["grid"] % 8 == 0 and p["grid"] <= 256
    assert p["groups"] * p["nchunks"] <= p["grid"]
    assert p["H"] % 3 == 0 and p["H"] * p["nchunks"] >= 16384
    # the ring and its dump row beside the static staging: within the CU's LDS, and more than half of it (one workgroup per CU)
    static = 8 * 3 * 192 * 8 + 256
    assert p["ring_rows"] == 18 and p["lds"] >= (p["ring_rows"] + 1) * 712 * 8
    assert 163840 // 2 < p["lds"] + static <= 163840
    assert plans["ring-12"]["ring_rows"] == 12 and 163840 // 2 < plans["ring-12"]["lds"] + static
    assert p["table"] and p["ipx"] == p["grid"] // 8


def run_children(jobs, timeout=400):
    out = {}
    for label, (env, names) in jobs.items():       # one after the other
        p = subprocess.run([sys.executable, os.path.join(HERE, "pair_worker.py"), *names], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0, f"{label} {env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        out[label] = json.loads(p.stdout.strip().splitlines()[-1])
        missing = [n for n in names if n not in out[label]]
        assert not missing, f"{label}: no result for {missing}\n{p.stderr[-3000:]}"
    return out


def iter2_launches(result):
    """(launches of the gate-free code-streaming instantiations that ran two iterations, those that ran one)"""
    two = one = 0
    for name in PLAIN_KERNELS:
        for bits, n in result["switches"].get(name, {}).items():
            if int(bits) & LEDGER_ITER2:
                two += n
            else:
                one += n
    return two, one


def expected_launches(script):
    """(two-iteration launches, single gate-free launches) of a call script on water that stays plain"""
    two = one = 0
    for op in script:
        steady = op[1] - 2 if op[0] == "block" else op[1] if op[0] == "iter" else 0      # a block's first launch flushes, its last folds the max diff
        two += max(steady, 0) // 2
        one += max(steady, 0) % 2
    return two, one


@pytest.mark.gpu
def test_forced_two_iteration_launches_match_the_oracle(hip):
    names = list(CASES)
    res = run_children({"forced": (FORCED, names),
                        "forced, skewed chunk weights": (dict(FORCED, WDPM_BALANCE="2"), ["group-and-a-half", "two-groups-one-strip", "tall-chunks"]),
                        "forced, a ring of two row triples": (dict(FORCED, WDPM_ITER2_RING="6"), ["tall-chunks", "one-group"]),
                        "off": (dict(FORCED, WDPM_ITER2="0"), ["one-group", "iterate-4"])})
    failures = []
    for label, results in res.items():
        for case, r in results.items():
            if not r["ok"]:
                failures.append(f"{case} [{label}]: {r['error']}")
                continue
            two, one = iter2_launches(r)
            want_two, want_one = expected_launches(CASES[case]["script"])
            print(f"{case} [{label}]: {two} two-iteration launches, {one} single")
            if label == "off":
                if two != 0 or one != 2 * want_two + want_one:
                    failures.append(f"{case} [{label}]: WDPM_ITER2=0 launched {two} two-iteration launches, {one} single ones")
            elif "skewed" in label and not any(int(b) & LEDGER_ITER2 and int(b) & LEDGER_BALANCE for k in PLAIN_KERNELS for b in r["switches"].get(k, {})):
                failures.append(f"{case} [{label}]: no two-iteration launch took its chunk heights from the balance table")
            elif (two, one) != (want_two, want_one):
                failures.append(f"{case} [{label}]: {two} two-iteration and {one} single launches, expected {want_two} and {want_one}")
    assert not failures, "\n".join(failures)
