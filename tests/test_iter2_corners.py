"""The two-iteration marching launch (wdpm_march.hip::iter2_march, offered by wdpm_dispatch.h::plan_iter2) at the operands, steps and
shapes the other suites never gave it - and, where a part says "both loops", the single marching loop beside it (WDPM_ITER2=0):

  A  operand corners: elevations and depths from the pools of test_hip_parity.py::test_adversarial_operands (subnormal depths, depths
     of 10^6 and 10^280, ties of water surfaces, neighbours one quantum apart, water that exactly fills the step to its neighbour), on
     one, two and three groups, 32-bit codes and 16-bit offsets, add and subtract; subnormal depths through a block of 30 at threshold 0
  B  the unclamped neighbour step on DEM codes (`deep` = 8 on every step, the ledger state ITER2 | NO_CLAMP): by WDPM_CLAMP=0, and by
     data - elevations around 1.2e9 m, which the codes take (k0 absorbs them) and the 2^30 m bound of the clamped step does not
  C  every height from 1 to 45 rows on one and two groups; from 7 rows on also with chunk heights from skewed weights and a ring of six
  D  every width around the edges the group geometry makes: 1 - 12 columns, the first strip's end, the first group's end, the end of
     group 1's first strip, the second group's end
  E  degenerate shapes, 1 x 2000 and 2000 x 1 included

Parts C, D and E run on coverage_worker's gentle raster without its NODATA frame (live_edge_case): the first and last rows and columns a
launch stores hold terrain and water.  Every case runs in a child process (tests/iter2_corners_worker.py; the switches are read once per process) through
coverage_worker.run_case: guard bands, every observation, the raster and totaldrain bit for bit against the CPU oracle.  A case passes
only with the launches the planner promises: tests/pair_plans_main.cpp plans each case's launch on the CPU (the `corner_plans` fixture;
test_the_planner_offers_every_case holds that without a GPU), and the ledger must show that many two-iteration and single launches of
the gate-free instantiation on the case's codes, with the plan's ledger bits - so a silent fall-back to single launches, to the gated
kernels or to the other codes fails the case.

On an MI355X each GPU test here takes 0.7 - 1.6 s, the file 13 s (profiles/r23/README.md, which also says which cases caught the
mutants of iter2_march the file was tried against).  Only part A can tell the clamped neighbour step from the exact one - it takes a
depth above 8 m - so the depths of 1e6 and 1e280 there are what holds `deep` in the two-iteration loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_dem16_bases import KERNEL16, KERNEL32  # noqa: E402
from test_iter2_retired_strips import K, consumer_stores, groups  # noqa: E402
from test_pair_iterations import CASES as PAIR_CASES, FORCED, LEDGER_BALANCE, LEDGER_ITER2, expected_launches  # noqa: E402

MISS = -99999.0
LEDGER_NO_CLAMP = 1
BASE = {k: v for k, v in FORCED.items() if k != "WDPM_ITER2"}           # WDPM_RELAY=0 WDPM_TRI=0
LOOPS = {"two-iteration": "2", "single": "0"}

# ------------------------------------------------------------------------------------------------ rasters

# test_adversarial_operands' pool of decimal elevations (seed == 4): the 32-bit check passes on the 1e-4 grid
DPOOL32 = np.array([1e-4, 0.5, 1.0, 499.9999, 500.0, 500.0001, 500.1, 512.0, 99999.9999])
# for the 16-bit offsets: within 6.5 m of each other around 500 m (65 000 quanta of 1e-4), exact ties, neighbours one quantum apart
DPOOL16 = np.array([497.0, 499.9998, 499.9999, 500.0, 500.0, 500.0001, 500.0002, 500.1, 500.8, 503.5])
# test_adversarial_operands' depths, 1e300 replaced by 1e280: scan_water_kernel calls anything above 1e290 "not plain"
WPOOL = np.array([0.0, 0.0, 0.0, 5e-324, 1e-310, 2.3e-308, 1e-300, 1e-16, 1.1368683772161603e-13, 1e-4, 1e-4, 0.1, 0.1,
                  np.nextafter(0.1, 1), 0.7999999999999, 0.8, 1.0, 8.0, 1e6, 1e280])


def operand_case(R, C, seed, pool, subnormal=False):
    """test_adversarial_operands' raster from the given pool of elevations; subnormal: test_subnormal_depths_are_not_flushed's water"""
    rng = np.random.default_rng(100 + seed)
    dpool = DPOOL16 if pool == 16 else DPOOL32
    dem = dpool[rng.integers(0, len(dpool), (R, C))]
    water = WPOOL[rng.integers(0, len(WPOOL), (R, C))]
    # runs of equal elevations / equal surfaces along rows so that ties and one-quantum differences meet as neighbours
    same = rng.random((R, C)) < 0.4
    for arr in (dem, water):
        arr[:, 1:] = np.where(same[:, 1:], arr[:, :-1], arr[:, 1:])
    fill = rng.random((R, C)) < 0.1                           # depth that brings the surface exactly to the left neighbour's
    water[:, 1:] = np.where(fill[:, 1:] & (dem[:, :-1] > dem[:, 1:]), dem[:, :-1] - dem[:, 1:], water[:, 1:])
    if subnormal:
        water = np.where(rng.random((R, C)) < 0.2, 0.0, 0.3 * rng.random((R, C))) * 1e-308      # 0 .. 3e-309
        water[::7, ::5] = 5e-324
    dem[rng.random((R, C)) < 0.05] = MISS
    water[dem <= MISS] = 0.0
    return dem, water


def far_dem_case(R, C, seed, grid_exp, deep):
    """elevations around 1.2e9 m on the 10^-grid_exp grid: encodable (k0 absorbs the offset), beyond the clamped step's 2^30 m"""
    rng = np.random.default_rng(500 + seed)
    y, x = np.mgrid[0:R, 0:C]
    scale = 10 ** grid_exp
    k = np.rint(scale * (3.0 + 2.0 * np.sin(x / 5.1) * np.cos(y / 3.3))).astype(np.int64) + rng.integers(0, 3, (R, C))
    dem = (1_200_000_000 * scale + k) / float(scale)
    dem[rng.random((R, C)) < 0.03] = MISS
    water = np.where((dem > MISS) & (rng.random((R, C)) >= 0.25), 0.3 * rng.random((R, C)), 0.0)
    if deep:
        sel = (rng.random((R, C)) < 0.02) & (dem > MISS)
        water[sel] = 3.0 + 4.0 * rng.random((R, C))[sel]
    return dem, water


def live_edge_case(make_case, R, C, seed):
    """coverage_worker.make_case's gentle raster (`make_case`) without its frame: that maker sets the raster's own first and last rows
    and columns to NODATA, so the last rows and columns a launch stores would hold +0.0 whatever the kernel did.  Here they hold
    terrain and water (the interior of a raster two cells larger each way), and the only wall is the padded border."""
    dem, water = make_case(R + 2, C + 2, seed)
    return np.ascontiguousarray(dem[1:-1, 1:-1]), np.ascontiguousarray(water[1:-1, 1:-1])


# ------------------------------------------------------------------------------------------------ cases

CASES = {}
SHAPES_A = [(40, 200), (41, 700), (30, 1345)]                           # one, two and three groups
SCRIPT_A = [("iter", 2), ("iter", 4), ("block", 6), ("block", 5, 0.0)]
for _R, _C in SHAPES_A:
    for _seed in (1, 2, 3, 4):
        for _pool in (32, 16):
            for _module in ("add", "subtract"):
                CASES[f"A-{_module}-pool{_pool}-{_R}x{_C}-s{_seed}"] = dict(
                    module=_module, shape=(_R, _C), seed=_seed, level=f"codes{_pool}", tiles=0, raster="operands", pool=_pool, script=SCRIPT_A)
    CASES[f"A-subnormal-{_R}x{_C}"] = dict(module="add", shape=(_R, _C), seed=1, level="codes16", tiles=0, raster="operands", pool=16,
                                           subnormal=True, script=[("block", 30, 0.0)])
PART_A = [n for n in CASES if n.startswith("A-")]

# B 1: WDPM_CLAMP=0 on part A's first seed and on test_pair_iterations' deep water
PART_B_SWITCH = [n for n in PART_A if n.endswith("-s1")] + ["B-deep-water"]
CASES["B-deep-water"] = dict(PAIR_CASES["deep-water"])
# B 2: by data
for _exp, _level, (_R, _C) in ((0, "codes16", (40, 200)), (0, "codes16", (41, 700)), (1, "codes32", (40, 200)), (1, "codes32", (41, 700))):
    for _deep in (False, True):
        CASES[f"B-far-1e-{_exp}-{'deep' if _deep else 'shallow'}-{_R}x{_C}"] = dict(
            module="add", shape=(_R, _C), seed=7, level=_level, tiles=0, raster="far", grid_exp=_exp, deep_cells=_deep,
            script=[("iter", 2), ("iter", 5), ("block", 6)])
PART_B_DATA = [n for n in CASES if n.startswith("B-far")]

# C: every height
SCRIPT_C = [("iter", 2), ("block", 5)]
for _C in (200, 700):
    for _R in range(1, 46):
        CASES[f"C-{_R}x{_C}"] = dict(module="add", shape=(_R, _C), level="codes16", tiles=0, raster="live-edges", script=SCRIPT_C)
PART_C = {c: [f"C-{r}x{c}" for r in range(1, 46)] for c in (200, 700)}
PART_C_TALL = [f"C-{r}x200" for r in range(7, 46)]                      # two chunks at least: the balance table, the short ring


# D: every width around the edges of the group geometry (test_iter2_retired_strips.py: the constants of wdpm_dispatch.h)
def edge_widths():
    """unpadded widths, by what they are near"""
    far = 10 ** 6
    first_strip_end = consumer_stores(far, 0, 0)[1] + 1                 # padded width that strip 0 of group 0 stores to its last column
    first_group_end = consumer_stores(far, 0, 3)[1] + 1                 # ... group 0: one more and group 1 stores exactly one column
    one_column_strip = consumer_stores(far, 1, 1)[0] + 1                # padded width at which strip 1 of group 1 stores one column
    second_group_end = consumer_stores(far, 1, 3)[1] + 1
    return {"narrow": list(range(1, 13)),
            "first-strip-end": [w - 2 for w in range(first_strip_end - 6, first_strip_end + 7)],
            "first-group-end": [w - 2 for w in range(first_group_end - 8, first_group_end + 9)],
            "group-1-first-strip-end": [w - 2 for w in range(one_column_strip - 6, one_column_strip + 7)],
            "second-group-end": [w - 2 for w in range(second_group_end - 8, second_group_end + 7)]}


WIDTHS_D = sorted({w for ws in edge_widths().values() for w in ws})
SCRIPT_D = [("iter", 2), ("block", 4)]
PART_D = {7: [], 26: []}
for _R in PART_D:
    for _i, _w in enumerate(WIDTHS_D):
        CASES[f"D-add-{_R}x{_w}"] = dict(module="add", shape=(_R, _w), level="codes32", tiles=0, raster="live-edges", script=SCRIPT_D)
        PART_D[_R].append(f"D-add-{_R}x{_w}")
        if _i % 3 == 0:
            CASES[f"D-subtract-{_R}x{_w}"] = dict(module="subtract", shape=(_R, _w), level="codes16", tiles=0, raster="live-edges", script=SCRIPT_D)
            PART_D[_R].append(f"D-subtract-{_R}x{_w}")

# E: test_hip_parity.py::test_degenerate_shapes' and two more
SHAPES_E = [(1, 1), (1, 700), (2, 3), (600, 1), (3, 171), (4, 172), (23, 178), (24, 179), (1, 2000), (2000, 1)]
for _R, _C in SHAPES_E:
    CASES[f"E-{_R}x{_C}"] = dict(module="add", shape=(_R, _C), level="codes16", tiles=0, raster="live-edges", script=[("iter", 2), ("iter", 5)])
PART_E = [f"E-{r}x{c}" for r, c in SHAPES_E]

# (label, environment beyond BASE and WDPM_ITER2, cases); each is one child per loop it runs under
CHILDREN = {
    "A": ({}, PART_A, tuple(LOOPS)),
    "B-switch": (dict(WDPM_CLAMP="0"), PART_B_SWITCH, tuple(LOOPS)),
    "B-data": ({}, PART_B_DATA, tuple(LOOPS)),
    "C-200": ({}, PART_C[200], ("two-iteration",)),
    "C-700": ({}, PART_C[700], ("two-iteration",)),
    "C-balance": (dict(WDPM_BALANCE="2"), PART_C_TALL, ("two-iteration",)),
    "C-ring": (dict(WDPM_ITER2_RING="6"), PART_C_TALL, ("two-iteration",)),
    "D-7": ({}, PART_D[7], ("two-iteration",)),
    "D-26": ({}, PART_D[26], ("two-iteration",)),
    "E": ({}, PART_E, ("two-iteration",)),
}


def unclamped(child, case):
    """must every launch of the case run the unclamped step?"""
    return child == "B-switch" or CASES[case].get("raster") == "far"


# ------------------------------------------------------------------------------------------------ the planner's word (CPU)

def plan_key(child, case):
    return f"{child}/{case}"


@pytest.fixture(scope="module")
def corner_plans(tmp_path_factory):
    """what plan_iter2 / plan_iteration decide for the steady launches of every case of every child, from tests/pair_plans_main.cpp"""
    exe = str(tmp_path_factory.mktemp("corner_plans") / "pair_plans")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(HERE, "pair_plans_main.cpp"), "-o", exe])
    args = []
    for child, (env, names, _) in CHILDREN.items():
        for n in names:
            R, C = CASES[n]["shape"]
            args.append(f"{plan_key(child, n)}:{R}:{C}:{int(CASES[n]['level'] == 'codes16')}:{env.get('WDPM_BALANCE', '1')}:"
                        f"{env.get('WDPM_ITER2_RING', '0')}:{int(not unclamped(child, n))}")
    plans = {}
    for k in range(0, len(args), 200):
        out = subprocess.run([exe, *args[k:k + 200]], capture_output=True, text=True, check=True).stdout
        plans.update({d["case"]: d for d in map(json.loads, out.strip().splitlines())})
    assert len(plans) == len(args)
    return plans


def test_the_lists_are_the_issues():
    assert len(PART_A) == 3 * 4 * 2 * 2 + 3 and len(PART_C[200]) == len(PART_C[700]) == 45 and len(PART_C_TALL) == 39
    assert [groups(c + 2) for _, c in SHAPES_A] == [1, 2, 3]
    w = edge_widths()
    assert w["first-strip-end"][6] + 2 == 179 and w["first-group-end"][8] + 2 == 680 and w["group-1-first-strip-end"][6] == 841
    assert w["second-group-end"][8] + 2 == 1343 and len(WIDTHS_D) == 12 + 13 + 17 + 13 + 15
    # the widths at which a strip or a group stores exactly one column, and none, are among them
    for grp, j in ((0, 1), (1, 0), (1, 1)):
        first = consumer_stores(10 ** 6, grp, j)[0]
        assert consumer_stores(first + 1, grp, j) == (first, first) and consumer_stores(first, grp, j) is None
        assert first - 1 in WIDTHS_D and first - 2 in WIDTHS_D
    assert groups(K["GroupIn"] - K["GroupHaloR"]) == 1 and groups(K["GroupIn"] - K["GroupHaloR"] + 1) == 2
    assert {groups(c + 2) for c in WIDTHS_D} == {1, 2, 3}


def test_the_rasters_are_what_the_cases_say():
    for pool in (32, 16):
        dem, water = operand_case(41, 700, 2, pool)
        valid = dem > MISS
        assert 0.03 < (~valid).mean() < 0.07 and (water[~valid] == 0).all()
        # plain water: nothing negative, no -0.0, nothing above 1e290 - or the gate-free kernels would not run
        assert (water >= 0).all() and not np.signbit(water).any() and water.max() < 1e290
        assert ((water > 0) & (water < 2.2e-308)).any() and (water >= 1e6).any() and (water == 1e280).any()
        q = np.rint(dem * 1e4).astype(np.int64)
        both = valid[:, 1:] & valid[:, :-1]
        assert (both & (q[:, 1:] == q[:, :-1])).any() and (both & (np.abs(q[:, 1:] - q[:, :-1]) == 1)).any()
        surface = dem + water
        assert (both & (water[:, 1:] > 0) & (surface[:, 1:] == dem[:, :-1]) & (dem[:, :-1] > dem[:, 1:])).any()      # fills the step exactly
        assert (both & (surface[:, 1:] == surface[:, :-1]) & (water[:, 1:] > 0)).any()                                # ties of surfaces
        if pool == 16:
            assert q[valid].max() - q[valid].min() <= 65000
    dem, water = operand_case(40, 200, 1, 16, subnormal=True)
    assert water.max() < 3.1e-309 and (water == 5e-324).any()
    import coverage_worker as cw
    for R, C in ((7, 178), (26, 841), (1, 2000), (2000, 1)):          # parts C, D, E: live cells with water on the raster's own edges
        dem, water = live_edge_case(cw.make_case, R, C, R * 7 + C)
        assert dem.shape == water.shape == (R, C)
        for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
            assert (dem[edge] > MISS).mean() > 0.8 and (water[edge] > 0).any()
    for exp in (0, 1):
        dem, water = far_dem_case(41, 700, 7, exp, True)
        v = dem[dem > MISS]
        assert v.min() >= 2.0 ** 30 and (np.rint(v * 10 ** exp) / 10 ** exp == v).all() and np.ptp(np.rint(v * 10 ** exp)) < 65535
        assert exp == 0 or (np.rint(v) != v).any()
        assert 3.0 < water.max() < 7.0


def test_the_planner_offers_every_case(corner_plans):
    """plan_iter2, forced, offers a two-iteration launch of the gate-free instantiation on the case's codes for every shape of every
    child - 1 x 1, 1 x 2000 and 2000 x 1 included; nothing is refused, so nothing is dropped from the GPU lists - and the single
    launches beside them (an odd one left over, WDPM_ITER2=0) are the marching kernel's gate-free ones on the same codes"""
    for child, (env, names, _) in CHILDREN.items():
        for n in names:
            p = corner_plans[plan_key(child, n)]
            codes = 2 if CASES[n]["level"] == "codes16" else 1
            assert p["iter2"] == 1 and p["codes"] == codes and p["block"] == 512, (child, n, p)
            assert p["single_marching"] and p["single_codes"] == codes, (child, n, p)
            assert p["ledger_sw"] & LEDGER_ITER2 and not p["single_ledger_sw"] & LEDGER_ITER2
            assert bool(p["ledger_sw"] & LEDGER_NO_CLAMP) == bool(p["single_ledger_sw"] & LEDGER_NO_CLAMP) == unclamped(child, n), (child, n, p)
            R, C = CASES[n]["shape"]
            assert p["groups"] == groups(C + 2) and p["H"] % 3 == 0 and p["H"] >= 6 and p["H"] * p["nchunks"] >= R, (child, n, p)
            assert p["ring_rows"] == (6 if child == "C-ring" else 18)
            assert bool(p["ledger_sw"] & LEDGER_BALANCE) == p["table"]
            if child == "C-balance":
                assert p["table"] and p["nchunks"] >= 2, (n, p)          # from 7 rows on every launch takes the table
            elif R < 7:
                assert p["nchunks"] == 1 and not p["table"]
    # the smallest rasters: one workgroup, one chunk of six rows, H raised from 3
    p = corner_plans[plan_key("E", "E-1x1")]
    assert (p["groups"], p["nchunks"], p["H"], p["grid"]) == (1, 1, 6, 8)
    assert corner_plans[plan_key("E", "E-2000x1")]["nchunks"] > 200 and corner_plans[plan_key("E", "E-1x2000")]["groups"] == 3


# ------------------------------------------------------------------------------------------------ GPU

def run_child(env, names, timeout):
    p = subprocess.run([sys.executable, os.path.join(HERE, "iter2_corners_worker.py"), *names], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"{env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    res = json.loads(p.stdout.strip().splitlines()[-1])
    missing = [n for n in names if n not in res]
    assert not missing, f"no result for {missing[:5]} ...\n{p.stderr[-3000:]}"
    return res


def judge(child, loop, results, plans):
    """the failures of one child: a case that did not match the oracle, or whose launches are not the planner's"""
    failures = []
    for case, r in results.items():
        if not r["ok"]:
            failures.append(f"{case} [{child}, {loop}]: {r['error']}")
            continue
        spec, plan = CASES[case], plans[plan_key(child, case)]
        kernel, other = (KERNEL16, KERNEL32) if spec["level"] == "codes16" else (KERNEL32, KERNEL16)
        want_two, want_one = expected_launches(spec["script"])
        if loop == "single":
            want_two, want_one = 0, 2 * want_two + want_one
        states = {int(b): n for b, n in r["switches"].get(kernel, {}).items()}
        two = sum(n for b, n in states.items() if b & LEDGER_ITER2)
        one = sum(n for b, n in states.items() if not b & LEDGER_ITER2)
        if (two, one) != (want_two, want_one) or other in r["switches"]:
            failures.append(f"{case} [{child}, {loop}]: {two} two-iteration and {one} single launches of {kernel}, expected {want_two} and {want_one}"
                            f"{' - and launches on the other codes' if other in r['switches'] else ''}")
        # the two-iteration launches in exactly the planner's ledger state (NO_CLAMP, BALANCE, PRIO, ITER2); the single ones clamped or not as planned
        wrong = [b for b in states if (b != plan["ledger_sw"] if b & LEDGER_ITER2 else (b ^ plan["single_ledger_sw"]) & LEDGER_NO_CLAMP)]
        if wrong:
            failures.append(f"{case} [{child}, {loop}]: launches in ledger states {sorted(states)}, planned {plan['ledger_sw']} (two iterations) and "
                            f"{plan['single_ledger_sw']} (one)")
    return failures


def play_child(child, loop, plans, timeout=120):          # a child takes one to two seconds
    env, names, loops = CHILDREN[child]
    assert loop in loops
    res = run_child(dict(BASE, WDPM_ITER2=LOOPS[loop], **env), names, timeout)
    failures = judge(child, loop, res, plans)
    assert not failures, f"{len(failures)} of {len(names)} cases:\n" + "\n".join(failures[:40])


@pytest.mark.gpu
def test_degenerate_shapes_through_two_iteration_launches(hip, corner_plans):
    play_child("E", "two-iteration", corner_plans)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [7, 26])
def test_every_width_around_the_group_geometrys_edges(hip, corner_plans, rows):
    play_child(f"D-{rows}", "two-iteration", corner_plans)


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["C-200", "C-700", "C-balance", "C-ring"])
def test_every_height(hip, corner_plans, child):
    play_child(child, "two-iteration", corner_plans)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", list(LOOPS))
def test_operand_corners(hip, corner_plans, loop):
    play_child("A", loop, corner_plans)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", list(LOOPS))
def test_unclamped_step_on_codes_by_switch(hip, corner_plans, loop):
    play_child("B-switch", loop, corner_plans)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", list(LOOPS))
def test_unclamped_step_on_codes_by_data(hip, corner_plans, loop):
    play_child("B-data", loop, corner_plans)
