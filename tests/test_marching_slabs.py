"""Marching and two-iteration launches (wdpm_dispatch.h::plan_iter2, wdpm_march.hip::iter2_march) on SLABS: contexts with a live
first and / or last row, a max diff over a row range, and groups of k iterations that end in the three windows of
wdpm_iterate_overlapped - what every slab of a multi-GPU run is, forced onto small rasters in child processes with
WDPM_RELAY=0 WDPM_TRI=0 WDPM_ITER2=2 (the switches are read once per process; tests/slab_worker.py is the child).

The contract is the halo rule (include/wdpm.h, wdpm_amd.rowblock.halo_depth): T iterations after its upload a slab holds the whole
raster's bits from row 3T-1 where its top edge is live, up to row rows-1-(6T-2) where its bottom edge is live.

A. one HIP slab context against the oracle's whole raster after every op of a script, on exactly those rows, with the max diff of
   `block` and `overlap` ops announced and read over the same rows on both sides;
B. groups through the C driver (wdpm_group_*) against one oracle context: whole raster and every block's max diff;
C. (CPU) the Part A cases with an ORACLE slab: the row ranges are pinned by the reference alone, so that a wrong bound in this
   file cannot pass.  Zero cells differ inside the bound; where the top is live the row just above it, 3T-2, differs every time:
   the top bound is sharp.  The bottom bound is asserted only as the contract: on these rasters the nearest differing row lies 2
   rows beyond it after one iteration, 5 after two and some 30 after eight (a perturbation that climbs from the bottom edge decays
   below one ulp before it has gone as far as the dependency allows), which is why cases of a single ("iter", 2) are among them.

The launch ledger says which launches ran two iterations; the counts are asserted exactly for every Part A script and every group
(derived below from wdpm_iterate, wdpm_iterate_overlapped and wdpm_rowblock.c::rank_iterate), under WDPM_BALANCE=2 as "at least
one two-iteration launch took its chunk heights from the table".  The wait loops between producer and consumer waves are not
provoked (tests/test_pair_iterations.py says why)."""
import json
import os
import subprocess
import sys
import time

import pytest

from test_pair_iterations import FORCED, LEDGER_BALANCE, LEDGER_ITER2, PLAIN_KERNELS, expected_launches, iter2_launches

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def windows(n):
    """(rows a neighbour needs from the top, from the bottom) of a slab between two others at a refresh every n iterations:
    wdpm_rowblock.c::plan_exchange - its own halo and the neighbour's, (3n-1) + (6n-2) either way"""
    return 9 * n - 3, 9 * n - 3


# widths: 678 one group of four strips, 1010 a group and a half, 1512 two groups and a strip, 841 a one-column last strip, 761 three
# retired strips.  Every slab begins on a row = 0 mod 3; one with a live bottom is a multiple of 3 rows tall.
CASES = {
    # one two-iteration launch on fresh water: the bounds are sharpest here
    "one-launch-1010": dict(module="add", shape=(400, 1010), slab=(99, 156), level="codes32", script=[("iter", 2)]),
    "one-launch-678": dict(module="add", shape=(400, 678), slab=(201, 150), level="codes16", script=[("iter", 2)]),
    # both edges live: two two-iteration launches between flush and fold; an odd iteration left over
    "middle-1010": dict(module="add", shape=(400, 1010), slab=(99, 156), level="codes32", patches=True, script=[("block", 6)]),
    "middle-761": dict(module="add", shape=(400, 761), slab=(99, 201), level="codes16", script=[("block", 5), ("iter", 3)]),
    # the raster's first rows: live bottom only, T = 8; subtract
    "top-1512": dict(module="subtract", shape=(400, 1512), slab=(0, 150), level="codes16", script=[("block", 4), ("block", 4)]),
    # tall: the ring wraps, producers wait for consumers
    "tall-700": dict(module="add", shape=(3300, 700), slab=(99, 3000), level="codes16", patches=True, script=[("block", 4), ("iter", 2)]),
    # depths above 3 m in places: the unclamped neighbour step beside clamped ones
    "deep-1400": dict(module="add", shape=(400, 1400), slab=(99, 156), level="codes16", deep=True, script=[("block", 5)]),
}
for _R in (400, 401, 402):      # the raster's last rows: live top only, short last triples, every height mod 3
    CASES[f"bottom-841-{_R}"] = dict(module="add", shape=(_R, 841), slab=(252, _R + 2 - 252), level="codes32",
                                     script=[("block", 5), ("iter", 2)])
for _n in (3, 4, 7, 8):         # what rank_iterate does with a group of n: iterate(n-1) in pairs, then the three windows
    CASES[f"overlap-{_n}"] = dict(module="add", shape=(400, 1010), slab=(99, 201), level="codes32", script=[("overlap", _n, *windows(_n))])
    CASES[f"overlap-plain-{_n}"] = dict(module="add", shape=(400, 1010), slab=(99, 201), level="codes32",
                                        script=[("overlap_plain", _n, *windows(_n))])
OVERLAPS = [n for n in CASES if n.startswith("overlap")]

GROUP_CASES = {
    "group-1010": dict(module="add", shape=(420, 1010), ranks=2, k=8, blocks=[10, 9], level="codes32"),
    "group-678": dict(module="add", shape=(500, 678), ranks=3, k=3, blocks=[7, 8], level="codes16"),
    "group-1512": dict(module="subtract", shape=(420, 1512), ranks=2, k=4, blocks=[9, 6], level="codes16"),
    "group-841": dict(module="add", shape=(420, 841), ranks=2, k=5, blocks=[11], level="codes32"),
    # iterate(1) and the windows: nothing to pair
    "group-k2": dict(module="add", shape=(420, 1010), ranks=2, k=2, blocks=[7, 4], level="codes32"),
}

# the children, one after the other: (environment, cases)
CHILDREN = {
    "forced": (FORCED, [n for n in CASES if n not in OVERLAPS and n != "tall-700"]),
    "forced, tall": (FORCED, ["tall-700"]),
    "forced, overlapped": (FORCED, OVERLAPS),
    "skewed chunk weights": (dict(FORCED, WDPM_BALANCE="2"), ["middle-1010", "middle-761", "tall-700"]),
    "a ring of two row triples": (dict(FORCED, WDPM_ITER2_RING="6"), ["tall-700", "middle-1010"]),
    "producers without priority": (dict(FORCED, WDPM_ITER2_PRIO="0"), ["middle-761"]),
    "off": (dict(FORCED, WDPM_ITER2="0"), ["middle-1010", "bottom-841-401"]),
    "groups": (FORCED, list(GROUP_CASES)),
    "groups, no overlap": (dict(FORCED, WDPM_OVERLAP="0"), ["group-841"]),
}


def expected_slab_launches(script):
    """(two-iteration launches, single gate-free launches) of a Part A script.  `block` and `iter`: test_pair_iterations.py's count.
    wdpm_iterate_overlapped(n) on a slab between two others is wdpm_iterate(n-1) with nothing folded, then three windows, each
    a single launch.  Outside a block ("overlap_plain") nothing is flushed: (n-1)//2 pairs, (n-1)%2 single launches and three
    gate-free windows.  In a block ("overlap") the call's first launch carries the threshold flush and pairs with nothing, which
    leaves n-2 iterations to pair, and the windows fold the max diff: neither is a gate-free instantiation."""
    two, one = expected_launches(script)
    for op in script:
        if op[0] == "overlap_plain":
            two, one = two + (op[1] - 1) // 2, one + (op[1] - 1) % 2 + 3
        elif op[0] == "overlap":
            two, one = two + max(op[1] - 2, 0) // 2, one + max(op[1] - 2, 0) % 2
    return two, one


def expected_group_launches(spec, overlap=True):
    """(two-iteration launches, single gate-free launches) of a group's blocks, summed over its ranks: wdpm_rowblock.c::rank_iterate.
    Every block begins on refreshed halos (wdpm_rank_max_diff), so a block of nb iterations is steps of k and a last shorter one.
    With the overlap on every step ends a group of k or the block, so every step is wdpm_iterate_overlapped(s): wdpm_iterate(s-1)
    with nothing folded - the block's first launch carries the flush and pairs with nothing - and the windows (two on the first and
    the last rank, three between), gate-free single launches unless they fold the block's max diff or carry its flush.
    WDPM_OVERLAP=0: every step is wdpm_iterate(s); the block's first launch flushes, its last folds, what lies between pairs."""
    n, k = spec["ranks"], spec["k"]
    two = one = 0
    for rank in range(n):
        nwin = 2 if rank in (0, n - 1) else 3
        for nb in spec["blocks"]:
            done = 0
            while done < nb:
                s = min(k, nb - done)
                first, last = done == 0, done + s == nb
                if overlap:
                    steady = s - 1 - (1 if first and s > 1 else 0)
                    if not last and not (first and s == 1):
                        one += nwin
                else:
                    steady = max(s - (1 if first else 0) - (1 if last else 0), 0)
                two, one = two + steady // 2, one + steady % 2
                done += s
    return two, one


def test_expected_launch_counts_of_the_driver():
    """the derivation above on the cases' own numbers: ten iterations at k = 8 are overlapped(8) = flush + 3 pairs + windows, then
    overlapped(2) = one single launch + folding windows, on both ranks; nine are overlapped(8), overlapped(1)"""
    assert expected_group_launches(GROUP_CASES["group-1010"]) == (2 * (3 + 3), 2 * (2 + 1 + 2))
    assert expected_group_launches(GROUP_CASES["group-k2"])[0] == 0
    assert expected_group_launches(GROUP_CASES["group-841"], overlap=False) == (2 * (2 + 2 + 0), 2 * (0 + 1 + 0))
    assert expected_slab_launches(CASES["overlap-3"]["script"]) == (0, 1) and expected_slab_launches(CASES["overlap-8"]["script"]) == (3, 0)
    assert expected_slab_launches(CASES["overlap-plain-3"]["script"]) == (1, 3) and expected_slab_launches(CASES["overlap-plain-8"]["script"]) == (3, 4)


@pytest.mark.parametrize("name", list(CASES))
def test_an_oracle_slab_holds_the_halo_rule_and_its_top_bound_is_sharp(oracle, name):
    """Part C: the reference alone on the rows this file compares.  Inside the bound nothing differs and the max diff over those
    rows is the whole raster's; the row above a live top bound, 3T-2, differs after every op.  The bottom bound is the contract and
    not sharp on this data (the module docstring has the distances)."""
    import slab_worker
    records = slab_worker.play_slab(oracle, oracle, CASES[name])
    print(name, [(r["op"], r["lo"], r["hi"], r["inside"], r["above"], r["below"]) for r in records])
    slab_worker.check_exact(records)
    for r in records:
        assert r["above"] is None or r["above"] > 0, f"{r['op']}: row {r['lo'] - 1} is exact as well after {r['T']} iterations"


def run_child(label):
    env, names = CHILDREN[label]
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(HERE, "slab_worker.py"), *names], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    print(f"child [{label}]: {time.time() - t0:.1f} s")
    assert p.returncode == 0, f"{label} {env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    results = json.loads(p.stdout.strip().splitlines()[-1])
    missing = [n for n in names if n not in results]
    assert not missing, f"{label}: no result for {missing}\n{p.stderr[-3000:]}"
    return results


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(CHILDREN))
def test_forced_marching_launches_on_slabs_match_the_oracle(hip, label):
    """Parts A and B, one child process per switch setting.  Launch counts are exact everywhere but under WDPM_BALANCE=2, where
    the claim is that a two-iteration launch ran from the balance table."""
    results = run_child(label)
    failures = []
    for case, r in results.items():
        two, one = iter2_launches(r)
        print(f"{case} [{label}]: {r['seconds']} s, {two} two-iteration launches, {one} single; {r['figures']}")
        if not r["ok"]:
            failures.append(f"{case} [{label}]: {r['error']}")
            continue
        if case in GROUP_CASES:
            want_two, want_one = expected_group_launches(GROUP_CASES[case], overlap=label != "groups, no overlap")
            if case != "group-k2" and two < 1:
                failures.append(f"{case} [{label}]: no two-iteration launch")
        else:
            want_two, want_one = expected_slab_launches(CASES[case]["script"])
        if label == "off":
            want_two, want_one = 0, 2 * want_two + want_one
        if label == "skewed chunk weights":
            if not any(int(b) & LEDGER_ITER2 and int(b) & LEDGER_BALANCE for k in PLAIN_KERNELS for b in r["switches"].get(k, {})):
                failures.append(f"{case} [{label}]: no two-iteration launch took its chunk heights from the balance table")
        elif (two, one) != (want_two, want_one):
            failures.append(f"{case} [{label}]: {two} two-iteration and {one} single launches, expected {want_two} and {want_one}")
    assert not failures, "\n".join(failures)
