"""Strips of a two-iteration launch that lie beyond the raster's right edge retire at once (wdpm_march.hip::iter2_march): a consumer
whose strip stores nothing, a producer none of whose ring columns lies inside the raster.  The producer leaves +0.0 in its columns of
the ring, and its neighbours read them.

CPU: the rule restated as a function of (padded width, group, strip), and the dependency simulation of tests/test_pair_iterations.py
- given the one thing the argument rests on, that the raster's last padded column is NODATA and neither gives nor receives (DESIGN
4.2) - shows that no stored column depends on a retired strip's columns; without that wall they would.

GPU: forced two-iteration launches (child processes, tests/retired_worker.py) on rasters of two groups whose last group has three,
two and one strips wholly beyond the edge, bit for bit against the oracle."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from test_pair_iterations import FORCED, LEDGER_BALANCE, LEDGER_ITER2, PLAIN_KERNELS, expected_launches, iter2_launches, taint  # noqa: E402

# unpadded widths 761, 882, 1053 (padded 763, 884, 1055): group 1 starts at padded column 663, its strips at 834, 1005, 1176
WIDTHS = {761: 3, 882: 2, 1053: 1}          # -> strips of the last group wholly beyond the edge
SCRIPT = [("block", 4), ("block", 21)]
CASES = {}
for _m, _module in enumerate(("add", "subtract")):
    for _l, _level in enumerate(("codes16", "codes32")):
        for _w, _width in enumerate(WIDTHS):
            _rows = 300 + (_m + _l + _w) % 3                                    # 0, 1 and 2 mod 3 all occur, for every width
            CASES[f"{_module}-{_level}-{_width}"] = dict(module=_module, shape=(_rows, _width), level=_level, tiles=0, script=SCRIPT)
# tall chunks: the ring wraps many times
CASES["tall-761"] = dict(module="add", shape=(3000, 761), level="codes16", tiles=0, patches=True, script=SCRIPT)
CASES["tall-1053"] = dict(module="subtract", shape=(3000, 1053), level="codes32", tiles=0, script=[("block", 4)])


def constants():
    """the strip and group geometry of wdpm_dispatch.h"""
    src = open(os.path.join(ROOT, "wdpm_amd", "csrc", "wdpm_dispatch.h")).read()
    k = {}
    m = re.search(r"constexpr int kHaloL = (\d+), kHaloR = (\d+);", src)
    k["HaloL"], k["HaloR"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"constexpr int kGroupHaloL = (\d+), kGroupHaloR = (\d+);", src)
    k["GroupHaloL"], k["GroupHaloR"] = int(m.group(1)), int(m.group(2))
    k["StripIn"] = 192
    assert re.search(r"constexpr int kStripIn = 3 \* kLanes;", src) and re.search(r"constexpr int kLanes = 64;", src)
    k["StripOut"] = k["StripIn"] - k["HaloL"] - k["HaloR"]
    k["GroupIn"] = 3 * k["StripOut"] + k["StripIn"]
    k["GroupOut"] = k["GroupIn"] - k["GroupHaloL"] - k["GroupHaloR"]
    assert (k["StripOut"], k["GroupIn"], k["GroupOut"]) == (171, 705, 663)
    return k


K = constants()


def groups(ncp):
    """wdpm_dispatch.h::wdpm_groups"""
    first = K["GroupIn"] - K["GroupHaloR"]
    return 1 if ncp <= first else (ncp - first + K["GroupOut"] - 1) // K["GroupOut"] + 1


def strip_origin(grp, j):
    return K["GroupOut"] * grp + K["StripOut"] * j


def producer_columns(grp, j):
    """the padded columns a producer deposits in the ring: its exact ones, and the group's outer halos"""
    c0 = strip_origin(grp, j)
    return c0 + (0 if j == 0 else K["HaloL"]), c0 + (K["StripIn"] - 1 if j == 3 else K["StripIn"] - 1 - K["HaloR"])


def producer_retires(ncp, grp, j):
    return producer_columns(grp, j)[0] >= ncp


def consumer_stores(ncp, grp, j):
    """the padded columns [lo, hi] a consumer stores, or None"""
    c0 = strip_origin(grp, j)
    lo = (0 if grp == 0 else K["GroupHaloL"]) if j == 0 else K["HaloL"]
    hi = min(K["StripIn"] - 1 - (K["GroupHaloR"] if j == 3 else K["HaloR"]), ncp - 1 - c0)
    return (c0 + lo, c0 + hi) if hi >= lo else None


def consumer_retires(ncp, grp, j):
    return consumer_stores(ncp, grp, j) is None


def test_which_strips_retire():
    for width, beyond in WIDTHS.items():
        ncp = width + 2
        assert groups(ncp) == 2
        assert [strip_origin(1, j) for j in range(4)] == [663, 834, 1005, 1176]
        assert sum(strip_origin(1, j) > ncp - 1 for j in range(4)) == beyond
        gone = [j for j in range(4) if producer_retires(ncp, 1, j)]
        assert gone == list(range(4 - beyond, 4)), (width, gone)
        assert [j for j in range(4) if consumer_retires(ncp, 1, j)] == gone
        assert not any(producer_retires(ncp, 0, j) or consumer_retires(ncp, 0, j) for j in range(4))
    # the flagship: 16384^2, 25 groups, only the last group's last strip (it starts at padded column 16425)
    ncp = 16386
    assert groups(ncp) == 25 and strip_origin(24, 3) == 16425
    gone = [(g, j) for g in range(25) for j in range(4) if producer_retires(ncp, g, j)]
    assert gone == [(24, 3)] and gone == [(g, j) for g in range(25) for j in range(4) if consumer_retires(ncp, g, j)]


def test_retirement_over_every_width():
    """for every padded width: the stored columns still tile the raster, a group's first strip never retires, a producer retires only
    together with its consumer, and a retired producer's columns all lie beyond the raster"""
    for ncp in range(3, 3000):
        ng = groups(ncp)
        covered = np.zeros(ncp, int)
        for g in range(ng):
            for j in range(4):
                st = consumer_stores(ncp, g, j)
                if st is not None:
                    assert 0 <= st[0] <= st[1] <= ncp - 1
                    covered[st[0]:st[1] + 1] += 1
                if j == 0:
                    assert not producer_retires(ncp, g, j) and not consumer_retires(ncp, g, j), (ncp, g)
                else:
                    assert producer_retires(ncp, g, j) == consumer_retires(ncp, g, j), (ncp, g, j)
                if producer_retires(ncp, g, j):
                    assert producer_columns(g, j)[0] >= ncp
        assert (covered == 1).all(), ncp


def taint_walled(rows, cols, k, bad, wall):
    """test_pair_iterations.py::taint with cells that neither give nor receive (NODATA): nothing passes to, from or through them"""
    nb = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
    t = bad.copy()
    for _ in range(k):
        for oi in (1, 2, 3):
            for oj in (1, 2, 3):
                R, C = np.meshgrid(np.arange(oi, rows - 1, 3), np.arange(oj, cols - 1, 3), indexing="ij")
                live = ~wall[R, C]
                acc = t[R, C].copy()
                for di, dj in nb:
                    moves = live & ~wall[R + di, C + dj]
                    tn = t[R + di, C + dj]
                    t[R + di, C + dj] = np.where(moves, tn | acc, tn)
                    acc = np.where(moves, acc | tn, acc)
                t[R, C] = acc
    return t


def test_walled_simulation_is_the_plain_one_without_walls():
    rng = np.random.default_rng(3)
    bad = rng.random((40, 70)) < 0.02
    assert (taint_walled(40, 70, 2, bad, np.zeros_like(bad)) == taint(40, 70, 2, bad)).all()


@pytest.mark.parametrize("width", list(WIDTHS) + [16384])
def test_no_stored_column_depends_on_a_retired_strip(width):
    """everything a retired producer would have deposited is unknown from the start (and so is every other column beyond the raster:
    the neighbours' clamped loads); two iterations later no column a consumer stores has seen any of it - because of the border column"""
    ncp = width + 2
    ng = groups(ncp)
    cols = strip_origin(ng - 1, 3) + K["StripIn"]            # the groups' whole extent
    rows = 40
    bad = np.zeros((rows, cols), bool)
    retired = [(g, j) for g in range(ng) for j in range(4) if producer_retires(ncp, g, j)]
    assert retired
    for g, j in retired:
        lo, hi = producer_columns(g, j)
        bad[:, lo:hi + 1] = True
    assert not bad[:, :ncp].any()
    bad[:, ncp:] = True
    stored = np.zeros(cols, bool)
    for g in range(ng):
        for j in range(4):
            st = consumer_stores(ncp, g, j)
            if st is not None:
                stored[st[0]:st[1] + 1] = True
    assert stored[:ncp].all() and not stored[ncp:].any()
    wall = np.zeros((rows, cols), bool)
    wall[:, ncp - 1] = True                                 # the reference's border column: DEM NODATA
    after = taint_walled(rows, cols, 2, bad, wall)
    assert not after[:, stored].any()
    # and the wall is what the argument needs: without it the unknown columns reach stored ones within two iterations
    assert taint(rows, cols, 2, bad)[:, stored].any()


def run_children(jobs, timeout=600):
    import json
    import subprocess
    out = {}
    for label, (env, names) in jobs.items():       # one after the other
        p = subprocess.run([sys.executable, os.path.join(HERE, "retired_worker.py"), *names], cwd=ROOT, env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0, f"{label} {env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        out[label] = json.loads(p.stdout.strip().splitlines()[-1])
        missing = [n for n in names if n not in out[label]]
        assert not missing, f"{label}: no result for {missing}\n{p.stderr[-3000:]}"
    return out


@pytest.mark.gpu
def test_retired_strips_match_the_oracle(hip):
    res = run_children({"forced": (FORCED, list(CASES)),
                        "forced, skewed chunk weights": (dict(FORCED, WDPM_BALANCE="2"), ["add-codes16-761", "subtract-codes32-882", "tall-761"]),
                        "forced, a ring of two row triples": (dict(FORCED, WDPM_ITER2_RING="6"), ["add-codes32-1053", "subtract-codes16-761", "tall-761"])})
    failures = []
    for label, results in res.items():
        for case, r in results.items():
            if not r["ok"]:
                failures.append(f"{case} [{label}]: {r['error']}")
                continue
            two, one = iter2_launches(r)
            want_two, want_one = expected_launches(CASES[case]["script"])
            print(f"{case} [{label}]: {two} two-iteration launches, {one} single")
            if "skewed" in label:
                if not any(int(b) & LEDGER_ITER2 and int(b) & LEDGER_BALANCE for k in PLAIN_KERNELS for b in r["switches"].get(k, {})):
                    failures.append(f"{case} [{label}]: no two-iteration launch took its chunk heights from the balance table")
            elif (two, one) != (want_two, want_one):
                failures.append(f"{case} [{label}]: {two} two-iteration and {one} single launches, expected {want_two} and {want_one}")
    assert not failures, "\n".join(failures)
