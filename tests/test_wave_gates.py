"""The wave-uniform fast paths of the iteration kernels, with ONE trigger cell in every register slot that decides them.

  any_nodata16 (wdpm_march.hip::decode_rows)   a step whose wave holds no NODATA offset decodes its nine 16-bit DEM codes without the
                                               NODATA select; a gate that misses one decodes that cell to (base + 65535) / 10^e
  any_above_3m / deep_next (wdpm_iteration.h,  a step whose window holds no depth above 3 m runs the clamped neighbour step; a gate that
  wdpm_march.hip), deep_sh (wdpm_small.hip)    misses one cuts a flow above 1 m down to 1 m.  Single marching loop (three modules), both
                                               roles of the two-iteration loop, the relay kernel (a workgroup's waves OR their flags)

Both are max-of-nine reductions written out by hand; one lane's one register decides for 64 lanes (for a relay workgroup: for all
its waves).  Every case here holds exactly one trigger cell - a NODATA cell in a raster without any other inside the strip's reach, or
a depth of 100 m over water of a few centimetres - and the sweep moves it through every row from 2 to R - 1 (all three phases of a row
triple, the first and last triple of a chunk of 6 and of 12 rows and the warm-up rows of the next, every position in and across relay
workgroups of four and eight waves) and through all three column slots of lanes 0, 1, 2, 3, 7, 31, 32, 56, 61, 62 and 63 of the strip
that touches neither border (wave_gates_model.py has the rasters).  The NODATA sweep is repeated, on rows 2 .. 13 and lanes 0, 31, 63,
at the smallest width (854) at which the strip that opens the SECOND two-iteration group touches no border.  The depth sweep is
replayed with the first depth above the gate's 3 m line, with NaN and with -0.25 m.

CPU part (no GPU, never the code under test): every case BITES, that is, the mistake it guards against would change the result -
  NODATA  the oracle on garbage_dem (the trigger decoded without the select) differs from the oracle on the real DEM, within the
          iterations played, in a valid cell of the columns that the gated strip stores;
  depth   the always-clamped model of one iteration differs from the oracle in a valid cell (add / subtract and drain), after the same
          model with the exact step has equalled the oracle bit for bit on the very same case.
No case is exempt.  test_the_old_nodata_cases_cannot_tell keeps on record why this file exists: the three NODATA kinds of
test_dem16_bases.py give ZERO differing cells under garbage_dem.

GPU part: one child process per variant (tests/wave_gates_worker.py; the WDPM_* switches are read once per process), all positions in
each, every raster (with the block's max diff, with totaldrain) bit for bit against the oracle - through 32-byte digests of the oracle's
results, computed once per module here and shared; a case that differs is replayed on the oracle by the child to say where.  The ledger
must show that the intended instantiation ran (16-bit, 32-bit or fp64 marching kernel with or without the two-iteration bit, the relay
kernel of the forced height) with the NO_CLAMP bit CLEAR: otherwise a green run could mean that the gate was never live.

Not here: a depth that crosses 3 m only DURING a two-iteration launch's first iteration, which the consumer's own test alone sees.
The seeded search for such a raster (wave_gates_model.funnel_search: a low cell beside a deep hole, fed by two rings of ground at up
to 3.0 m of water under a dry rim) found none that bites: 2000 candidates for each of the nine colour phases of the low cell, in two
parametrisations of the ring heights and depths, not one on which "iteration 1 exact, iteration 2 always clamped" differs from the
oracle while iteration 1 leaves exactly one cell above 3 m.  The reason is the clamp's own margin: a flow exceeds 1 m only from a
centre above 8 m; with every OTHER cell at 3 m or less after iteration 1 the low cell, tuned by hand, stood at 7.25 m when it poured
in iteration 2.  No funnel is shipped that does not bite; test_the_funnel_search_finds_nothing keeps the search runnable.  What
holds the consumer's gate is the depth sweep under WDPM_ITER2=2: iterate(2) and iterate(4) from a 100 m and a 400 m cell leave depths
far above 3 m for the consumer to load, in rows and columns that the producer's test never saw deep."""
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import wave_gates_model as wg  # noqa: E402
from helpers import find_drain, n_bit_diff  # noqa: E402
from test_clamped_step import clamped_drain_step, clamped_step  # noqa: E402
from test_stencil_forms import nz_drain_step, nz_step  # noqa: E402

MISS = wg.MISS
LEDGER_NO_CLAMP, LEDGER_ITER2, LEDGER_RELAY_NO_CLAMP = 1, 16, 4
ITERATION_KERNELS = ("fused_iteration_kernel<", "relay_iteration_kernel<", "tri_iteration_kernel<", "pass_kernel<")
MARCH = dict(WDPM_RELAY="0", WDPM_TRI="0")
CODES = {"fp64": 0, "codes32": 1, "codes16": 2}

# variant -> what its child plays.  groups: (DEM level, chunk_rows, replays too?) - one context each
VARIANTS = {
    "nodata-single": dict(kind="nodata", env=dict(MARCH, WDPM_ITER2="0"), module="add", family="marching", iter2=False,
                          groups=[("codes16", 6, False), ("codes16", 12, False)]),
    "nodata-iter2": dict(kind="nodata", env=dict(MARCH, WDPM_ITER2="2"), module="add", family="marching", iter2=True,
                         groups=[("codes16", 0, False)]),
    "clamp-iter2-add": dict(kind="clamp", env=dict(MARCH, WDPM_ITER2="2"), module="add", family="marching", iter2=True,
                            groups=[("codes16", 0, True), ("codes32", 0, False)]),
    "clamp-relay-nw4": dict(kind="clamp", env=dict(WDPM_RELAY="2", WDPM_RELAY_NW="4"), module="add", family="relay", iter2=False,
                            relay=(4, False), groups=[(None, 0, True)]),
    "clamp-relay-nw8": dict(kind="clamp", env=dict(WDPM_RELAY="2", WDPM_RELAY_NW="8"), module="add", family="relay", iter2=False,
                            relay=(8, False), groups=[(None, 0, True)]),
    "clamp-relay-nw8-dem32": dict(kind="clamp", env=dict(WDPM_RELAY="2", WDPM_RELAY_NW="8", WDPM_DEM32="2"), module="add", family="relay",
                                  iter2=False, relay=(8, True), groups=[(None, 0, True)]),
}
for _module in ("add", "subtract", "drain"):
    for _level in CODES:
        VARIANTS[f"clamp-single-{_module}-{_level}"] = dict(kind="clamp", env=dict(MARCH, WDPM_ITER2="0"), module=_module, family="marching",
                                                            iter2=False, groups=[(_level, 6, True), (_level, 12, False)])
NODATA_VARIANTS = [v for v in VARIANTS if VARIANTS[v]["kind"] == "nodata"]
CLAMP_VARIANTS = [v for v in VARIANTS if VARIANTS[v]["kind"] == "clamp"]


def nodata_cases():
    """[(raster, (row, column))]: the 40 x 400 sweep, then the sweep at the group seam"""
    return [("main", p) for p in wg.main_positions()] + [("seam", p) for p in wg.seam_positions()]


def nodata_rasters():
    """{raster: (R, C, padded DEM without a trigger, padded water)}"""
    out = {}
    for name, R, C, pos in (("main", wg.R_MAIN, wg.C_MAIN, wg.main_positions()), ("seam", wg.R_SEAM, wg.C_SEAM, wg.seam_positions())):
        out[name] = (R, C) + wg.nodata_raster(R, C, pos)
    return out


def clamp_classes(replays):
    """{class: depth of the trigger}: 100 m, and the replays where the group plays them"""
    return dict(deep=wg.DEEP, **(wg.REPLAYS if replays else {}))


def clamp_cases():
    """[(class, (row, column))] in the reference's order: the 100 m sweep first, then the replays"""
    return [(cls, p) for cls in clamp_classes(True) for p in wg.main_positions()]


def reference_module(module):
    """the oracle runs add and subtract through the same sweep (oracle/wdpm_oracle.c::orc_pass looks at the module for drain alone),
    and so does the reference (runoffs()): one set of results serves both"""
    return "drain" if module == "drain" else "add"


def outlet_of(bd):
    return find_drain(bd)


# ------------------------------------------------------------------------------------------------ the rasters are what the file says

def test_positions_rasters_and_wells():
    pos = wg.main_positions()
    assert len(pos) == 38 * 33 and {r for r, _ in pos} == set(range(2, 40)) and len({r % 3 for r, _ in pos}) == 3
    cols = sorted({c for _, c in pos})
    assert cols[0] == 171 and cols[-1] == 362 and 171 + 3 * 31 in cols and 171 + 3 * 32 + 2 in cols
    # strip 1 of the 402-column raster loads 171 .. 362: no border column, and it is the only strip of which that is true
    strips = wg.strip_geometry(wg.C_MAIN + 2)
    assert len(strips) == 3 and [s[0] for s in strips] == [0, 171, 342] and strips[2][0] + wg.STRIP_IN - 1 >= wg.C_MAIN + 1
    assert wg.gated_store("main") == (179, 349)
    # the seam: 854 columns, padded 856; group 1 opens at 663 and its first strip loads 663 .. 854; one column less and it loads the border
    assert wg.C_SEAM == 854 and wg.strip_origin(1, 0) + wg.STRIP_IN - 1 == wg.C_SEAM and wg.gated_store("seam") == (680, 841)
    assert len(wg.seam_positions()) == 12 * 9
    for name, (R, C, bd, bw) in nodata_rasters().items():
        trig = sorted({c for r, c in (wg.main_positions() if name == "main" else wg.seam_positions())})
        valid = bd > MISS
        assert valid[1:-1, 1:-1].all() and not valid[0].any() and not valid[:, 0].any() and not valid[-1].any() and not valid[:, -1].any()
        q = np.rint(bd * 1e4).astype(np.int64)
        wells = np.nonzero(q[1] == wg.K_WELL)[0]
        assert (q[1:-1][:, wells] == wg.K_WELL).all() and (bw[:, wells] == 0).all()
        assert min(abs(w - t) for w in wells for t in trig) >= 3
        for g in range((C + 2 + wg.GROUP - 1) // wg.GROUP):                       # one well in every group of every row, spans <= 65534
            grp = q[1:-1, wg.GROUP * g:wg.GROUP * g + wg.GROUP]
            v = valid[1:-1, wg.GROUP * g:wg.GROUP * g + wg.GROUP]
            lo = np.where(v, grp, 1 << 40).min(axis=1)
            hi = np.where(v, grp, -1).max(axis=1)
            assert (lo == wg.K_WELL).all() and (hi - lo <= 65534).all() and ((grp == wg.K_WELL) & v).sum(axis=1).tolist() == [1] * R
        plateau = valid & (q != wg.K_WELL)
        assert q[plateau].min() >= 5_060_000 and q[plateau].max() <= 5_065_534 and (q[plateau] & 1).all() and (bw[plateau] == 0.8).all()
        # the garbage elevation, 506.5535, lies under every surface next to a trigger
        for r, c in ((2, trig[0]), (R - 1, trig[-1]), (7, trig[len(trig) // 2])):
            d, w = wg.with_nodata(bd, bw, (r, c))
            gd = wg.garbage_dem(d, MISS, wg.GRID_EXP, (r, c))
            assert gd[r, c] == 506.5535 and n_bit_diff(np.delete(gd.ravel(), r * (C + 2) + c), np.delete(d.ravel(), r * (C + 2) + c)) == 0
            around = (d + w)[r - 1:r + 2, c - 1:c + 2]
            assert (around[d[r - 1:r + 2, c - 1:c + 2] > MISS] > 506.5535).all()
    bd, bw = wg.clamp_raster(wg.R_MAIN, wg.C_MAIN)
    inner = bw[1:-1, 1:-1]
    assert (bd[1:-1, 1:-1] > 505.9).all() and 0 < inner.min() and inner.max() <= 0.1
    assert 3.0 < wg.REPLAYS["just-above-3m"] < 3.00001 and np.float64(wg.REPLAYS["just-above-3m"]).view(np.uint64) >> 32 == 0x40080001


def test_garbage_dem_follows_the_encoder():
    """the base is the lowest valid code of the cell's 48 padded columns of its row - not of the raster, not of the row"""
    bd = np.full((5, 100), MISS)
    bd[1:-1, 1:-1] = 700.0
    bd[2, 10], bd[2, 50], bd[3, 50] = 650.0, 640.0, MISS
    bd[2, 20] = bd[2, 60] = bd[1, 97] = MISS
    gd = wg.garbage_dem(bd, MISS, 4)
    assert gd[2, 20] == (6_500_000 + 65535) / 1e4 and gd[2, 60] == (6_400_000 + 65535) / 1e4 and gd[1, 97] == (7_000_000 + 65535) / 1e4
    assert gd[3, 50] == (7_000_000 + 65535) / 1e4 and gd[0, 0] == MISS and gd[2, 99] == MISS
    assert n_bit_diff(wg.garbage_dem(bd, MISS, 4, (2, 20)), np.where(np.arange(500).reshape(5, 100) == 220, gd, bd)) == 0


# ------------------------------------------------------------------------------------------------ every case bites (CPU)

def _oracle_runs(oracle, module, R, C, jobs, outlet=None):
    """jobs: [(padded DEM or None for "as uploaded last", padded water, iterations)] on one context; yields the rasters"""
    kw = dict(module=module, nrows=R, ncols=C, missingvalue=MISS)
    if module == "drain":
        kw.update(drainrow=outlet[0], draincol=outlet[1])
    with oracle.context(**kw) as o:
        for bd, bw, n in jobs:
            if bd is not None:
                o.upload(bd, bw)
            else:
                o.upload_water(bw)
            o.iterate(n)
            yield o.download_water()


def test_every_nodata_case_bites(oracle):
    """the oracle on the DEM whose trigger cell holds the select-free decode's elevation, against the oracle on the real DEM: a valid
    cell of the gated strip's stored columns differs after 1, 2 or 5 iterations - the steps the GPU cases play"""
    rasters = nodata_rasters()
    late, blind = {}, []
    for name, pos in nodata_cases():
        R, C, bd, bw = rasters[name]
        lo, hi = wg.gated_store(name)
        d, w = wg.with_nodata(bd, bw, pos)
        g = wg.garbage_dem(d, MISS, wg.GRID_EXP, pos)
        kw = dict(module="add", nrows=R, ncols=C, missingvalue=MISS)
        with oracle.context(**kw) as a, oracle.context(**kw) as b:
            a.upload(d, w)
            b.upload(g, w)
            done = 0
            for n in (1, 2, 5):
                for c in (a, b):
                    c.iterate(n - done)
                done = n
                wa, wb = a.download_water(), b.download_water()
                differ = (wa.view(np.uint64) != wb.view(np.uint64)) & (d > MISS)
                if differ[:, lo:hi + 1].any():
                    break
            else:
                blind.append((name, pos))
            if n > 1:
                late[(name, pos)] = n
    assert not blind, f"{len(blind)} cases would not show a missed NODATA offset: {blind[:10]}"
    # where it takes more than one iteration: the lanes in the strip's halo, whose columns the strip does not store
    assert all(not (lo <= c <= hi) for (name, (r, c)) in late for lo, hi in [wg.gated_store(name)]), sorted(late)[:10]


def crop_origin(c, ncp, width):
    """first padded column of the window of `width` columns around column c: a multiple of 3, so that the window's blocks are the raster's"""
    return min(max(3 * ((c - width // 2) // 3), 0), ncp - width)


@pytest.mark.parametrize("depth", [wg.DEEP, wg.DEEPER])
@pytest.mark.parametrize("module", ["add", "drain"])
def test_model_equals_oracle_and_every_depth_case_bites(oracle, module, depth):
    """One iteration on every 100 m case, and on every 400 m case.  The model runs on a window of 87 columns around the trigger (all rows), all cases of a
    window at once; what it says is compared on the 41 columns around the trigger, where neither the window's edge (an error travels
    at most two cells per colour pass, 18 per iteration) nor anything else can reach - and outside those the oracle's raster must be
    the trigger-free raster's, so the comparison covers the whole case.  First the exact step: bit for bit the oracle.  Then the
    always-clamped step: a valid cell differs.  (add serves subtract: reference_module.)

    The third history bit of deep_next (the rows loaded two steps ago) has a condition of its own: the step clamped in the last row
    alignment only (oi = 3, the stage that runs on those rows) and exact in the first two.  For a trigger in the last row of a triple
    (padded row = 2 mod 3) whose row below lies inside the raster that must differ from the oracle - and it does at 400 m and does
    NOT at 100 m, which is why the 400 m replay exists: mutants of deep_next that keep two bits pass every 100 m case."""
    W, HALF = 87, 20
    bd, bw = wg.clamp_raster(wg.R_MAIN, wg.C_MAIN)
    ncp = wg.C_MAIN + 2
    assert (ncp - W) % 3 == 0
    outlet = outlet_of(bd) if module == "drain" else None
    exact, clamped = (nz_drain_step, clamped_drain_step) if module == "drain" else (nz_step, clamped_step)
    pos = wg.main_positions()
    runs = _oracle_runs(oracle, module, wg.R_MAIN, wg.C_MAIN, [(bd, bw, 1)] + [(None, wg.with_depth(bw, p, depth), 1) for p in pos], outlet)
    base = next(runs)
    want = dict(zip(pos, runs))
    windows = {}
    for p in pos:
        windows.setdefault(crop_origin(p[1], ncp, W), []).append(p)
    toothless = []
    for lo, group in windows.items():
        sl = slice(lo, lo + W)
        batch = np.stack([wg.with_depth(bw, p, depth)[:, sl] for p in group])
        out_c = (outlet[0], outlet[1] - lo) if outlet is not None and 1 <= outlet[1] - lo <= W - 2 else None
        got = {}
        for name, step in (("exact", exact), ("clamped", clamped), ("late", {1: exact, 2: exact, 3: clamped})):
            res = wg.iterate(batch, bd[:, sl], MISS, step, outlet=out_c)
            got[name] = res[0] if out_c is not None else res
        for k, (r, c) in enumerate(group):
            a, b = max(c - HALF, 0), min(c + HALF + 1, ncp)
            o = want[(r, c)]
            assert n_bit_diff(got["exact"][k][:, a - lo:b - lo], o[:, a:b]) == 0, f"the exact model is not the oracle at {(r, c)}"
            assert n_bit_diff(o[:, :a], base[:, :a]) == 0 and n_bit_diff(o[:, b:], base[:, b:]) == 0, f"the trigger at {(r, c)} reaches further"
            differ = (got["clamped"][k][:, a - lo:b - lo].view(np.uint64) != o[:, a:b].view(np.uint64)) & (bd[:, a:b] > MISS)
            if not differ.any():
                toothless.append((r, c))
            if r % 3 == 2 and r + 1 <= wg.R_MAIN:
                late = int(((got["late"][k][:, a - lo:b - lo].view(np.uint64) != o[:, a:b].view(np.uint64)) & (bd[:, a:b] > MISS)).sum())
                assert (late > 0) == (depth == wg.DEEPER), f"{depth} m at {(r, c)}: clamping the last row alignment alone changes {late} cells"
    assert not toothless, f"{len(toothless)} cases on which the clamped step changes nothing: {toothless[:10]}"


def test_drain_model_with_the_trigger_at_the_outlet(oracle):
    """the drain sweep's outlet handling in the model - centre skipped, both cells emptied, the 3 x 3 cleared, totaldrain - whole raster"""
    bd, bw = wg.clamp_raster(wg.R_MAIN, wg.C_MAIN)
    out = outlet_of(bd)
    for dr, dc in ((1, 1), (0, -1), (-1, 0), (2, 2)):
        w0 = wg.with_depth(bw, (out[0] + dr, out[1] + dc), wg.DEEP)
        with oracle.context(module="drain", nrows=wg.R_MAIN, ncols=wg.C_MAIN, missingvalue=MISS, drainrow=out[0], draincol=out[1]) as o:
            o.upload(bd, w0)
            o.iterate(2)
            w, td = o.download_water(), o.totaldrain
        wm, tdm = wg.iterate(w0, bd, MISS, nz_drain_step, n=2, outlet=out)
        assert n_bit_diff(wm, w) == 0 and np.float64(tdm).view(np.uint64) == np.float64(td).view(np.uint64)


def test_the_old_nodata_cases_cannot_tell(oracle):
    """On record: the three NODATA kinds of test_dem16_bases.py, at all five widths, give ZERO differing valid cells when every
    interior NODATA cell holds the select-free decode's elevation - the relief there is under 1 m per group, so the mis-decoded cell
    stands 6.55 m above its group's base, above every surface around it, holds no water and nothing flows.  Those cases check the
    geometry of the bases (group edges, first columns, empty groups), NOT the select; this file does."""
    import test_dem16_bases as old
    for kind in ("one-nodata", "nodata-first-column", "nodata-group"):
        replaced = 0
        for w in old.WIDTHS:
            c = old.build_case(f"{kind}-{w}")
            g = wg.garbage_dem(c["bd"], c["miss"], 4)
            assert (g[1:-1, 1:-1] > c["miss"]).all()
            replaced += int((c["bd"][1:-1, 1:-1] <= c["miss"]).sum())
            runs = list(_oracle_runs(oracle, "add", c["R"], c["C"], [(c["bd"], c["bw"], old.BLOCK), (g, c["bw"], old.BLOCK)]))
            differ = (runs[0].view(np.uint64) != runs[1].view(np.uint64)) & (c["bd"] > c["miss"])
            assert differ.sum() == 0, (kind, w, int(differ.sum()))
        assert replaced > 0, kind


def test_the_funnel_search_finds_nothing():
    """on record (see the module's docstring): a sample of the seeded search, last colour phase - the low cell pours after all eight
    neighbours - finds no funnel that bites; the one deep cell of iteration 1 stays far under the 8 m a flow above 1 m takes"""
    hits, deepest = wg.funnel_search((0, 0), 100, 1000, nz_step, clamped_step)
    assert hits == [] and 3.0 < deepest < 6.0


# ------------------------------------------------------------------------------------------------ the oracle's word, once (GPU part)

def _threads():
    return max(1, min(16, os.cpu_count() or 1))


def _spread(n, parts):
    step = (n + parts - 1) // parts
    return [range(a, min(a + step, n)) for a in range(0, n, step)]


def nodata_reference(oracle):
    """digests [case][step] of every NODATA case, in nodata_cases()' order"""
    rasters, cases = nodata_rasters(), nodata_cases()
    out = np.zeros((len(cases), len(wg.NODATA_STEPS), 32), np.uint8)

    def work(idx):
        ctxs = {}
        for i in idx:
            name, pos = cases[i]
            R, C, bd, bw = rasters[name]
            if name not in ctxs:
                ctxs[name] = oracle.context(module="add", nrows=R, ncols=C, missingvalue=MISS)
            d, w = wg.with_nodata(bd, bw, pos)
            ctxs[name].upload(d, w)
            for s, (raster, scalars) in enumerate(wg.play_nodata(ctxs[name], w)):
                out[i, s] = wg.digest(raster, *scalars)
        for c in ctxs.values():
            c.close()

    with ThreadPoolExecutor(_threads()) as pool:
        list(pool.map(work, _spread(len(cases), 4 * _threads())))
    return out


def clamp_reference(oracle, module):
    """digests [case][step] of every depth case of the module, in clamp_cases()' order"""
    bd, bw = wg.clamp_raster(wg.R_MAIN, wg.C_MAIN)
    cases, classes = clamp_cases(), clamp_classes(True)
    out = np.zeros((len(cases), len(wg.CLAMP_STEPS), 32), np.uint8)
    kw = dict(module=module, nrows=wg.R_MAIN, ncols=wg.C_MAIN, missingvalue=MISS)
    if module == "drain":
        kw.update(zip(("drainrow", "draincol"), outlet_of(bd)))

    def work(idx):
        with oracle.context(**kw) as o:
            o.upload(bd, bw)
            for i in idx:
                cls, pos = cases[i]
                for s, (raster, scalars) in enumerate(wg.play_clamp(o, wg.with_depth(bw, pos, classes[cls]), module == "drain")):
                    out[i, s] = wg.digest(raster, *scalars)

    with ThreadPoolExecutor(_threads()) as pool:
        list(pool.map(work, _spread(len(cases), 4 * _threads())))
    return out


@pytest.fixture(scope="module")
def references(oracle, tmp_path_factory):
    """path of the file the children read, filled per kind on first use"""
    d = tmp_path_factory.mktemp("wave_gates")
    made = {}

    def get(kind, module):
        key = f"{kind}-{reference_module(module)}"
        if key not in made:
            made[key] = str(d / f"{key}.npy")
            np.save(made[key], nodata_reference(oracle) if kind == "nodata" else clamp_reference(oracle, reference_module(module)))
        return made[key]
    return get


# ------------------------------------------------------------------------------------------------ GPU

def kernel_name(v, level, plain):
    """the instantiation a group's steady launches must be"""
    if v["family"] == "relay":
        nw, dem32 = v["relay"]
        return f"relay_iteration_kernel<0, false, {'true' if plain else 'false'}, {nw}, {'true' if dem32 else 'false'}>"
    return f"fused_iteration_kernel<{2 if v['module'] == 'drain' else 0}, false, {CODES[level]}, false, false, {'true' if plain else 'false'}>"


def launches_per_case(v, plain):
    """(two-iteration launches, single launches) of the steady instantiation that one case adds to the ledger"""
    if v["kind"] == "nodata":             # test_dem16_bases.expected_launches: a block's first launch flushes, its last folds the max diff
        steady = [1, 2, 5, 6 - 2]
    else:
        steady = [1, 2, 4]
    if v["iter2"] and plain:
        return sum(s // 2 for s in steady), sum(s % 2 for s in steady)
    return 0, sum(steady)


def judge(name, res):
    v = VARIANTS[name]
    failures = list(res["failures"])
    if res.get("fatal"):
        failures.append(f"stopped: {res['fatal']}")
    no_clamp = LEDGER_RELAY_NO_CLAMP if v["family"] == "relay" else LEDGER_NO_CLAMP
    for g in res["groups"]:
        level = g["level"]
        if v["kind"] == "nodata" or level == "codes16":
            if g["dem16"] != 1:
                failures.append(f"{g['label']}: WDPM_OPT_DEM16 reports {g['dem16']}: the 16-bit codes are not in use")
        for cls, c in g["classes"].items():
            plain = cls not in ("nan", "negative")
            kernel = kernel_name(v, level, plain)
            states = {int(b): n for b, n in c["switches"].get(kernel, {}).items()}
            two = sum(n for b, n in states.items() if v["family"] == "marching" and b & LEDGER_ITER2)
            one = sum(states.values()) - two
            want = tuple(n * c["cases"] for n in launches_per_case(v, plain))
            if (two, one) != want:
                failures.append(f"{g['label']}/{cls}: {two} two-iteration and {one} single launches of {kernel}, expected {want}")
            for k, by in c["switches"].items():
                if not k.startswith(ITERATION_KERNELS):
                    continue
                if any(int(b) & no_clamp for b in by):
                    failures.append(f"{g['label']}/{cls}: {k} ran with the NO_CLAMP bit set (states {sorted(by)}): the gate under test was not live")
                steady_only = v["kind"] == "clamp"          # a block's first and last launch are other instantiations of the same family and codes
                if (k != kernel) if steady_only else (not k.startswith("fused_iteration_kernel<0, false, 2, ")):
                    failures.append(f"{g['label']}/{cls}: launches of {k} beside {kernel}")
    return failures


def play_variant(name, references, timeout=300):
    v = VARIANTS[name]
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(HERE, "wave_gates_worker.py"), references(v["kind"], v["module"]), name], cwd=ROOT,
                       env=dict(os.environ, **v["env"]), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"{name}: {res['cases']} cases, {res['seconds']:.1f} s in the child, {time.time() - t0:.1f} s in all")
    failures = judge(name, res)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])
    expected = sum(len(nodata_cases()) if v["kind"] == "nodata" else len(wg.main_positions()) * len(clamp_classes(r)) for _, _, r in v["groups"])
    assert res["cases"] == expected, (res["cases"], expected)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", NODATA_VARIANTS)
def test_one_nodata_cell_in_every_slot(hip, references, variant):
    play_variant(variant, references)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", CLAMP_VARIANTS)
def test_one_deep_cell_in_every_slot(hip, references, variant):
    play_variant(variant, references)
