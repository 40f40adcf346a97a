"""The one check of the pond outlets over row blocks (include/wdpm_group_pond_outlets.h) and the patterns that need a row-block
boundary, shared by tests/test_group_pond_outlets.py (N ranks on one GPU), tests/test_group_pond_outlets_tall.py and
tests/test_group_pond_outlets_multi_gpu.py (one rank per GPU).

Every check is equality: the outlet table and its counts against tests/pond_outlets_model.outlets on the labels the group returns,
the water the group downloads and device_dem of the uploaded DEM (integers by value, pour_level by bit pattern); against
Ponds.label_outlets on a twin whole-raster context that holds the same DEM and that water; labels, pond table, rim table, basin
raster, catchment table and catchment counts of the same call, bit for bit, against the label_catchments() of a twin group that holds
the same rasters; the two statements of include/wdpm_pond_outlets.h about every call; and no guard byte changed.  Patterns are
placed with rowblock.partition (padded rows; file = padded - 1)."""
import numpy as np

import group_pond_rims_cases as rc
from group_pond_catchments_cases import boundaries
from group_pond_rims_cases import ramp_dem
from group_ponds_cases import MISS, WET
from helpers import pad
from pond_catchments_model import catchments
from pond_outlets_model import assert_invariants, assert_same_outlets, outlets
from pond_rims_model import device_dem
from ponds_model import assert_same, inventory

Q = 2 ** 24
NONE = (np.inf, -1, -1, -1, -1, -1, 0, 0, 0, 0)
VARYING = ("resolve_ms", "rounds")          # of the catchment counts: host time, and rounds of relaxed atomics that really race


def row(table, k):
    return tuple(table[k].tolist())


def lesser(p):
    """what a label_catchments() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments()


def check_outlets(grp, p, bd, md, twin=None, whole=None):
    """label_outlets at md on the group's current water; returns (outlet table, outlet stats, basins, labels).  `twin`: a GroupPonds
    on a group with the same rasters, whose label_catchments() must leave everything else the call leaves.  `whole`: a (Context,
    Ponds) pair of the raster's shape, which is given the DEM and the group's water and must give the same table and counts."""
    from wdpm_amd.ponds import OUTLET_DTYPE
    n = p.label_outlets(md)
    table, stats, basin, labels = p.outlets(), p.outlet_stats(), p.basins(), p.labels()
    assert p.guard_bad() == 0
    water = grp.download_water()
    ref_labels, ref_ponds = inventory(bd > MISS, water, md)
    assert n == len(ref_ponds) == stats["ponds"] == len(table) == p.stats()["ponds"], (n, len(ref_ponds), stats)
    assert_same(labels, p.table(), ref_labels, ref_ponds)
    dem = device_dem(bd, MISS)
    ref_basin, _, _ = catchments(ref_labels, dem, water, ref_ponds)
    assert (basin == ref_basin).all()
    assert table.dtype == OUTLET_DTYPE
    assert_same_outlets(table, stats, *outlets(ref_labels, dem, water, ref_ponds, basin=ref_basin))
    assert_invariants(table, p.rims())
    assert stats["ranks"] == grp.size and 0 <= stats["seam_outlets"] <= n - stats["no_outlet"] and 0 <= stats["split_ponds"] <= n, stats
    assert stats["merge_ms"] >= 0, stats
    if grp.size == 1:
        assert stats["seam_outlets"] == stats["split_ponds"] == 0, stats
    if twin is not None:
        assert twin.label_catchments(md) == n
        for mine, theirs in zip(lesser(p), lesser(twin)):
            assert mine.tobytes() == theirs.tobytes()
        mine, theirs = p.catchment_stats(), twin.catchment_stats()
        assert {k: v for k, v in mine.items() if k not in VARYING} == {k: v for k, v in theirs.items() if k not in VARYING}
        assert p.rims_stats()["slots"] == twin.rims_stats()["slots"] and p.stats()["merged"] == twin.stats()["merged"]
        assert twin.guard_bad() == 0
    if whole is not None:
        ctx, q = whole
        ctx.upload(bd, water)
        assert q.label_outlets(md) == n
        assert q.outlets().tobytes() == table.tobytes()
        assert q.outlet_stats() == {k: stats[k] for k in ("ponds", "no_outlet", "to_land", "divide_cells")}
        assert q.guard_bad() == 0
    assert p.guard_bad() == 0
    return table, stats, basin, labels


class OutletCase:
    """Two groups with one handle each and a whole-raster context with its handle, for several DEMs and waters of one shape: the
    group under test, its twin, and the single-context answer."""

    def __init__(self, hip, R, Cc, devices, every=1, whole=True):
        from wdpm_amd.ponds import GroupPonds, Ponds
        from wdpm_amd.rowblock import Group
        self.R, self.Cc, self.n = R, Cc, len(devices)
        kw = {} if every is None else dict(exchange_every=every)
        self.grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.twin_grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.ponds = GroupPonds(self.grp)
        self.twin = GroupPonds(self.twin_grp)
        self.ctx = self.whole = None
        if whole:
            self.ctx = hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS, device=devices[0])
            self.whole = Ponds(self.ctx)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ponds.close()
        self.twin.close()
        self.grp.close()
        self.twin_grp.close()
        if self.whole is not None:
            self.whole.close()
            self.ctx.close()

    def upload(self, water, dem=None, nodata=None):
        assert water.shape == (self.R, self.Cc)
        if dem is None:
            dem = ramp_dem(self.R, self.Cc, nodata=nodata)
        elif nodata is not None:
            dem = np.where(nodata, MISS, dem)
        self.bd, bw = pad(dem, water, MISS)
        self.grp.upload(self.bd, bw)
        self.twin_grp.upload(self.bd, bw)

    def check(self, water, dem=None, nodata=None, thresholds=(WET,)):
        """water and dem in file layout; returns what check_outlets returns for the last threshold"""
        self.upload(water, dem, nodata)
        out = None
        for md in thresholds:
            out = check_outlets(self.grp, self.ponds, self.bd, md, self.twin, (self.ctx, self.whole) if self.whole is not None else None)
        return out


def empty(R, Cc):
    """a raster of NODATA and no water, file layout, and a setter that takes padded coordinates"""
    dem = np.full((R, Cc), MISS)
    w = np.zeros((R, Cc))

    def cell(r, c, e, d=0.0):
        dem[r - 1, c - 1], w[r - 1, c - 1] = e, d
    return dem, w, cell


# ---- the outlet pair across every boundary -------------------------------------------------------------------------------------
def lines_across(R, Cc, slabs, dr, dc):
    """tests/test_pond_outlets.lines_scene with every pair (a, b) across a row-block boundary: a rough plateau near 1000 m that holds
    short lines of low cells along (dr, dc), dr != 0, far from each other, each with one pair that is by far the lowest pass of both
    its ponds -
        kind 0:  pond (1.5 m) | a (3 m, drains back) | b (2.5 m, drains on) | pond (1.5 m)      a is a cell of the catchment
        kind 1:  a (a pond cell, surface 3 m) | b (2.5 m) | pond (1.5 m)                        a is a pond cell
    a in the last owned row above the boundary for dr > 0 and in the first one below it for dr < 0, on every boundary: with a on lane
    63 and b on lane 0 of the next segment or the other way round (straight: both on that lane), a in the middle of a segment, and a
    on padded column 1 / ncp - 2.  Returns the file rasters and the pairs as padded (a row, a col, b row, b col)."""
    rng = np.random.default_rng(100 + 17 * (3 * dr + dc) + R)
    dem = 1000.0 + np.round(rng.random((R, Cc)) * 8) / 4
    water = np.zeros((R, Cc))
    ncp = Cc + 2
    pairs = []
    for b, hi in enumerate(boundaries(slabs)):
        ar = hi if dr > 0 else hi + 1
        low = dc > 0 or (dc == 0 and dr > 0)
        want = [(1 if low else Cc, 1)] + [(seam - 1 if low else seam, (b + i) % 2) for i, seam in enumerate(range(64, ncp, 64))] + [(30, (b + 1) % 2)]
        taken = []                               # column ranges of the lines on this boundary: they keep two columns apart
        for ac, kind in want:
            cells = [(ar + k * dr, ac + k * dc) for k in ((-1, 0, 1, 2) if kind == 0 else (0, 1, 2))]
            lo, hi_c = min(c for _, c in cells), max(c for _, c in cells)
            if not all(1 <= r <= R and 1 <= c <= Cc for r, c in cells) or any(lo <= t1 + 2 and hi_c >= t0 - 2 for t0, t1 in taken):
                continue
            taken.append((lo, hi_c))
            levels = ((1.0, 0.5), (3.0, 0.0), (2.5, 0.0), (1.0, 0.5)) if kind == 0 else ((2.5, 0.5), (2.5, 0.0), (1.0, 0.5))
            for (r, c), (e, d) in zip(cells, levels):
                dem[r - 1, c - 1], water[r - 1, c - 1] = e, d
            pairs.append((ar, ac, ar + dr, ac + dc, kind))
    return dem, water, pairs


def run_lines_across(case, slabs, directions=((-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1))):
    for dr, dc in directions:
        dem, water, pairs = lines_across(case.R, case.Cc, slabs, dr, dc)
        table, stats, basin, _ = case.check(water, dem)
        assert len(pairs) >= 3 * (case.n - 1) and {k for *_, k in pairs} == {0, 1}
        for ar, ac, br, bc, _ in pairs:
            k, j = basin[ar, ac], basin[br, bc]
            assert k > 0 and j > 0 and k != j
            assert row(table, k - 1)[:6] == (3.0, ar, ac, br, bc, j) and row(table, j - 1)[:6] == (3.0, br, bc, ar, ac, k)
        assert stats["seam_outlets"] >= 2 * len(pairs) > 0, stats
        cols = {(ac, bc) for _, ac, _, bc, _ in pairs}
        assert ((63, 64) in cols if dc > 0 else (64, 63) in cols if dc < 0 else (63, 63) in cols or (64, 64) in cols), cols
        assert any(ac in (1, case.Cc) for ac, _ in cols), cols


# ---- ties across a boundary ----------------------------------------------------------------------------------------------------
def run_ties_across(case, slabs):
    """Pond A of two cells on both rows of a boundary, a pond above it and one below it behind one ridge cell each, both ridges at
    one level: the upper ridge drains up and away, so A meets it from a pond cell of the upper rank; the lower ridge ties and
    drains up into A, so A meets the pond below from that ridge, a cell of the lower rank.  Two passes at one height on two ranks:
    the upper rank's has the smaller index and wins.  A's fill cells lie on both ranks."""
    R, Cc = case.R, case.Cc
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in (63, 64, 1, Cc):
            for level in (3.0, 0.0, -0.0):
                dem, w, cell = empty(R, Cc)
                base = level - 2.0
                cell(hi - 2, c, base, 0.5)             # the pond above
                cell(hi - 1, c, level)                 # its ridge: both neighbours tie, up comes first
                cell(hi, c, base, 0.5)                 # A
                cell(hi + 1, c, base, 0.5)
                cell(hi + 2, c, level)                 # ties too, and drains up: A's catchment
                cell(hi + 3, c, base, 0.5)             # the pond below
                table, stats, basin, labels = case.check(w, dem)
                assert len(table) == 3 and basin[hi - 1, c] == 1 and basin[hi + 2, c] == 2, basin[hi - 2:hi + 4, c]
                assert row(table, 1)[:6] == (level, hi, c, hi - 1, c, 1) and np.signbit(table["pour_level"][1]) == np.signbit(level), table[1]
                assert (table["divide_cells"][1], table["fill_cells"][1], table["fill_q"][1]) == (2, 2, 3 * Q), table[1]
                assert stats["split_ponds"] == 1 and stats["seam_outlets"] == 0, stats      # every pair lies within one rank's rows


# ---- a basin over three ranks and more -----------------------------------------------------------------------------------------
def run_long_basin(case, slabs):
    """One pond down a whole column through every rank; its only pass is a ridge cell beside it in the middle of the second rank's
    rows, with another pond behind: every rank holds fill cells, one rank alone the pass."""
    R, Cc, n = case.R, case.Cc, case.n
    rm = (slabs[1].own_lo + slabs[1].own_hi) // 2
    for c in (62, 63, 1):
        dem, w, cell = empty(R, Cc)
        for r in range(1, R + 1):
            cell(r, c, 1.0, 0.5)
        cell(rm, c + 1, 3.0)                   # ties between the long pond (up-left comes first) and the pond behind
        cell(rm, c + 2, 1.0, 0.5)
        table, stats, basin, _ = case.check(w, dem)
        assert len(table) == 2 and basin[rm, c + 1] == 1
        assert row(table, 0) == (3.0, rm, c + 1, rm, c + 2, 2, 0, 1, R, R * int(1.5 * Q)), table[0]
        assert row(table, 1)[:6] == (3.0, rm, c + 2, rm, c + 1, 1), table[1]
        assert stats["split_ponds"] == 1 and stats["seam_outlets"] == 0, stats


# ---- a remote pond -------------------------------------------------------------------------------------------------------------
def run_remote(case, slabs):
    """tests/group_pond_catchments_cases.run_snake: a channel down one column through every rank, round in the last rank's rows and up
    another column into a pond cell in the first rank.  The basin's one pass lies beside the channel in the last rank's rows, which -
    with three ranks and more - neither owns nor borders the pond: the outlet is found through a remote slot."""
    R, Cc, n = case.R, case.Cc, case.n
    a = 4
    dem, w, cell = empty(R, Cc)
    path = [(r, a) for r in range(1, R + 1)] + [(R, a + 1)] + [(r, a + 2) for r in range(R, 1, -1)]
    for k, (r, c) in enumerate(path):
        cell(r, c, 300.0 - 0.125 * k)
    cell(1, a + 2, 100.0, 0.5)                 # the pond: label 1
    cell(R - 1, a + 3, 350.0)                  # beside the way up, drains away to ...
    cell(R - 1, a + 4, 100.0, 0.25)            # ... pond 2
    table, stats, basin, _ = case.check(w, dem)
    assert len(table) == 2 and basin[R - 1, a + 3] == 2 and (basin[1:-1, a] == 1).all()
    assert row(table, 0)[:6] == (350.0, R - 2, a + 2, R - 1, a + 3, 2) and table["fill_cells"][0] == len(path) + 1, table[0]
    assert row(table, 1)[:6] == (350.0, R - 1, a + 3, R - 2, a + 2, 1), table[1]
    assert stats["split_ponds"] == 1, stats
    if n >= 3:
        assert case.ponds.catchment_stats()["remote"] >= n - 2


# ---- mutual outlets, other destinations, barriers ------------------------------------------------------------------------------
def run_columns(case, slabs):
    """the hand-written answers of tests/test_pond_outlets.py stood on end, the pair (a, b) across a boundary, both ways up"""
    R, Cc = case.R, case.Cc
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in (63, 64, 1, Cc):
            for flip in (False, True):
                def column(levels, depths, first):
                    dem, w, cell = empty(R, Cc)
                    rows = list(range(first, first + len(levels)))
                    for r, e, d in zip(rows[::-1] if flip else rows, levels, depths):
                        cell(r, c, e, d)
                    return case.check(w, dem), (rows[::-1] if flip else rows)
                # two ponds that are each other's outlet: the 3 m cell on one side, the 2 m cell on the other, one pass each way
                if not flip:
                    (t, s, _, _), rows = column([1, 2, 3, 2, 1], [0.5, 0, 0, 0, 0.5], hi - 2)
                    assert row(t, 0) == (3.0, rows[2], c, rows[3], c, 2, 0, 1, 2, int(2.5 * Q)), t
                    assert row(t, 1) == (3.0, rows[3], c, rows[2], c, 1, 0, 1, 2, int(2.5 * Q)), t
                    assert s["seam_outlets"] == 2 and s["no_outlet"] == 0, s
                # basin 0 beyond the boundary
                (t, s, _, _), rows = column([1, 2, 3, 2.5, 2.75], [0.5, 0, 0, 0, 0], hi - 1 if flip else hi - 2)
                assert row(t, 0) == (3.0, rows[2], c, rows[3], c, 0, 0, 1, 2, int(2.5 * Q)) and s["to_land"] == 1 and s["seam_outlets"] == 1, (t, s)
                # a pond cell as `from` on one side, the ridge it spills to - which drains to the shallower pond - on the other
                (t, s, basin, _), rows = column([1, 3, 1], [0.5, 0, 0.25], hi - 1 if flip else hi)
                deep, other = basin[rows[0], c], basin[rows[2], c]
                assert sorted((deep, other)) == [1, 2] and basin[rows[1], c] == other
                assert row(t, deep - 1)[:6] == (3.0, rows[0], c, rows[1], c, other) and row(t, other - 1)[:6] == (3.0, rows[1], c, rows[0], c, deep), t
                assert s["seam_outlets"] == 2, s


def run_barriers(case, slabs):
    """NODATA along every boundary; one basin; no pond"""
    R, Cc = case.R, case.Cc
    w, nodata = rc.noise(R, Cc, 0.30, 17)
    for hi in boundaries(slabs):
        nodata[hi - 1, :] = True
    table, stats, _, _ = case.check(w, nodata=nodata)
    assert len(table) > 3 and stats["seam_outlets"] == 0, stats
    table, stats, basin, _ = case.check(np.full((R, Cc), 0.5))
    assert len(table) == 1 and row(table, 0) == NONE and stats["no_outlet"] == 1 and stats["split_ponds"] == 0, (table, stats)
    table, stats, _, _ = case.check(np.zeros((R, Cc)))
    assert len(table) == 0 and stats["ponds"] == 0 and len(case.ponds.outlets(capacity=0)) == 0, stats


# ---- a quiet row that is not quiet ---------------------------------------------------------------------------------------------
def run_not_quiet(case, slabs):
    """All of one rank's rows are one pond and nothing else; the facing row of the rank next door is NODATA but for one low dry
    cell, a pit: the rank's window is one basin wherever it looks in its own rows, and the one foreign cell of the halo row - on lane
    0 of a segment (beside the segment before it) or on lane 63 (beside the one after it) - is the pond's only pass."""
    R, Cc = case.R, case.Cc
    for b in sorted({0, len(slabs) - 2}):
        hi = slabs[b].own_hi
        for x in (64, 63):
            for below in (True, False):
                dem, w, cell = empty(R, Cc)
                own = slabs[b] if below else slabs[b + 1]
                for r in range(max(own.own_lo, 1), min(own.own_hi, R) + 1):
                    dem[r - 1, :], w[r - 1, :] = 10.0, 0.5
                halo, edge = (hi + 1, hi) if below else (hi, hi + 1)
                cell(halo, x, 5.0)
                table, stats, basin, _ = case.check(w, dem)
                assert len(table) == 1 and basin[halo, x] == 0
                assert row(table, 0) == (10.5, edge, x - 1, halo, x, 0, 0, 3, 0, 0), table[0]
                assert stats["seam_outlets"] == 1 and stats["to_land"] == 1 and stats["split_ponds"] == 0, stats


# ---- levels on the seam rows ---------------------------------------------------------------------------------------------------
def run_seam_levels(case, slabs):
    """signed zeros, films at or below the threshold and NaN water on both rows of every boundary: the neighbour's level comes from
    its owner's key"""
    R, Cc = case.R, case.Cc
    rng = np.random.default_rng(R * Cc + case.n)
    dem = ramp_dem(R, Cc, seed=3)
    w = np.zeros((R, Cc))
    for hi in boundaries(slabs):
        for r in (hi, hi + 1):
            dem[r - 1, :] = rng.choice([0.0, -0.0, 0.25, -0.25], Cc)
            kind = rng.random(Cc)
            w[r - 1, :] = np.where(kind < 0.2, WET, np.where(kind < 0.4, WET / 2, np.where(kind < 0.5, np.nan, np.where(kind < 0.6, 0.3, 0.0))))
    table, stats, _, _ = case.check(w, dem, thresholds=(WET, 0.0))
    assert len(table) > 3 and stats["seam_outlets"] > 0, stats


def run_noise(case, densities=(0.30, 0.41, 0.60), thresholds=(WET, 0.01)):
    for d in densities:
        w, nodata = rc.noise(case.R, case.Cc, d, int(d * 100) + case.R + case.n)
        table, stats, _, _ = case.check(w, nodata=nodata, thresholds=thresholds)
        assert len(table) > 10 and stats["seam_outlets"] > 0 and stats["split_ponds"] > 0, stats
