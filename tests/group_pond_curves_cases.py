"""The one check of the pond stage curves over row blocks (include/wdpm_group_pond_curves.h) and the scenes that need a row-block
boundary, shared by tests/test_group_pond_curves.py (N ranks on one GPU) and tests/test_group_pond_curves_multi_gpu.py (one rank per
GPU).

Every check is equality: the curve table and its counts against tests/pond_curves_model.curves on the water the group downloads and
device_dem of the uploaded DEM (integers by value, doubles by bit pattern; the reference is computed once per water:
tests/test_pond_curves.reference); against Ponds.label_curves on a twin whole-raster context that holds the same DEM and that water;
labels, pond table, rim table, basin raster, catchment table, outlet table and the counts of the same call against the
label_outlets() of a twin group that holds the same rasters; what include/wdpm_pond_curves.h states of every call; and no guard byte
changed.  Scenes are placed with rowblock.partition (padded rows; file = padded - 1)."""
import numpy as np

from group_pond_catchments_cases import boundaries
from group_pond_outlets_cases import VARYING, OutletCase, empty
from group_ponds_cases import MISS, WET
from pond_curves_model import STAGES, assert_invariants, assert_same_curves, stage_levels
from test_pond_curves import reference

Q = 2 ** 24
WHOLE = ("ponds", "no_curve", "flat", "stage_cells")


def older(p):
    """what a label_outlets() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.outlets()


def plain(stats, drop):
    return {k: v for k, v in stats.items() if k not in drop}


def check_curves(grp, p, bd, md, twin=None, whole=None):
    """label_stage_curves at md on the group's current water; returns (curve table, curve stats, basins)"""
    from wdpm_amd.ponds import CURVE_DTYPE
    n = p.label_stage_curves(md)
    table, stats, basin = p.stage_curves(), p.stage_curve_stats(), p.basins()
    assert p.guard_bad() == 0
    water = grp.download_water()
    ref_basin, ref_out, ref_table, ref_stats = reference(bd, MISS, water, md)
    assert n == len(ref_table) == stats["ponds"] == len(table) == p.stats()["ponds"], (n, len(ref_table), stats)
    assert table.dtype == CURVE_DTYPE and (basin == ref_basin).all()
    assert_same_curves(table, stats, ref_table, ref_stats)
    assert_invariants(table, p.outlets())
    assert stats["ranks"] == grp.size and 0 <= stats["remote_beds"] <= stats["split_basins"] <= n and stats["merge_ms"] >= 0, stats
    if grp.size == 1:
        assert stats["split_basins"] == stats["remote_beds"] == 0, stats
    if twin is not None:
        assert twin.label_outlets(md) == n
        for mine, theirs in zip(older(p), older(twin)):
            assert mine.tobytes() == theirs.tobytes()
        assert plain(p.catchment_stats(), VARYING) == plain(twin.catchment_stats(), VARYING)
        assert plain(p.outlet_stats(), ("merge_ms",)) == plain(twin.outlet_stats(), ("merge_ms",))
        assert p.rims_stats()["slots"] == twin.rims_stats()["slots"] and p.stats()["merged"] == twin.stats()["merged"]
        assert twin.guard_bad() == 0
    if whole is not None:
        ctx, q = whole
        ctx.upload(bd, water)
        assert q.label_curves(md) == n
        assert q.curves().tobytes() == table.tobytes()
        assert q.curve_stats() == {k: stats[k] for k in WHOLE}
        assert q.guard_bad() == 0
    assert p.guard_bad() == 0
    return table, stats, basin


class CurveCase(OutletCase):
    """the group under test, its twin and the single-context answer of tests/group_pond_outlets_cases.OutletCase, asked for curves"""

    def check(self, water, dem=None, nodata=None, thresholds=(WET,)):
        """water and dem in file layout; returns what check_curves returns for the last threshold"""
        self.upload(water, dem, nodata)
        out = None
        for md in thresholds:
            out = check_curves(self.grp, self.ponds, self.bd, md, self.twin, (self.ctx, self.whole) if self.whole is not None else None)
        return out


def counts_below(ground, bed, top):
    """how many of `ground` lie strictly below each of the sixteen stages between bed and top, by the model's stage rule"""
    h = stage_levels(bed, top)[1:, 0]
    return [int((np.asarray(ground) < hs).sum()) for hs in h]


def column(case, c, start, step, levels, depths, **kw):
    """one column of cells in a raster of NODATA: levels[i] on padded row start + i * step; returns (check's answer, those rows)"""
    dem, w, cell = empty(case.R, case.Cc)
    rows = [start + i * step for i in range(len(levels))]
    for r, e, d in zip(rows, levels, depths):
        cell(r, c, e, d)
    return case.check(w, dem, **kw), rows


def both_ways(hi):
    """(start, step) of a column whose first cell is the last owned row above the boundary below `hi` and that runs down across it,
    and of its mirror image: the first cell on the first owned row below, running up"""
    return ((hi, 1), (hi + 1, -1))


# ---- a bed that lies in another rank -------------------------------------------------------------------------------------------
def run_remote_bed(case, slabs):
    """pond | 2 m || 3 m | 4 m | ridge 5 m | 2 m | pond: the first basin's bed (1 m) lies on one side of the boundary (||), its
    higher ground on the other; the ridge drains away, so the basin spills at 5 m.  A rank that took its own lowest ground (3 m) for
    the bed would form other heights and count other cells: that is asserted from the model's stage rule before the device is asked.
    flip: the bed below the boundary."""
    levels, depths = [1.0, 2.0, 3.0, 4.0, 5.0, 2.0, 0.5], [0.5, 0, 0, 0, 0, 0, 0.5]
    right, wrong = counts_below([3.0, 4.0], 1.0, 5.0), counts_below([3.0, 4.0], 3.0, 5.0)
    assert right != wrong and right == [0] * 8 + [1] * 4 + [2] * 4 and wrong == [1] * 8 + [2] * 8
    ran = 0
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in (63, 64, 1, case.Cc):
            for start, step in both_ways(hi):
                if not 1 <= start + 5 * step <= case.R:       # the pond cell lies one row before `start`, the last cell five rows on
                    continue
                ran += 1
                (t, s, basin), rows = column(case, c, start - step, step, levels, depths)
                k = basin[rows[0], c]
                assert len(t) == 2 and k > 0 and all(basin[r, c] == k for r in rows[:4]) and basin[rows[4], c] != k
                assert (t["bed_level"][k - 1], t["top_level"][k - 1]) == (1.0, 5.0)
                assert t["cells"][k - 1].tolist() == counts_below([1.0, 2.0, 3.0, 4.0], 1.0, 5.0) == [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4
                assert t["q"][k - 1][15] == (4 + 3 + 2 + 1) * Q
                if case.n > 1:
                    assert s["split_basins"] >= 1 and s["remote_beds"] >= 1, s
    assert ran >= 8


# ---- one basin over every rank -------------------------------------------------------------------------------------------------
def run_skipped_rank(case, slabs):
    """One basin down a whole column through all eight ranks: its bed, a pond cell, in the middle of rank 5's rows; its only pass in
    rank 0's rows, beside the column's third row; the ground rises by 1/4 m per row away from the pond's surface.  Ranks 1 to 4 hold cells of
    the catchment only, neither the bed nor the pass, and must form the heights from a bed they never saw.  The last rank's cells
    all stand AT or above the top and are counted at no stage.  (A rank BETWEEN pass and bed cannot hold such cells only: every
    descent from the pass cell to the bed crosses its rows, strictly falling from a level that is at most the pour level.)"""
    R, n = case.R, case.n
    assert n == 8
    rb = (slabs[5].own_lo + slabs[5].own_hi) // 2
    lo7 = slabs[7].own_lo
    for c in (62, 1, case.Cc - 2):
        dem, w, cell = empty(R, case.Cc)
        top = 0.5 + 0.25 * (rb - 2) - 0.125
        for r in range(2, R + 1):
            cell(r, c, 0.5 + 0.25 * abs(r - rb) if r < lo7 else top + 0.5 * (r - lo7))
        cell(rb, c, 0.0, 0.5)
        cell(2, c + 1, top)                    # below the column's second row, above its third: drains on to ...
        cell(2, c + 2, -10.0, 0.5)             # ... the pond behind
        assert 0.5 + 0.25 * (lo7 - 1 - rb) < top
        t, s, basin = case.check(w, dem)
        k = basin[rb, c]
        assert len(t) == 2 and (basin[2:R + 1, c] == k).all() and basin[2, c + 1] != k
        assert (t["bed_level"][k - 1], t["top_level"][k - 1]) == (0.0, top), t[k - 1]
        assert t["cells"][k - 1][15] == (lo7 - 1) - 3 + 1, t[k - 1]          # rows 3 .. lo7 - 1: neither row 2 nor the last rank's
        assert s["split_basins"] >= 1 and s["remote_beds"] >= 1, s


# ---- beds on the edges of waves, strips and rasters ----------------------------------------------------------------------------
def cones(R, Cc, spots, radius=2):
    """tests/test_pond_curves.cones_scene with small cones: a plateau near 1000 m that falls slowly towards the last column, one pit
    per spot (padded row, padded column) whose ground rises 1/4 m per step of Chebyshev distance from a bed of its own height; the
    bed cell holds water.  The plateau to the left of a pit drains into it: every basin is a band across the segments."""
    r, c = np.mgrid[1:R + 1, 1:Cc + 1]
    dem = 1000.0 - c / 1024.0
    water = np.zeros((R, Cc))
    beds = []
    for i, (pr, pc) in enumerate(spots):
        d = np.maximum(abs(r - pr), abs(c - pc))
        bed = 998.5 + i / 64.0
        dem = np.where(d <= radius, bed + d * 0.25, dem)
        water[pr - 1, pc - 1] = 0.2
        beds.append(bed)
    return dem, water, beds


def run_edges(case, slabs):
    """a bed on the last owned row above and on the first owned row below every boundary: on lanes 63 and 0 (padded columns 63 and
    64) and on padded columns 1 and ncp - 2"""
    Cc = case.Cc
    pairs = [(63, 1), (64, Cc), (1, 64), (Cc, 63)]
    spots = []
    for b, hi in enumerate(boundaries(slabs)):
        above, below = pairs[b % 4]
        spots += [(hi, above), (hi + 1, below)]
    dem, water, beds = cones(case.R, Cc, spots)
    t, s, basin = case.check(water, dem)
    assert len(t) == len(spots) and s["no_curve"] == 0
    for (pr, pc), bed in zip(spots, beds):
        k = basin[pr, pc]
        assert k > 0 and t["bed_level"][k - 1] == bed and t["top_level"][k - 1] > bed and t["cells"][k - 1][0] >= 1, (pr, pc, t[k - 1])
    cols = [np.flatnonzero((basin == k + 1).any(axis=0)) for k in range(len(t))]
    assert any(cc.min() <= 63 and cc.max() >= 64 for cc in cols)              # a band of basin across lanes 63 | 0
    assert s["split_basins"] > 0, s
    return t, s


def stripes(R, Cc):
    """tests/test_pond_curves.test_a_lane_whose_basin_changes_row_by_row stood on end: every odd column is a perched pond of its own
    down all rows, over a wavy bed; every even column a valley 100 m lower that falls to a pit in the last row.  Along a row the basin
    changes in every lane, and every pond lies in every rank."""
    r, c = np.mgrid[1:R + 1, 1:Cc + 1]
    k = (c + 1) // 2
    pond = c % 2 == 1
    dem = np.where(pond, 299.75 + k - (r % 8) / 64.0, 200.0 - r / 256.0)
    return dem, np.where(pond, 300.0 + k - dem, 0.0)


def run_stripes(case):
    R, Cc = case.R, case.Cc
    t, s, basin = case.check(*stripes(R, Cc)[::-1])
    ponds = (Cc + 1) // 2
    assert len(t) == ponds and plain(s, ("merge_ms",)) == dict(ponds=ponds, no_curve=0, flat=0, stage_cells=ponds * R, ranks=case.n,
                                                                 split_basins=ponds if case.n > 1 else 0,
                                                                 remote_beds=ponds if case.n > 1 else 0), s
    assert (basin[1:-1, 2:-1:2] == 0).all() and (t["top_level"] - t["bed_level"] == 0.25 + 7 / 64.0).all()


# ---- the stage rule ------------------------------------------------------------------------------------------------------------
def run_stage_rule(case, slabs):
    """the stepped pyramid of tests/test_pond_curves_model.py (Z = 0, P = 16, h_s = s) centred on a boundary: a cell at exactly h_s
    lies on either side of it; and the half-to-even pair of that file as a column, one cell of the pair in either rank"""
    from test_pond_curves_model import half_to_even_row, pyramid, pyramid_row
    R, Cc = case.R, case.Cc
    mids = [hi for hi in boundaries(slabs) if 17 <= hi and hi + 17 <= R]
    assert mids
    for hi in sorted({mids[0], mids[-1]}):
        for cx in (20, 64):                                # within one segment; across lanes 63 | 0
            for cy in (hi - 1, hi):                        # file row: the centre is the last row above the boundary, the first below
                t, s, _ = case.check(*pyramid(R, Cc, cy, cx)[::-1])
                cells, q = pyramid_row()
                assert len(t) == 1 and (t["bed_level"][0], t["top_level"][0]) == (0.0, 16.0)
                assert t["cells"][0].tolist() == cells and t["q"][0].tolist() == q
                assert plain(s, ("merge_ms", "ranks")) == dict(ponds=1, no_curve=0, flat=0, stage_cells=961, split_basins=1, remote_beds=1), s
        levels, depths = half_to_even_row()
        for start, step in both_ways(hi):
            (t, s, basin), rows = column(case, 64, start - step, step, levels, depths)      # pond, 2 - 3e || 2 - e, 2, 1.5
            k = basin[rows[0], 64]
            assert t["top_level"][k - 1] == 2.0 and t["cells"][k - 1].tolist() == [1] * 15 + [3] and t["q"][k - 1][15] == Q + 2, t[k - 1]


# ---- curves that are none ------------------------------------------------------------------------------------------------------
def run_degenerate(case, slabs):
    """P == Z and P one ulp above Z with the pond on one side of a boundary and the land it spills to on the other; a -0.0 bed in
    another rank than the rest of its pond"""
    up = float(np.nextafter(5.0, 6.0))
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in (63, 64):
            for start, step in both_ways(hi):
                (t, s, _), rows = column(case, c, start, step, [1024.0, 1000.0], [2.0 ** -60, 0.0], thresholds=(0.0,))
                assert len(t) == 1 and t["bed_level"][0] == t["top_level"][0] == 1024.0 and not t["cells"].any() and not t["q"].any()
                assert plain(s, ("merge_ms", "ranks", "split_basins", "remote_beds")) == dict(ponds=1, no_curve=0, flat=1, stage_cells=0), s
                (t, s, _), rows = column(case, c, start, step, [5.0, up, 4.0, 4.5], [2.0 ** -60, 0, 0, 0], thresholds=(0.0,))
                assert (t["bed_level"][0], t["top_level"][0]) == (5.0, up) and t["cells"][0].tolist() == [0] * 8 + [1] * 8 and not t["q"].any()
                (t, s, _), rows = column(case, c, start, step, [-0.0, 0.0, 0.0, 1.0, 0.5, 0.75], [0.25, 0.25, 0.25, 0, 0, 0])
                assert np.signbit(t["bed_level"][0]) and t["bed_level"][0] == 0.0 and t["top_level"][0] == 1.0
                assert t["cells"][0][15] == 3 and t["q"][0][15] == 3 * Q
                if case.n > 1:
                    assert s["split_basins"] == 1 and s["remote_beds"] == 1, s


def run_no_outlet(case, slabs):
    """tests/test_pond_curves.test_no_outlet: one basin over all ranks; two bowls walled in by NODATA; no pond at all.  Then all of
    one rank's rows one pond and nothing else, which spills into a pit in the row beyond (tests/group_pond_outlets_cases
    .run_not_quiet)"""
    from test_pond_curves import bowl
    R, Cc = case.R, case.Cc
    t, s, basin = case.check(*bowl(R, Cc)[::-1])
    assert (basin[1:-1, 1:-1] == 1).all() and np.isposinf(t["top_level"][0]) and t["bed_level"][0] == 50.0
    assert not t["cells"].any() and not t["q"].any()
    assert plain(s, ("merge_ms", "ranks")) == dict(ponds=1, no_curve=1, flat=0, stage_cells=0, split_basins=int(case.n > 1), remote_beds=0), s
    dem, water = bowl(R, Cc)
    r, c = np.mgrid[1:R + 1, 1:Cc + 1]
    wall = Cc // 3
    d2 = (r - R // 2) ** 2 + (c - 5) ** 2
    dem = np.where(c < wall, 40.0 + d2 / 64.0, dem)
    water = np.where(c < wall, np.where(d2 <= 2, 0.01, 0.0), water)
    dem[:, wall - 1] = MISS
    t, s, _ = case.check(water, dem)
    assert len(t) == 2 and s["no_curve"] == 2 and sorted(t["bed_level"].tolist()) == [40.0, 50.0] and not t["cells"].any()
    t, s, _ = case.check(np.zeros((R, Cc)), dem)
    assert len(t) == 0 and plain(s, ("merge_ms", "ranks")) == dict(ponds=0, no_curve=0, flat=0, stage_cells=0, split_basins=0, remote_beds=0)
    assert len(case.ponds.stage_curves(capacity=0)) == 0
    if case.n > 1:
        own = slabs[1]
        dem, w, cell = empty(R, Cc)
        rows = range(max(own.own_lo, 1), min(own.own_hi, R) + 1)
        for rr in rows:
            dem[rr - 1, :], w[rr - 1, :] = 10.0, 0.5
        cell(own.own_lo - 1, 64, 5.0)
        t, s, basin = case.check(w, dem)
        assert len(t) == 1 and basin[own.own_lo - 1, 64] == 0 and (t["bed_level"][0], t["top_level"][0]) == (10.0, 10.5)
        assert t["cells"][0].tolist() == [len(rows) * Cc] * STAGES and s["split_basins"] == 0, (t, s)


def run_beside(case, slabs):
    """tests/test_pond_curves.test_basin_0_and_nodata_beside_a_basin with the cone's bed on a boundary: a dry pit (basin 0) on one
    side, a NODATA wall on the other; neither is counted"""
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        dem, water, _ = cones(case.R, case.Cc, [(hi, 62)], radius=4)
        dem[hi - 3:hi + 3, 66] = MISS                                         # padded column 67, the column beside the cone, is a wall
        dem[hi - 1, 54] = 800.0                                               # a dry pit two cells from the cone's foot
        t, s, basin = case.check(water, dem)
        assert len(t) == 1 and (basin == 0).sum() > 0 and (basin[hi - 2:hi + 4, 67] == -1).all()
        assert 25 <= t["cells"][0][15] <= (basin == 1).sum()


# ---- denser inputs -------------------------------------------------------------------------------------------------------------
def run_films(case):
    """tests/test_pond_curves.test_films_and_nan_water_in_the_basins"""
    from helpers import rough_dem
    R, Cc = case.R, case.Cc
    rng = np.random.default_rng(R)
    dem = rough_dem(R, Cc, R, step=0.25)
    water = np.where(dem < np.quantile(dem, 0.2), 0.3, 0.0)
    film = (water == 0) & (rng.random((R, Cc)) < 0.3)
    water[film] = rng.random(int(film.sum())) * WET
    water[rng.random((R, Cc)) < 0.01] = np.nan
    water[rng.random((R, Cc)) < 0.01] = -0.5
    t, s, _ = case.check(water, dem, thresholds=(WET, 0.0))
    assert len(t) > 3 and s["stage_cells"] > 0


def run_noise(case, densities=(0.30, 0.41, 0.60), thresholds=(WET, 0.01)):
    """tests/test_pond_curves.test_noise, at two thresholds on one handle"""
    from helpers import rough_dem
    R, Cc = case.R, case.Cc
    for density in densities:
        rng = np.random.default_rng(int(density * 100))
        dem = rough_dem(R, Cc, int(density * 100))
        depth = 0.002 + rng.random((R, Cc)) * 0.02
        depth[rng.random((R, Cc)) < 0.10] = 3.0
        water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
        dem[rng.random((R, Cc)) < 0.03] = MISS
        t, s, _ = case.check(water, dem, thresholds=thresholds)
        assert len(t) > 10 and s["no_curve"] < len(t)
        if case.n > 1:
            assert s["split_basins"] > 0, s


def run_smooth_bowls(case):
    from test_pond_curves import smooth_bowls
    dem, water = smooth_bowls()
    t, s, _ = case.check(water, dem)
    assert len(t) >= 20 and s["stage_cells"] > 10000
    assert s["split_basins"] > 0 and s["remote_beds"] > 0, s
