"""The pond stage curves on the device (include/wdpm_pond_curves.h, wdpm_amd/csrc/wdpm_pond_curves.hip) against the host model
(tests/pond_curves_model.py, itself held against hand-written answers and a plain double loop in tests/test_pond_curves_model.py).

Every case compares the WHOLE curve table and the counts for equality - integers by value, doubles by bit pattern; the definitions
are exact, there is no tolerance; holds labels, pond table, rim table, basin raster, catchment table and outlet table of the same
call, bit for bit, against a label_outlets() of a twin context; asserts what the header states of every call (stage heights that
never fall and never pass the top, counts and sums that never fall, cells[15] >= fill_cells and q[15] >= fill_q); and asserts that
no guard byte around the handle's buffers changed.  Shapes are file cells: 46 x 70 is two segments, 67 x 193 one block row of four,
131 x 385 seven segments over two blocks; a wave owns a 64-column segment, so padded column 63 is lane 63 and padded column 64 lane 0
of the next.
"""
import hashlib

import numpy as np
import pytest

from helpers import find_drain, n_bit_diff, pad, rough_dem
from pond_catchments_model import catchments
from pond_curves_model import STAGES, TooDeep, assert_invariants, assert_same_curves, curves
from pond_outlets_model import outlets
from pond_rims_model import device_dem
from ponds_model import inventory
from test_pond_curves_model import half_to_even_row, pyramid, pyramid_row

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001
THRES = 0.005 / 1000
SHAPES = [(46, 70), (67, 193), (131, 385)]
Q = 2 ** 24
_REFERENCES = {}


def reference(bd, miss, water, md):
    """(basin raster, outlet table, curve table, curve stats) of the model, or the TooDeep it raised: computed once per water"""
    key = hashlib.sha1(bd.tobytes() + np.ascontiguousarray(water).tobytes() + repr((bd.shape, miss, md)).encode()).hexdigest()
    if key not in _REFERENCES:
        labels, ponds = inventory(bd > miss, water, md)
        dem = device_dem(bd, miss)
        basin, _, _ = catchments(labels, dem, water, ponds)
        out, _ = outlets(labels, dem, water, ponds, basin=basin)
        try:
            _REFERENCES[key] = (basin, out) + curves(basin, dem, out)
        except TooDeep as e:
            _REFERENCES[key] = e
    return _REFERENCES[key]


def older(p):
    """what a label_outlets() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.outlets()


def hold_against_model(bd, miss, water, md, p, n):
    """the curve table and its counts of handle p against the model of the same water; returns (table, stats, basins)"""
    table, stats, basins, out = p.curves(), p.curve_stats(), p.basins(), p.outlets()
    ref_basin, ref_out, ref_table, ref_stats = reference(bd, miss, water, md)
    assert n == len(ref_table) == stats["ponds"] == len(table)
    assert (basins == ref_basin).all() and out["pour_level"].view(np.uint64).tolist() == ref_out["pour_level"].view(np.uint64).tolist()
    assert_same_curves(table, stats, ref_table, ref_stats)
    assert_invariants(table, out)
    return table, stats, basins


def curves_on_device(hip, bd, bw, thresholds=(WET,), rows_per_wave=None):
    """Upload padded rasters, label with curves at each threshold on ONE handle, hold the curve table against the model and
    everything else the call leaves against the label_outlets() of a twin context.  Returns what the last threshold left."""
    from wdpm_amd.ponds import CURVE_DTYPE, Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    kw = dict(module="add", nrows=R, ncols=Cc, missingvalue=MISS)
    with hip.context(**kw) as ctx, hip.context(**kw) as twin:
        ctx.upload(bd, bw)
        twin.upload(bd, bw)
        with Ponds(ctx) as p, Ponds(twin) as q:
            for md in thresholds:
                n = p.label_curves(md)
                assert p.curves().dtype == CURVE_DTYPE
                got = hold_against_model(bd, MISS, ctx.download_water(), md, p, n)
                assert q.label_outlets(md) == n
                for mine, theirs in zip(older(p), older(q)):
                    assert mine.tobytes() == theirs.tobytes()
                assert p.catchment_stats() == q.catchment_stats() and p.outlet_stats() == q.outlet_stats()
                if rows_per_wave is not None:
                    assert p.stats()["rows_per_wave"] == rows_per_wave, p.stats()
            assert p.guard_bad() == 0
    return got


def check(hip, dem, water, **kw):
    return curves_on_device(hip, *pad(np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(water, dtype=np.float64)),
                                      MISS), **kw)


def grid(R, Cc):
    """padded row and column of every file cell"""
    return np.mgrid[1:R + 1, 1:Cc + 1]


# ---- the bed: where it lies in the wave and in the strip --------------------------------------------------------------------------
def cones_scene(R, Cc, spots, radius=4):
    """A plateau at 1000 m that falls slowly towards the last column, with one cone-shaped pit per spot (padded row, padded column):
    the ground rises by 1/4 m per step of Chebyshev distance from a bed of its own height about 1.3 m below the plateau, and the bed
    cell holds 0.2 m of water.  The plateau to the left of a pit drains into it, so every basin is a band across the segments, and it
    spills over the plateau.  Returns file rasters and the bed heights."""
    r, c = grid(R, Cc)
    dem = 1000.0 - c / 1024.0
    water = np.zeros((R, Cc))
    beds = []
    for i, (pr, pc) in enumerate(spots):
        d = np.maximum(abs(r - pr), abs(c - pc))
        bed = 998.5 + i / 16.0
        dem = np.where(d <= radius, bed + d * 0.25, dem)
        water[pr - 1, pc - 1] = 0.2
        beds.append(bed)
    return dem, water, beds


def check_cones(hip, R, Cc, spots, **kw):
    dem, water, beds = cones_scene(R, Cc, spots)
    table, stats, basins = check(hip, dem, water, **kw)
    assert len(table) == len(spots) and stats["no_curve"] == 0 and stats["flat"] == 0
    for (pr, pc), bed in zip(spots, beds):
        k = basins[pr, pc]
        assert k > 0 and table["bed_level"][k - 1] == bed and table["top_level"][k - 1] > bed
        assert table["cells"][k - 1][0] >= 1 and len(set(table["cells"][k - 1].tolist())) >= 4
    return table


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_bed_cells_at_lane_and_raster_edges(hip, R, Cc):
    """the bed cell on lane 0 and lane 63 (padded columns 64 and 63), on padded columns 1 and ncp - 2, on padded rows 1 and rows - 2"""
    spots = [(R // 2, 63), (R // 2, 1), (R // 2 + 12, Cc), (1, 20), (R, 30), (R // 2 - 12, 64)]
    if Cc > 70:
        spots += [(R // 2 + 12, 127), (R // 2 + 12, 140)]
    check_cones(hip, R, Cc, spots)


@pytest.mark.parametrize("rpw", [1, 2, 3, 64])
def test_basins_across_strip_seams_and_lanes_63_0(hip, monkeypatch, rpw):
    """basins nine rows high on every residue of the strip height, one of them across lanes 63 | 0, with every row, every second and
    every third row the first of a strip; 64 rows: one strip and a short one"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    check_cones(hip, 67, 193, [(10, 64), (21, 30), (32, 100), (43, 127), (54, 160), (60, 10)], rows_per_wave=rpw)


def test_equal_minima_and_a_negative_zero_bed(hip):
    """two cells at the lowest height; and a -0.0 bed among +0.0 cells: -0.0 lies below +0.0, and a term of +0.0 - -0.0 is nothing"""
    t, s, _ = check(hip, [1.0, 1.0, 3.0, 2.0, 2.5], [0.5, 0.5, 0, 0, 0])
    assert t["bed_level"][0] == 1.0 and t["top_level"][0] == 3.0 and t["cells"][0][15] == 2 and t["q"][0][15] == 4 * Q
    t, s, _ = check(hip, [0.0, -0.0, 0.0, 1.0, 0.5, 0.75], [0.25, 0.25, 0.25, 0, 0, 0])
    assert np.signbit(t["bed_level"][0]) and t["bed_level"][0] == 0.0 and t["top_level"][0] == 1.0
    assert t["cells"][0][15] == 3 and t["q"][0][15] == 3 * Q
    rng = np.random.default_rng(3)
    dem = np.where(rng.random((46, 70)) < 0.5, 0.0, -0.0)
    water = np.where(rng.random((46, 70)) < 0.05, 0.4, 0.0)
    dem[water > 0] = np.where(rng.random(int((water > 0).sum())) < 0.5, -5.0, -5.5)
    t, s, _ = check(hip, dem, water)
    assert len(t) > 5 and set(np.unique(t["bed_level"])) <= {-5.0, -5.5}


@pytest.mark.parametrize("rpw", [1, 2, 3])
def test_a_lane_whose_basin_changes_row_by_row(hip, monkeypatch, rpw):
    """Every odd row is a perched pond of its own, level at 300 m + its number over a wavy bed; every even row a valley 100 m lower
    that falls to a pit in the last column (basin 0).  Every row with a basin brings every lane another basin: bed and top are
    reloaded each time, and every basin is sent before the next."""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    R, Cc = 46, 70
    r, c = grid(R, Cc)
    k = (r + 1) // 2
    pond = r % 2 == 1
    dem = np.where(pond, 299.75 + k - (c % 8) / 64.0, 200.0 - c / 256.0)
    water = np.where(pond, 300.0 + k - dem, 0.0)
    t, s, basins = check(hip, dem, water, rows_per_wave=rpw)
    assert len(t) == 23 and s == dict(ponds=23, no_curve=0, flat=0, stage_cells=23 * Cc)
    assert t["top_level"].tolist() == [300.0 + i for i in range(1, 24)] and (t["top_level"] - t["bed_level"] == 0.25 + 7 / 64.0).all()
    assert all(len(set(row.tolist())) == 5 for row in t["cells"]) and (basins[2:-1:2, 1:-1] == 0).all()


# ---- the stage rules: the hand-written answers of tests/test_pond_curves_model.py ---------------------------------------------------
@pytest.mark.parametrize("at", [(3, 3), (5, 44), (27, 150)], ids=lambda a: "r%dc%d" % a)
def test_a_stepped_pyramid_computed_by_hand(hip, at):
    """integer ground, Z = 0, P = 16 and h_s = s: a cell at exactly h_s is not counted at s and is counted at s + 1; the bowl within one
    segment, across lanes 63 | 0 and across three segments' seams"""
    R, Cc = 67, 193
    dem, water = pyramid(R, Cc, at[0] + 16, at[1] + 16)
    t, s, _ = check(hip, dem, water)
    cells, q = pyramid_row()
    assert len(t) == 1 and t["bed_level"][0] == 0.0 and t["top_level"][0] == 16.0
    assert t["cells"][0].tolist() == cells and t["q"][0].tolist() == q and s == dict(ponds=1, no_curve=0, flat=0, stage_cells=961)


def test_half_to_even(hip):
    t, s, _ = check(hip, *half_to_even_row())
    assert t["top_level"][0] == 2.0 and t["cells"][0].tolist() == [1] * 15 + [3] and t["q"][0][15] == Q + 2


def test_top_one_ulp_above_the_bed_and_top_at_the_bed(hip):
    up = np.nextafter(5.0, 6.0)
    t, s, _ = check(hip, [5.0, up, 4.0, 4.5], [2.0 ** -60, 0, 0, 0], thresholds=(0.0,))
    assert t["bed_level"][0] == 5.0 and t["top_level"][0] == up and t["cells"][0].tolist() == [0] * 8 + [1] * 8 and not t["q"].any()
    t, s, _ = check(hip, [1024.0, 1000.0], [2.0 ** -60, 0.0], thresholds=(0.0,))
    assert t["bed_level"][0] == t["top_level"][0] == 1024.0 and not t["cells"].any() and s == dict(ponds=1, no_curve=0, flat=1, stage_cells=0)


def bowl(R, Cc):
    r, c = grid(R, Cc)
    d2 = (r - R // 2) ** 2 + (c - Cc // 2) ** 2
    return 50.0 + d2 / 64.0, np.where(d2 <= 9, 0.01, 0.0)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_no_outlet(hip, monkeypatch, R, Cc):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    t, s, basins = check(hip, *bowl(R, Cc), rows_per_wave=16)             # one basin over everything
    assert (basins[1:-1, 1:-1] == 1).all() and np.isposinf(t["top_level"][0]) and t["bed_level"][0] == 50.0
    assert not t["cells"].any() and not t["q"].any() and s == dict(ponds=1, no_curve=1, flat=0, stage_cells=0)
    # two bowls with a NODATA ridge between them, each walled in by it and the border
    dem, water = bowl(R, Cc)
    r, c = grid(R, Cc)
    wall = Cc // 3
    d2 = (r - R // 2) ** 2 + (c - 5) ** 2
    dem = np.where(c < wall, 40.0 + d2 / 64.0, dem)
    water = np.where(c < wall, np.where(d2 <= 2, 0.01, 0.0), water)
    dem[:, wall - 1] = MISS
    t, s, basins = check(hip, dem, water, rows_per_wave=16)
    assert len(t) == 2 and s["no_curve"] == 2 and sorted(t["bed_level"].tolist()) == [40.0, 50.0] and not t["cells"].any()
    t, s, _ = check(hip, dem, np.zeros((R, Cc)))                          # no pond at all: an empty table
    assert len(t) == 0 and s == dict(ponds=0, no_curve=0, flat=0, stage_cells=0)


def test_basin_0_and_nodata_beside_a_basin(hip):
    """a cone whose neighbours are a dry pit (basin 0) on one side and NODATA cells on the other: neither is counted"""
    R, Cc = 46, 70
    dem, water, _ = cones_scene(R, Cc, [(20, 62)])
    dem[17:23, 66] = MISS                                                 # padded column 67, the column beside the cone, is a wall
    dem[19, 54] = 800.0                                                   # a dry pit two cells from the cone's foot
    t, s, basins = check(hip, dem, water)
    assert len(t) == 1 and (basins == 0).sum() > 0 and (basins[18:24, 67] == -1).all()
    inside = basins == 1
    assert t["cells"][0][15] <= inside.sum() and t["cells"][0][15] >= 49


# ---- films, NaN water, depths the sums cannot hold -----------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
def test_films_and_nan_water_in_the_basins(hip, R, Cc):
    rng = np.random.default_rng(R)
    dem = rough_dem(R, Cc, R, step=0.25)
    water = np.where(dem < np.quantile(dem, 0.2), 0.3, 0.0)
    film = (water == 0) & (rng.random((R, Cc)) < 0.3)
    water[film] = rng.random(int(film.sum())) * WET            # at most the threshold: slope cells at WET, pond cells at 0
    water[rng.random((R, Cc)) < 0.01] = np.nan
    water[rng.random((R, Cc)) < 0.01] = -0.5
    t, s, _ = check(hip, dem, water, thresholds=(WET, 0.0))
    assert len(t) > 3 and s["stage_cells"] > 0


def test_a_600_m_pit_fails_and_the_handle_stays_usable(hip):
    """A pit whose floor lies 600 m below the only way out of its walls, with 500 m of water in it: the water stands 100 m below the
    outlet, so label_outlets() has nothing to say, and the floor 600 m below the last stage, which q cannot hold.  (A cell with
    512 m of water or more would already fail the pond table.)"""
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    R, Cc = 46, 70
    dem, water, _ = cones_scene(R, Cc, [(10, 20), (30, 50)])
    ok_d, ok_w = pad(dem, water, MISS)
    deep = dem.copy()
    deep[29:32, 39:45] = 1700.0                                  # walls
    deep[30, 40:43] = [1000.0, 1600.0, 1001.0]                  # the floor, the way out, lower land beyond it
    pit_w = water.copy()
    pit_w[30, 40] = 500.0
    bd, bw = pad(deep, pit_w, MISS)
    assert isinstance(reference(bd, MISS, bw, WET), TooDeep)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            n = p.label_outlets(WET)                             # the lesser call succeeds
            assert n == 3 and 1600.0 in p.outlets()["pour_level"].tolist()
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_curves_label.*512 m"):
                p.label_curves(WET)
            p.n = n
            for ask in (p.curves, p.curve_stats):
                with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
                    ask()
            for ask in (p.table, p.outlets):                     # no table of any kind
                with pytest.raises(wdpm_amd.WdpmError):
                    ask()
            assert p.label_outlets(WET) == n and len(p.outlets()) == n
            ctx.upload(ok_d, ok_w)                               # and the handle labels another water as if nothing had happened
            n = p.label_curves(WET)
            hold_against_model(ok_d, MISS, ok_w, WET, p, n)
            assert p.guard_bad() == 0


# ---- noise, and basins large enough for the bulk path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, density):
    """water at three densities on rough ground, 3 % NODATA with water on it, at two thresholds on one handle: basins of a cell or
    two, every label change a send"""
    R, Cc = 131, 385
    rng = np.random.default_rng(int(density * 100))
    dem = rough_dem(R, Cc, int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    t, s, _ = check(hip, dem, water, thresholds=(WET, 0.01))
    assert len(t) > 10 and s["no_curve"] < len(t)


def smooth_bowls():
    """round(500 + 3 sin(x / 9) cos(y / 8) + 0.002 x + 0.01 U, 4) at 131 x 385 with water up to 497.6 m: some thirty basins of about
    a thousand cells, each with sixteen distinct stage counts, several across a segment boundary"""
    R, Cc = 131, 385
    y, x = np.mgrid[0:R, 0:Cc]
    u = np.random.default_rng(18).random((R, Cc))
    dem = np.round(500.0 + 3.0 * np.sin(x / 9.0) * np.cos(y / 8.0) + 0.002 * x + 0.01 * u, 4)
    return dem, np.maximum(497.6 - dem, 0.0)


@pytest.mark.parametrize("rpw", [0, 1, 2, 3])
def test_smooth_bowls(hip, monkeypatch, rpw):
    """the bulk path: large basins over many rows and strips, with the library's strips and with 1, 2 and 3 rows per wave"""
    if rpw:
        monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    else:
        monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    dem, water = smooth_bowls()
    bd, bw = pad(dem, water, MISS)
    basin, out, ref, _ = reference(bd, MISS, bw, WET)
    big = [k for k in range(len(ref)) if (basin == k + 1).sum() >= 1000 and len(set(ref["cells"][k].tolist())) == STAGES]
    assert big, "the recipe must leave a basin of 1000 cells with sixteen distinct stage counts"
    ncp = bd.shape[1]
    cols = [np.flatnonzero((basin == k + 1).any(axis=0)) for k in big]
    assert any(c.min() // 64 != c.max() // 64 for c in cols) and ncp > 64
    t, s, _ = curves_on_device(hip, bd, bw, rows_per_wave=rpw or None)
    assert len(t) >= 20 and s["stage_cells"] > 10000


def noise_case():
    rng = np.random.default_rng(8)
    dem = rough_dem(131, 385, 8, step=0.125)
    water = np.where(rng.random((131, 385)) < 0.41, 0.002 + rng.random((131, 385)), 0.0)
    dem[rng.random((131, 385)) < 0.03] = MISS
    return dem, water


@pytest.mark.parametrize("rpw", [1, 2, 3, 64])
def test_noise_with_rows_per_wave_forced(hip, monkeypatch, rpw):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    check(hip, *noise_case(), rows_per_wave=rpw)


@pytest.mark.parametrize("R,Cc", [(1, 1), (131, 1), (3, 700), (1, 200)])
def test_thin_rasters(hip, R, Cc):
    rng = np.random.default_rng(R * Cc)
    dem = rough_dem(R, Cc, R + Cc, step=0.25)
    t, s, _ = check(hip, dem, np.zeros((R, Cc)))                                    # no pond
    assert len(t) == 0
    t, s, _ = check(hip, dem, np.full((R, Cc), 0.5))                                # all pond
    assert len(t) == 1 and np.isposinf(t["top_level"][0])
    if R * Cc > 1:
        check(hip, dem, np.where(rng.random((R, Cc)) < 0.3, 0.3, 0.0), thresholds=(WET, 0.25))


# ---- the handle -----------------------------------------------------------------------------------------------------------------------
def test_handle_state(hip):
    import wdpm_amd
    from wdpm_amd.ponds import CURVE_DTYPE, Ponds, bind
    R, Cc = 46, 70
    dem = rough_dem(R, Cc, 5)
    water = np.where(np.random.default_rng(5).random((R, Cc)) < 0.3, 0.3, 0.0)
    bd, bw = pad(dem, water, MISS)
    dll = bind(hip)
    none = dict(ponds=0, no_curve=0, flat=0, stage_cells=0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="Ponds.curves: label_curves\\(\\) has not succeeded"):
                p.curves()
            with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):             # nothing labelled yet
                p.n = 0
                p.curves(capacity=10)
            n = p.label_curves(WET)
            want, stats, _ = hold_against_model(bd, MISS, bw, WET, p, n)
            assert n >= 4
            for call in (p.label, p.label_rims, p.label_catchments, p.label_outlets):
                assert call(WET) == n                                                   # each lesser label call takes the table away
                for ask in (p.curves, p.curve_stats):
                    with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
                        ask()
                assert p.label_curves(WET) == n and p.curves().tobytes() == want.tobytes() and p.curve_stats() == stats
            buf = np.full(n * CURVE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_curves_table(p._h, buf.ctypes.data, n - 1) != 0             # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_curves_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                                  # ... and writes nothing
            assert dll.wdpm_curves_table(p._h, buf.ctypes.data, n) == 0
            assert buf.tobytes() == want.tobytes() and p.curves(capacity=n + 7).tobytes() == want.tobytes()
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_curves_label"):
                p.label_curves(float("nan"))
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_curves_label"):
                p.label_curves(-1.0)
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.curve_phase_ms()
            assert p.label_curves(5.0) == 0                                             # no pond at this threshold: an empty table
            assert len(p.curves()) == 0 and p.curve_stats() == none
            assert p.label_curves(WET) == n and p.curves().tobytes() == want.tobytes()
            ctx.run_block(1, THRES)                                                     # the water moves on: a label call of the new
            assert p.label_outlets(WET) >= 0                                            # water leaves no curve table either
            with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
                p.curves()
            n2 = p.label_curves(WET)
            hold_against_model(bd, MISS, ctx.download_water(), WET, p, n2)
            assert p.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import CURVE_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    dem, water = smooth_bowls()
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=131, ncols=385, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            p.label_curves(WET)
            ms = p.curve_phase_ms()
            assert tuple(ms) == CURVE_PHASES == ("bed", "stages") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.outlet_phase_ms()) == {"passes", "locate"} and len(p.phase_ms()) == 6


# ---- real water, and the context is left as it was ------------------------------------------------------------------------------------
def real_case(hip, module):
    dem = hip.synth_dem(385, 131)[:131, :385].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    kw = dict(module=module, nrows=131, ncols=385, missingvalue=MISS)
    if module == "drain":
        dr, dc = find_drain(bd)
        kw.update(drainrow=dr, draincol=dc)
    return bd, bw, kw


@pytest.mark.parametrize("module", ["add", "drain"])
def test_real_water_and_state_neutrality(hip, module):
    """Two blocks of real iterations; curves (the owed drain() of the drain module applied by the call) against the model; a third
    block with another curve call between begin_block and its first iteration.  The third block is, bit for bit, what a twin
    context computes that never took an inventory."""
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    bd, bw, kw = real_case(hip, module)
    with hip.context(**kw) as a, hip.context(**kw) as b:
        for c in (a, b):
            c.upload(bd, bw)
            c.totaldrain = 0.0
            c.run_block(100, THRES)
            c.run_block(100, THRES)
        with Ponds(a) as p:
            n = p.label_curves(WET)
            t, s, _ = hold_against_model(bd, MISS, a.download_water(), WET, p, n)
            assert n >= 1 and s["stage_cells"] > 0
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label_curves(0.0)
            flushed = a.download_water()
            a.iterate(100)
            md_a = a.max_diff()
            hold_against_model(bd, MISS, flushed, 0.0, p, n2)
            assert p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        assert md_a == md_b
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
        assert a.totaldrain == b.totaldrain
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0


def test_basin5(hip, basin5):
    """basin5 after an add of 300 mm and 300 iterations: the curve table against the model"""
    from wdpm_amd.ponds import Ponds
    dem, hdr = basin5
    miss = hdr["NODATA_value"] if "NODATA_value" in hdr else hdr[[k for k in hdr if k.lower().startswith("nodata")][0]]
    R, Cc = dem.shape
    bd, _ = pad(dem, np.zeros_like(dem), miss)
    bw = np.where(bd > miss, 0.3, 0.0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=miss) as ctx:
        ctx.upload(bd, bw)
        ctx.run_block(300, THRES)
        with Ponds(ctx) as p:
            n = p.label_curves(WET)
            t, s, _ = hold_against_model(bd, miss, ctx.download_water(), WET, p, n)
            assert n >= 1 and s["stage_cells"] > 0 and p.guard_bad() == 0
