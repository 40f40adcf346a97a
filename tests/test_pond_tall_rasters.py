"""The pond units past their size gates, on rasters that are tall and one to three columns wide.

Three things in the pond code are chosen by the number of SEGMENTS (64 columns of one padded row), and none of the other pond
suites has enough of them:

  * ponds_scan_sums_kernel scans the sums of the scan blocks (1024 segments each) in trips of 256 and carries the total from one
    trip to the next: a second trip wants more than 262 144 segments;
  * ponds_rows_per_wave gives every wave one row up to 32 768 segments and strips of several rows beyond; the other suites reach
    strips only by forcing them through WDPM_PONDS_ROWS_PER_WAVE, which every case here removes from the environment;
  * the catchments jump pointers in batches of four rounds: a descent of 400 000 cells is longer than two batches can halve away.

A raster of R x Cc file cells has (R + 2) * ceil((Cc + 2) / 64) segments, so 262 143 rows of one to three columns pass the gate
with under a million cells, which the numpy models walk in seconds.  Every case makes one label_outlets() call and holds each of
its five outputs against that output's own model - labels and pond table (ponds_model), rim table (pond_rims_model), basin raster,
catchment table and counts (pond_catchments_model), outlet table and counts (pond_outlets_model) - integers by value, doubles by
bit pattern, no guard byte changed; and asserts from stats() that the gate was passed: the segment count, and rows_per_wave ==
ceil(segments / 32768) > 1 with nothing forced.

With one segment per row the LAST segment is the border row below the raster, which holds no pond.  At 262 143 rows (262 145
segments, 257 scan blocks) that border row is the whole second trip: the trip runs, the leading barrier of block_exclusive_scan
with it, but no pond takes its number from the carry.  The ponds of "noise 300000x3", of the rows beyond 262 144 in the taller
"lattice" and "ends only" cases and of both ranks of the row-block cases do.

Chains of unions beyond 16 384 wet rows in one column are not run here: find_root has no path compression and how a longer chain
behaves is unmeasured.
"""
import numpy as np
import pytest

from helpers import pad, rough_dem
from pond_catchments_model import assert_same_catchments, catchments
from pond_outlets_model import assert_invariants, assert_same_outlets, outlets
from pond_rims_model import assert_same_rims, device_dem, rims
from ponds_model import assert_same, inventory

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001
TRIP = 256 * 1024        # segments one trip of ponds_scan_sums_kernel covers
TABLE_WAVES = 32768      # kTableWaves: the waves ponds_rows_per_wave aims at
ROUND_CAP = 40
NONE = (np.inf, -1, -1, -1, -1, -1, 0, 0, 0, 0)
TALL = 262143            # file rows: 262 145 padded rows
TALLER = 264191          # 264 193 padded rows: a whole scan block and one more segment beyond the first trip


def segments_of(R, Cc):
    return (R + 2) * -(-(Cc + 2) // 64)


def assert_gate_passed(stats, segments=None, boundary=False):
    """the segment count is past (or, for the boundary case, on) the scan's trip, and the strips are the library's own choice"""
    seg = stats["segments"]
    if segments is not None:
        assert seg == segments, stats
    assert seg == TRIP if boundary else seg > TRIP, stats
    assert stats["rows_per_wave"] == -(-seg // TABLE_WAVES) > 1, stats


def hold_against_models(bd, water, md, p, n):
    """everything a label_outlets() call left on handle p, each output against its own model of the same water"""
    from wdpm_amd.ponds import CATCH_DTYPE, OUTLET_DTYPE, RIM_DTYPE
    got = dict(labels=p.labels(), table=p.table(), rims=p.rims(), basins=p.basins(), catch=p.catchments(),
               catch_stats=p.catchment_stats(), outlets=p.outlets(), outlet_stats=p.outlet_stats())
    assert (got["rims"].dtype, got["catch"].dtype, got["outlets"].dtype) == (RIM_DTYPE, CATCH_DTYPE, OUTLET_DTYPE)
    ref_labels, ref_table = inventory(bd > MISS, water, md)
    assert n == len(ref_table) == p.stats()["ponds"] == got["catch_stats"]["ponds"] == got["outlet_stats"]["ponds"]
    assert_same(got["labels"], got["table"], ref_labels, ref_table)
    dem = device_dem(bd, MISS)
    assert_same_rims(got["rims"], rims(ref_labels, dem, water, n))
    ref_basin, ref_catch, ref_cstats = catchments(ref_labels, dem, water, ref_table)
    assert_same_catchments(got["basins"], got["catch"], got["catch_stats"], ref_basin, ref_catch, ref_cstats)
    assert 1 <= got["catch_stats"]["rounds"] <= ROUND_CAP
    assert_same_outlets(got["outlets"], got["outlet_stats"], *outlets(ref_labels, dem, water, ref_table, basin=ref_basin))
    assert_invariants(got["outlets"], got["rims"])
    got["ref_catch_stats"], got["ref_catch"] = ref_cstats, ref_catch
    return got


def tall(hip, monkeypatch, dem, water, thresholds=(WET,), boundary=False):
    """Upload, label with outlets at each threshold on ONE handle with nothing forced, hold everything against the models and
    assert the gates.  Returns what the last threshold left."""
    from wdpm_amd.ponds import Ponds
    monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    R, Cc = dem.shape
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            for md in thresholds:
                n = p.label_outlets(md)
                got = hold_against_models(bd, ctx.download_water(), md, p, n)
                assert_gate_passed(p.stats(), segments_of(R, Cc), boundary)
            assert p.guard_bad() == 0
    return got


def row(table, k):
    return tuple(table[k].tolist())


def last_pond_of_the_first_trip(table):
    """how many ponds begin in the segments of the first trip (one segment per padded row here)"""
    return int((table["first_row"] < TRIP).sum())


# ---- scenes (file layout) ----------------------------------------------------------------------------------------------------------
def noise_scene(R, Cc):
    """rough ground in steps of 1/8 m, water at density 0.41 - a few millimetres, some cells 3 m - and 3 % NODATA with water on it"""
    rng = np.random.default_rng(R + Cc)
    dem = rough_dem(R, Cc, R + Cc, step=0.125)
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.02] = 3.0
    water = np.where(rng.random((R, Cc)) < 0.41, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    return dem, water


def lattice_scene(R, Cc):
    """a pond of one cell, a metre deep in the ground, at every other row and column"""
    dem = rough_dem(R, Cc, 3, step=0.125)
    water = np.zeros((R, Cc))
    k = np.arange(((R + 1) // 2) * ((Cc + 1) // 2)).reshape((R + 1) // 2, (Cc + 1) // 2)
    water[::2, ::2] = 0.125 + (k % 64) * 2.0 ** -10
    dem[water > 0] -= 1.0
    return dem, water


def ends_scene(R, Cc):
    """one pond cell in the first row, a pond of five cells in the last two, stepped ground between"""
    dem = rough_dem(R, Cc, 5, step=0.125)
    water = np.zeros((R, Cc))
    water[0, 1] = 0.5
    water[R - 2, 0:3] = [0.25, 0.375, 0.5]
    water[R - 1, 0:2] = [0.625, 0.75]
    dem[water > 0] -= 1.0
    return dem, water


def tall_pond_scene(R, Cc, height=16384):
    """one trench two metres deep and `height` rows long in the middle column, its depth changing from row to row"""
    dem = rough_dem(R, Cc, 7, step=0.125)
    water = np.zeros((R, Cc))
    r0 = (R - height) // 2
    water[r0:r0 + height, Cc // 2] = 0.25 + (np.arange(height) % 97) * 2.0 ** -7
    dem[water > 0] -= 2.0
    return dem, water


def descent_scene(R):
    """One column that falls by 2^-10 m per row.  The last cell lies a further metre lower and holds a quarter of a metre: its
    surface is below the cell above it, which so has a receiver and is no pit."""
    dem = 1000.0 - np.arange(R)[:, None] * 2.0 ** -10
    water = np.zeros((R, 1))
    dem[R - 1, 0] -= 1.0
    water[R - 1, 0] = 0.25
    return dem, water


# ---- whole rasters -------------------------------------------------------------------------------------------------------------------
def test_noise_on_exactly_256_scan_blocks(hip, monkeypatch):
    """262 144 segments: the first trip of the scan is full and there is no second"""
    got = tall(hip, monkeypatch, *noise_scene(TALL - 1, 1), boundary=True)
    assert len(got["table"]) > 10000


def test_noise_on_257_scan_blocks(hip, monkeypatch):
    got = tall(hip, monkeypatch, *noise_scene(TALL, 1))
    assert len(got["table"]) > 10000


def test_noise_three_columns_two_thresholds(hip, monkeypatch):
    """300 000 x 3, then a second threshold on the same handle; thousands of ponds are numbered by the second trip"""
    got = tall(hip, monkeypatch, *noise_scene(300000, 3), thresholds=(WET, 0.01))
    n = len(got["table"])
    assert n > 10000 and n - last_pond_of_the_first_trip(got["table"]) > 1000
    assert got["outlet_stats"]["divide_cells"] > 0 and got["outlet_stats"]["no_outlet"] < n


@pytest.mark.parametrize("R,Cc", [(TALL, 3), (TALLER, 1)], ids=["262143x3", "264191x1"])
def test_lattice(hip, monkeypatch, R, Cc):
    """Every scan block holds roots, so every block sum counts.  At 262 143 rows the ponds end with the first trip; at 264 191 the
    last thousand take their numbers from the second trip and the carry."""
    got = tall(hip, monkeypatch, *lattice_scene(R, Cc))
    n = len(got["table"])
    assert n == ((R + 1) // 2) * ((Cc + 1) // 2) and (got["table"]["cells"] == 1).all()
    if R == TALL:
        assert n == 262144
    else:
        assert n - last_pond_of_the_first_trip(got["table"]) > 1000
    assert (got["table"]["first_row"] == np.repeat(np.arange(1, R + 1, 2), (Cc + 1) // 2)).all()


@pytest.mark.parametrize("R", [TALL, TALLER])
def test_ponds_at_both_ends_only(hip, monkeypatch, R):
    """Every block sum but the first and one of the last is zero.  At 264 191 rows pond 2 begins in the second trip of the scan:
    the block sum before it is nothing but the carry."""
    got = tall(hip, monkeypatch, *ends_scene(R, 3))
    t = got["table"]
    assert len(t) == 2 and t["cells"].tolist() == [1, 5]
    assert (t["first_row"][0], t["first_col"][0]) == (1, 2) and (t["first_row"][1], t["first_col"][1]) == (R - 1, 1)
    assert last_pond_of_the_first_trip(t) == (2 if R == TALL else 1)


def test_one_pond_down_16384_rows(hip, monkeypatch):
    """one label carried down some 1 800 strips of the library's own height, one table row that takes the atomics of all of them"""
    R, Cc, height = TALL, 3, 16384
    got = tall(hip, monkeypatch, *tall_pond_scene(R, Cc, height))
    t = got["table"]
    assert len(t) == 1 and t["cells"][0] == height and t["row_max"][0] - t["row_min"][0] + 1 == height
    assert t["col_min"][0] == t["col_max"][0] == 1 + Cc // 2
    assert got["rims"]["surface_min"][0] < got["rims"]["surface_max"][0]


def test_a_descent_of_400000_cells(hip, monkeypatch):
    """One chain over every cell.  A round of pointer jumping follows five links, so eight rounds shorten a chain 5^8 = 390 625
    times at the most unless a cell reads what another has just stored: two batches cannot be expected to end this one."""
    R = 400000
    got = tall(hip, monkeypatch, *descent_scene(R))
    ref = got["ref_catch_stats"]
    assert ref["unponded_cells"] == 0 and ref["slope_cells"] == R - 1 and int(got["ref_catch"]["catch_cells"][0]) == R - 1
    assert len(got["table"]) == 1 and got["catch"]["catch_cells"][0] == R - 1 and got["catch_stats"]["pit_cells"] == 0
    assert (got["basins"][1:-1, 1:-1] == 1).all()
    assert row(got["outlets"], 0) == NONE
    rounds = got["catch_stats"]["rounds"]
    assert rounds % 4 == 0 and 8 <= rounds <= ROUND_CAP, rounds


# ---- row blocks ----------------------------------------------------------------------------------------------------------------------
def assert_every_rank_past_the_gate(case):
    for i in range(case.n):
        assert_gate_passed(case.ponds.rank_stats(i))


def test_row_blocks_label(hip, monkeypatch):
    """540 000 x 1 on two ranks of one GPU: each rank's view has its own scan blocks, its own second trip and its own strips"""
    import group_ponds_cases as gc
    monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    R, Cc = 540000, 1
    with gc.GroupCase(hip, R, Cc, [0, 0]) as case:
        w, nodata = gc.noise(R, Cc, 0.41, 41)
        s = case.check(w, nodata)
        assert s["ponds"] > 10000 and s["local_ponds"] >= s["ponds"], s
        assert_every_rank_past_the_gate(case)


def test_row_blocks_label_rims(hip, monkeypatch):
    import group_pond_rims_cases as grc
    monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    R, Cc = 540000, 1
    with grc.RimCase(hip, R, Cc, [0, 0]) as case:
        w, nodata = grc.noise(R, Cc, 0.41, 41)
        _, t, s, rs = case.check(w, nodata=nodata)
        assert s["ponds"] > 10000 and (t["wall_cells"] > 0).any(), s
        assert_every_rank_past_the_gate(case)
