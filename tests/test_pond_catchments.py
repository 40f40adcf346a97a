"""The pond catchments on the device (include/wdpm_pond_catchments.h, wdpm_amd/csrc/wdpm_pond_catchments.hip) against the host model
(tests/pond_catchments_model.py, itself held against hand-written answers in tests/test_pond_catchments_model.py).

Every case compares the WHOLE basin raster, the WHOLE catchment table and the counts for equality - integers by value, doubles by
bit pattern; the definitions are exact, there is no tolerance - next to the label raster and the pond table of the same call;
holds the rim table of the call, bit for bit, against a label_rims() of a twin context; asserts the identity
sum(pond cells) + sum(catch_cells) + unponded_cells == cells with a level; and asserts that no guard byte around the handle's
buffers changed.  Shapes are file cells: 46 x 70 is two segments, 67 x 193 one block row of four, 131 x 385 seven segments over
two blocks; a wave owns a 64-column segment, so padded column 63 is lane 63 and padded column 64 lane 0 of the next.
"""
import numpy as np
import pytest

from helpers import find_drain, n_bit_diff, pad, rough_dem
from pond_catchments_model import assert_same_catchments, catchments, descent_length
from pond_rims_model import device_dem
from ponds_model import assert_same, inventory

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001
THRES = 0.005 / 1000
SHAPES = [(46, 70), (67, 193), (131, 385)]
ROUND_CAP = 40


def taken(p):
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.catchment_stats()


def hold_against_model(bd, miss, water, md, got, n):
    labels, table, _, basin, catch, stats = got
    ref_labels, ref_table = inventory(bd > miss, water, md)
    assert n == len(ref_table) == stats["ponds"]
    assert_same(labels, table, ref_labels, ref_table)
    dem = device_dem(bd, miss)
    ref = catchments(ref_labels, dem, water, ref_table)
    assert_same_catchments(basin, catch, stats, *ref)
    assert int(table["cells"].sum()) + int(catch["catch_cells"].sum()) + stats["unponded_cells"] == int((dem < np.inf).sum())
    assert stats["slope_cells"] == int(catch["catch_cells"].sum()) + stats["unponded_cells"]
    assert 1 <= stats["rounds"] <= ROUND_CAP
    return ref_labels, dem


def catch_on_device(hip, bd, bw, thresholds=(WET,), rows_per_wave=None):
    """Upload padded rasters, label with catchments at each threshold on ONE handle, hold everything the call leaves against the
    models and its rim table against the label_rims() of a twin context.  Returns what the last threshold left."""
    from wdpm_amd.ponds import CATCH_DTYPE, Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    kw = dict(module="add", nrows=R, ncols=Cc, missingvalue=MISS)
    with hip.context(**kw) as ctx, hip.context(**kw) as twin:
        ctx.upload(bd, bw)
        twin.upload(bd, bw)
        with Ponds(ctx) as p, Ponds(twin) as q:
            for md in thresholds:
                n = p.label_catchments(md)
                got = taken(p)
                assert got[4].dtype == CATCH_DTYPE
                hold_against_model(bd, MISS, ctx.download_water(), md, got, n)
                assert q.label_rims(md) == n
                assert got[2].tobytes() == q.rims().tobytes() and got[1].tobytes() == q.table().tobytes()
                if rows_per_wave is not None:
                    assert p.stats()["rows_per_wave"] == rows_per_wave, p.stats()
            assert p.guard_bad() == 0
    return got


def check(hip, dem, water, **kw):
    return catch_on_device(hip, *pad(dem, water, MISS), **kw)


def grid(R, Cc):
    """padded row and column of every file cell"""
    return np.mgrid[1:R + 1, 1:Cc + 1]


# ---- ramps: every receiver that comes from memory and not from a lane -----------------------------------------------------------
DIRECTIONS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("dr,dc", DIRECTIONS)
def test_ramps_in_the_eight_directions(hip, monkeypatch, R, Cc, dr, dc):
    """A plane that falls half a metre per cell towards one of the eight neighbours, the two lowest lines under water: every
    descent runs across lanes 0 / 63, columns 1 / ncp - 2, rows 1 / rows - 2 and the boundaries of the 16-row strips, and on the
    straight directions three neighbours tie, so that the smallest index decides all the way down."""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    r, c = grid(R, Cc)
    down = dr * r + dc * c
    dem = 1000.0 - 0.5 * down
    water = np.where(down >= down.max() - 1, 0.3, 0.0)
    labels, table, _, basin, catch, stats = check(hip, dem, water, rows_per_wave=16)
    assert stats["pit_cells"] == 0 and stats["unponded_cells"] == 0 and int(catch["catch_cells"].sum()) == R * Cc - int(table["cells"].sum())
    assert (basin[1:-1, 1:-1] > 0).all()


# ---- ridges on every seam ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("side", [0, 1])
def test_ridges_on_every_seam(hip, monkeypatch, R, Cc, side):
    """Ridges along lane 0 (side 0) or lane 63 (side 1) of every segment and along the first or last row of every 16-row strip, the
    land falling a quarter of a metre per ring away from them into one pond per cell of the lattice: a ridge cell sees the same
    level on both sides and goes to the smaller index, and the rings are flat, so ties decide everywhere."""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    r, c = grid(R, Cc)
    dcol = np.minimum((c + side) % 64, 64 - (c + side) % 64)
    drow = np.minimum((r + side) % 16, 16 - (r + side) % 16)
    d = np.minimum(dcol, drow)
    dem = 100.0 - 0.25 * d
    water = np.where(d >= 6, 0.1, 0.0)
    labels, table, _, basin, catch, stats = check(hip, dem, water, rows_per_wave=16)
    assert len(table) >= 4 and (catch["catch_cells"] > 0).all()      # (a cell of the lattice cut short by the raster's edge holds no pond)
    ridge = d == 0
    assert ridge.any() and (basin[1:-1, 1:-1][ridge] > 0).sum() > ridge.sum() // 2


# ---- a long descent -----------------------------------------------------------------------------------------------------------------
def serpentine(R, Cc):
    """a channel that snakes through every other row between high walls and ends in one pond cell"""
    dem = 20000.0 + np.arange(R)[:, None] + np.zeros((R, Cc))
    water = np.zeros((R, Cc))
    k, r, c, step = 0, 0, 0, 1
    while True:
        dem[r, c] = 10000.0 - 0.125 * k
        k += 1
        if 0 <= c + step < Cc:
            c += step
            continue
        if r + 2 >= R:
            break
        dem[r + 1, c] = 10000.0 - 0.125 * k
        k += 1
        r += 2
        step = -step
    dem[r, c] -= 1.0
    water[r, c] = 0.5
    return dem, water


def test_serpentine_channel(hip):
    R, Cc = 131, 385
    dem, water = serpentine(R, Cc)
    bd, bw = pad(dem, water, MISS)
    labels, _ = inventory(bd > MISS, bw, WET)
    assert descent_length(labels, device_dem(bd, MISS), bw) > 20000
    _, table, _, basin, catch, stats = catch_on_device(hip, bd, bw)
    assert len(table) == 1 and catch["catch_cells"][0] == R * Cc - 1 and stats["unponded_cells"] == 0
    assert 2 <= stats["rounds"] <= ROUND_CAP


# ---- labels that alternate under the tally ----------------------------------------------------------------------------------------
def comb(R, Cc):
    """teeth two columns wide that fall towards the last rows, a ridge column between them, one pond at the foot of every tooth"""
    r, c = grid(R, Cc)
    ridge = c % 3 == 0
    dem = np.where(ridge, 500.0 + 0.001 * c, 200.0 - 0.1 * r)
    water = np.where(~ridge & (r >= R - 1), 0.05, 0.0)
    return dem, water


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_comb_of_catchments(hip, R, Cc):
    dem, water = comb(R, Cc)
    labels, table, _, basin, catch, stats = check(hip, dem, water)
    assert len(table) == (Cc + 1) // 3 + (Cc % 3 == 1) and (catch["catch_cells"] >= R - 2).all()
    assert (np.diff(basin[R // 2, 1:-1]) != 0).sum() >= len(table) - 1


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_one_catchment_over_all_segments_and_strips(hip, monkeypatch, R, Cc):
    """a bowl: every cell drains to the one pond in the middle, so one carry runs down every strip"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    r, c = grid(R, Cc)
    d2 = (r - R // 2) ** 2 + (c - Cc // 2) ** 2
    dem = 50.0 + d2 / 64.0
    water = np.where(d2 <= 9, 0.01, 0.0)
    _, table, _, basin, catch, stats = check(hip, dem, water, rows_per_wave=16)
    assert len(table) == 1 and catch["catch_cells"][0] == R * Cc - table["cells"][0] and stats["pit_cells"] == 0
    assert tuple(catch[0].tolist()[3:]) == (1, R, 1, Cc)


# ---- films, signed zeros, walls, NaN water ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
def test_films_and_nan_water_on_the_slopes(hip, R, Cc):
    rng = np.random.default_rng(R)
    dem = rough_dem(R, Cc, R, step=0.25)
    water = np.where(dem < np.quantile(dem, 0.2), 0.3, 0.0)
    film = (water == 0) & (rng.random((R, Cc)) < 0.3)
    water[film] = rng.random(int(film.sum())) * WET            # at most the threshold: slope cells at WET, pond cells at 0
    water[rng.random((R, Cc)) < 0.01] = np.nan
    water[rng.random((R, Cc)) < 0.01] = -0.5
    _, table, _, _, catch, stats = check(hip, dem, water, thresholds=(WET, 0.0))
    assert len(table) > 3 and stats["pit_cells"] > 0


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_signed_zeros(hip, R, Cc):
    rng = np.random.default_rng(Cc)
    dem = np.where(rng.random((R, Cc)) < 0.5, 0.0, -0.0)
    water = np.where(rng.random((R, Cc)) < 0.05, 0.4, 0.0)
    dem[water > 0] = -5.0
    _, table, _, basin, catch, stats = check(hip, dem, water)
    heads = catch["head_level"][catch["catch_cells"] > 0]
    assert (heads == 0).all() and np.signbit(heads).any() and (~np.signbit(heads)).any()
    assert 0 < stats["pit_cells"] < stats["slope_cells"]


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_nodata_walls(hip, R, Cc):
    """walls of NODATA with gaps across a slope: descents go round them or end at them"""
    rng = np.random.default_rng(R + Cc)
    r, c = grid(R, Cc)
    dem = 300.0 - 0.5 * r - 0.001 * c + rng.integers(0, 3, (R, Cc)) * 0.25
    water = np.where(r >= R - 1, 0.2, 0.0)
    wall = (r % 9 == 4) & (c % 23 != 0)
    wall |= (c % 64 == 63) & (r % 5 != 0)
    dem[wall] = MISS
    dem[rng.random((R, Cc)) < 0.002] = np.nan
    _, table, _, basin, catch, stats = check(hip, dem, water)
    assert (basin[1:-1, 1:-1][wall] == -1).all() and stats["pit_cells"] > 0 and int(catch["catch_cells"].sum()) > 0


# ---- noise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, density):
    """water at three densities on rough ground, 3 % NODATA with water on it, at two thresholds on one handle"""
    R, Cc = 131, 385
    rng = np.random.default_rng(int(density * 100))
    dem = rough_dem(R, Cc, int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    _, table, _, _, catch, stats = check(hip, dem, water, thresholds=(WET, 0.01))
    assert len(table) > 10 and int(catch["inflow_cells"].sum()) > 0


# ---- rows per wave --------------------------------------------------------------------------------------------------------------------
def noise_case():
    rng = np.random.default_rng(8)
    dem = rough_dem(131, 385, 8, step=0.125)
    water = np.where(rng.random((131, 385)) < 0.41, 0.002 + rng.random((131, 385)), 0.0)
    dem[rng.random((131, 385)) < 0.03] = MISS
    return dem, water


FORCED = {"noise": noise_case, "comb": lambda: comb(67, 193), "serpentine": lambda: serpentine(33, 200),
          "all wet": lambda: (rough_dem(67, 193, 1), np.full((67, 193), 0.5))}


@pytest.mark.parametrize("rpw", [1, 2, 7, 64, 1000])
@pytest.mark.parametrize("name", list(FORCED))
def test_rows_per_wave_forced(hip, monkeypatch, name, rpw):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    dem, water = FORCED[name]()
    check(hip, dem, water, rows_per_wave=min(rpw, dem.shape[0] + 2))


# ---- thin and degenerate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", [(1, 1), (131, 1), (3, 700)])
def test_thin_rasters(hip, R, Cc):
    rng = np.random.default_rng(R * Cc)
    dem = rough_dem(R, Cc, R + Cc, step=0.25)
    _, table, _, basin, catch, stats = check(hip, dem, np.zeros((R, Cc)))                     # no pond
    assert len(table) == 0 and len(catch) == 0 and stats["unponded_cells"] == R * Cc and (basin[1:-1, 1:-1] == 0).all()
    _, table, _, basin, catch, stats = check(hip, dem, np.full((R, Cc), 0.5))                 # all pond
    assert len(table) == 1 and tuple(catch[0].tolist()) == (0, 0, -np.inf, 1, R, 1, Cc) and stats["slope_cells"] == 0
    if R * Cc > 1:
        check(hip, dem, np.where(rng.random((R, Cc)) < 0.3, 0.3, 0.0), thresholds=(WET, 0.25))


def test_no_pond_and_all_pond(hip):
    R, Cc = 67, 193
    dem = rough_dem(R, Cc, 4)
    _, table, _, basin, catch, stats = check(hip, dem, np.full((R, Cc), WET))                 # exactly the threshold: dry
    assert len(table) == 0 and stats["ponds"] == 0 and stats["slope_cells"] == R * Cc and stats["pit_cells"] > 0
    _, table, _, basin, catch, stats = check(hip, dem, 0.05 + np.random.default_rng(5).random((R, Cc)))
    assert len(table) == 1 and (basin[1:-1, 1:-1] == 1).all() and stats["slope_cells"] == 0


# ---- the handle -----------------------------------------------------------------------------------------------------------------------
def test_handle_state(hip):
    import wdpm_amd
    from wdpm_amd.ponds import CATCH_DTYPE, Ponds, bind
    R, Cc = 46, 70
    dem, water = comb(R, Cc)
    bd, bw = pad(dem, water, MISS)
    dll = bind(hip)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):        # nothing labelled yet
                p.n = 0
                p.catchments(capacity=10)
            n = p.label(WET)
            for ask in (p.catchments, p.basins, p.catchment_stats):
                with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):    # a plain label leaves none
                    ask()
            assert p.label_rims(WET) == n
            rims = p.rims()
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):        # nor does a rim call
                p.catchments()
            assert p.label_catchments(WET) == n == 24
            got = taken(p)
            assert got[2].tobytes() == rims.tobytes()                                   # rims() answers after label_catchments()
            hold_against_model(bd, MISS, bw, WET, got, n)
            want = got[4]
            buf = np.full(n * CATCH_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_catch_table(p._h, buf.ctypes.data, n - 1) != 0              # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_catch_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                                  # ... and writes nothing
            assert dll.wdpm_catch_table(p._h, buf.ctypes.data, n) == 0
            assert buf.tobytes() == want.tobytes() and p.catchments(capacity=n + 7).tobytes() == want.tobytes()
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_catch_label"):
                p.label_catchments(float("nan"))
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_catch_label"):
                p.label_catchments(-1.0)
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.catchment_phase_ms()
            assert p.label_catchments(0.06) == 0                                        # no pond at this threshold: an empty table
            assert len(p.catchments()) == 0 and p.catchment_stats()["unponded_cells"] == R * Cc
            assert p.label_catchments(WET) == n and p.catchments().tobytes() == want.tobytes()
            assert p.label(WET) == n                                                    # a plain label takes the table away again
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):
                p.catchments()
            assert p.label_catchments(WET) == n and p.catchments().tobytes() == want.tobytes()   # and it answers again
            assert p.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import CATCH_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    dem, water = noise_case()
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=131, ncols=385, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            p.label_catchments(WET)
            ms = p.catchment_phase_ms()
            assert tuple(ms) == CATCH_PHASES == ("receivers", "jump", "tally") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.rims_phase_ms()) == {"rims", "locate"} and len(p.phase_ms()) == 6


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
    """Two blocks of real iterations; catchments (the owed drain() of the drain module applied by the call) against the model; a
    third block with another catchment call between begin_block and its first iteration.  The third block is, bit for bit, what a
    twin context computes that never took an inventory."""
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
            n = p.label_catchments(WET)
            got = taken(p)
            hold_against_model(bd, MISS, a.download_water(), WET, got, n)
            assert n >= 1 and int(got[4]["catch_cells"].sum()) > 0
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label_catchments(0.0)
            got = taken(p)
            flushed = a.download_water()
            a.iterate(100)
            md_a = a.max_diff()
            hold_against_model(bd, MISS, flushed, 0.0, got, n2)
            assert p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        assert md_a == md_b
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
        assert a.totaldrain == b.totaldrain
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0


def test_basin5(hip, basin5):
    """basin5 after an add of 300 mm and 300 iterations: everything the call leaves against the models"""
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
            n = p.label_catchments(WET)
            got = taken(p)
            hold_against_model(bd, miss, ctx.download_water(), WET, got, n)
            assert n >= 1 and int(got[4]["catch_cells"].sum()) > 0 and p.guard_bad() == 0
