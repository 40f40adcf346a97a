"""The pond rims on the device (include/wdpm_pond_rims.h, wdpm_amd/csrc/wdpm_pond_rims.hip) against the host model
(tests/pond_rims_model.py, itself held against hand-written answers in tests/test_pond_rims_model.py).

Every case compares the WHOLE rim table for equality - integers by value, doubles by bit pattern; the definitions are exact, there
is no tolerance - next to the label raster and the pond table of the same call, and asserts that no guard byte around the
handle's buffers changed.  Shapes are the smallest at which each mechanism can fail: a wave owns a 64-column segment, a block
four of them; widths are file columns, so the padded width is two more and file column 62 is lane 63 of the first segment.  The
elevations take few distinct values, so that ties between rim cells decide nearly every pond.
"""
import numpy as np
import pytest

from helpers import find_drain, n_bit_diff, pad
from pond_rims_model import assert_same_rims, device_dem, rims
from ponds_model import assert_same, inventory

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001
THRES = 0.005 / 1000


def rims_on_device(hip, bd, bw, thresholds=(WET,), rows_per_wave=None):
    """Upload padded rasters, label with rims at each threshold on ONE handle, hold labels, pond table and rim table against the
    models.  Returns labels and rim table of the last threshold."""
    from wdpm_amd.ponds import RIM_DTYPE, Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            for md in thresholds:
                n = p.label_rims(md)
                labels, table, got, stats = p.labels(), p.table(), p.rims(), p.stats()
                water = ctx.download_water()
                ref_labels, ref_table = inventory(bd > MISS, water, md)
                assert n == len(ref_table) == stats["ponds"]
                assert_same(labels, table, ref_labels, ref_table)
                assert got.dtype == RIM_DTYPE
                assert_same_rims(got, rims(ref_labels, device_dem(bd, MISS), water, n))
                if rows_per_wave is not None:
                    assert stats["rows_per_wave"] == rows_per_wave, stats
            assert p.guard_bad() == 0
    return labels, got


def stepped_dem(R, Cc, seed, nodata=None):
    """few levels, a quarter of a metre apart: ties everywhere"""
    dem = 100.0 + 0.25 * np.random.default_rng(seed).integers(0, 12, (R, Cc))
    if nodata is not None:
        dem[nodata] = MISS
    return dem


def check(hip, water, dem=None, nodata=None, **kw):
    if dem is None:
        dem = stepped_dem(*water.shape, seed=water.size, nodata=nodata)
    return rims_on_device(hip, *pad(dem, water, MISS), **kw)


# ---- seams ------------------------------------------------------------------------------------------------------------------
SEAM_SHAPES = [(70, 200), (67, 193), (131, 385)]


@pytest.mark.parametrize("R,Cc", SEAM_SHAPES)
def test_lines_across_every_seam(hip, R, Cc):
    """a full row, a full column and a staircase (tests/test_ponds.py): one pond whose shoreline crosses every lane, wave and
    block boundary on both sides, with 3 % NODATA among its neighbours"""
    rng = np.random.default_rng(R)
    w = np.zeros((R, Cc))
    w[R // 3, :] = 1
    w[:, Cc // 3] = 1
    cols = [i * (Cc - 1) // (R - 1) for i in range(R)] + [Cc - 1]
    for i in range(R):
        w[i, cols[i]:cols[i + 1] + 1] = 1
    w *= 0.01 + rng.random((R, Cc))
    nodata = (rng.random((R, Cc)) < 0.03) & (w == 0)
    _, t = check(hip, w, nodata=nodata)
    assert len(t) == 1 and t["rim_cells"][0] > 2 * (R + Cc) and t["wall_cells"][0] > 0


@pytest.mark.parametrize("R,Cc", SEAM_SHAPES)
def test_dry_channels_along_every_seam(hip, monkeypatch, R, Cc):
    """All wet, but for one-cell-wide dry channels on both sides of every 64-column seam and of every boundary between the
    strips of rows a wave owns (forced to 16): every rim cell there takes labels from the lanes next door or from memory beside
    the segment, or from a row another wave owns.  The channels break in places, so ponds join across them."""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    rng = np.random.default_rng(Cc)
    w = 0.05 + rng.random((R, Cc))
    for pc in range(64, Cc + 2, 64):                   # padded column pc is lane 0, pc - 1 lane 63; file column = padded - 1
        side = pc // 64 % 2
        w[:, pc - 1 - side] = 0.0
    for pr in range(16, R + 2, 16):
        w[pr - 1 - (pr // 16 % 2), :] = 0.0
    w[rng.random((R, Cc)) < 0.01] = 0.7                # breaches
    _, t = check(hip, w, rows_per_wave=16)
    assert len(t) >= 4


def lowest_rim_targets(R, Cc):
    """padded (row, column) of the cell that is to hold the rim level"""
    rows, ncp = R + 2, Cc + 2
    return {"lane 0": (rows // 2, 64), "lane 63": (rows // 2, 63), "lane 0 of the third segment": (7, 128), "lane 63 of the second": (9, 127),
            "column 1": (rows // 3, 1), "column ncp - 2": (rows // 3, ncp - 2), "row 1": (1, ncp // 2), "row rows - 2": (rows - 2, 65),
            "first corner": (1, 1), "last corner": (rows - 2, ncp - 2)}


@pytest.mark.parametrize("where", list(lowest_rim_targets(70, 200)))
def test_lowest_rim_cell_at_the_edges_of_segments_and_raster(hip, where):
    R, Cc = 70, 200
    r, c = lowest_rim_targets(R, Cc)[where]
    rng = np.random.default_rng(r * 1000 + c)
    dem = stepped_dem(R, Cc, 3)
    w = 0.05 + rng.random((R, Cc))
    dry = rng.random((R, Cc)) < 0.02                   # other rim cells, all higher
    dry[r - 1, c - 1] = True
    w[dry] = 0.0
    dem[r - 1, c - 1] = 50.0
    _, t = check(hip, w, dem=dem)
    assert len(t) == 1
    assert (t["rim_level"][0], t["rim_row"][0], t["rim_col"][0]) == (50.0, r, c)
    assert t["rim_level"][0] - t["surface_max"][0] < 0          # water stands above its spill point: not settled


# ---- four ponds at one rim cell ---------------------------------------------------------------------------------------------
def lattice(R, Cc):
    w = np.zeros((R, Cc))
    w[::2, ::2] = 0.5 + np.arange(((R + 1) // 2) * ((Cc + 1) // 2)).reshape((R + 1) // 2, (Cc + 1) // 2) * 2.0 ** -10
    return w


@pytest.mark.parametrize("R,Cc,shift", [(64, 130, 0), (65, 131, 1)])
def test_four_ponds_at_one_rim_cell(hip, R, Cc, shift):
    """isolated cells at pitch 2: every interior dry cell is a rim cell of 2 or 4 ponds.  Without the shift the ponds sit on
    lane 63 and their rim cells on lane 0 of the next segment; with it the other way round."""
    w = np.roll(lattice(R, Cc), shift, axis=1)
    w[:, :shift] = 0.0
    labels, t = check(hip, w)
    assert len(t) > 2000
    interior = (t["wall_cells"] == 0)
    assert interior.any() and (t["rim_cells"][interior] == 8).all()
    assert int(t["rim_cells"].sum()) > 4 * (R // 2 - 1) * (Cc // 2 - 1)


# ---- random noise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, density):
    """below, in and above the percolation region at 257 x 515; 3 % NODATA with water on it; water below the threshold and NaN water
    on dry cells: the one counts on the rim, the other falls to the DEM"""
    R, Cc = 257, 515
    rng = np.random.default_rng(int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    w = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    film = (w == 0) & (rng.random((R, Cc)) < 0.3)
    w[film] = rng.random(int(film.sum())) * WET        # at most the threshold: dry at WET, wet at 0
    w[rng.random((R, Cc)) < 0.002] = np.nan
    nodata = rng.random((R, Cc)) < 0.03
    _, t = check(hip, w, nodata=nodata, thresholds=(WET, 0.0))
    assert len(t) > 10


# ---- one giant pond with a long shoreline ------------------------------------------------------------------------------------
def serpentine(R, Cc):
    w = np.zeros((R, Cc))
    w[::2, :] = 1
    w[1::4, -1] = 1
    w[3::4, 0] = 1
    return w


def comb(R, Cc):
    w = np.zeros((R, Cc))
    w[:, ::2] = 1
    w[-1, :] = 1
    return w


@pytest.mark.parametrize("name", ["serpentine", "comb"])
def test_giant_pond(hip, name):
    w = {"serpentine": serpentine, "comb": comb}[name](129, 130)
    w *= 0.002 + np.arange(w.size).reshape(w.shape) * 1e-5
    _, t = check(hip, w)
    assert len(t) == 1 and t["rim_cells"][0] > 8000


# ---- rows per wave -----------------------------------------------------------------------------------------------------------
def noise(R, Cc, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((R, Cc)) < density, 0.002 + rng.random((R, Cc)) * 2.0, 0.0), rng.random((R, Cc)) < 0.03


FORCED = {"all wet": lambda: 0.05 + np.random.default_rng(7).random((150, 200)),           # one label down every strip
          "stripes": lambda: np.repeat(np.arange(1, 131)[:, None] % 2 * 0.5, 200, axis=1),   # a new pond on every other row
          "lattice": lambda: lattice(64, 66),                                                # labels alternate inside a row
          "serpentine": lambda: serpentine(129, 130) * (0.002 + np.arange(129 * 130).reshape(129, 130) * 1e-5),
          "noise": lambda: noise(131, 385, 0.41, 8)}


@pytest.mark.parametrize("rpw", [2, 7, 64, 1000])
@pytest.mark.parametrize("name", list(FORCED))
def test_rows_per_wave_forced(hip, monkeypatch, name, rpw):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    made = FORCED[name]()
    w, nodata = made if isinstance(made, tuple) else (made, None)
    check(hip, w, nodata=nodata, rows_per_wave=min(rpw, w.shape[0] + 2))


# ---- thin and degenerate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", [(1, 1), (1, 300), (300, 1), (3, 5000)])
def test_thin_rasters(hip, R, Cc):
    rng = np.random.default_rng(R * Cc)
    _, t = check(hip, np.full((R, Cc), 0.5))
    assert (t["rim_cells"][0], t["wall_cells"][0], t["rim_row"][0], t["rim_col"][0]) == (0, 2 * (R + Cc) + 4, -1, -1)
    assert t["rim_level"][0] == np.inf
    if R * Cc > 1:
        check(hip, np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))


def test_all_wet_and_all_dry(hip):
    from wdpm_amd.ponds import RIM_DTYPE, Ponds, bind
    R, Cc = 150, 200
    _, t = check(hip, 0.05 + np.random.default_rng(5).random((R, Cc)))
    assert len(t) == 1 and (t["rim_cells"][0], t["wall_cells"][0]) == (0, 2 * (R + Cc) + 4)
    assert t["surface_min"][0] < t["surface_max"][0] and t["rim_level"][0] - t["surface_max"][0] == np.inf
    bd, bw = pad(stepped_dem(R, Cc, 1), np.full((R, Cc), WET), MISS)             # exactly the threshold: dry
    dll = bind(hip)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            assert p.label_rims(WET) == 0
            assert dll.wdpm_rims_table(p._h, None, 0) == 0                       # N = 0: capacity 0 will do
            t = p.rims()
            assert len(t) == 0 and t.dtype == RIM_DTYPE and p.guard_bad() == 0


def test_a_pond_enclosed_by_nodata(hip):
    R, Cc = 9, 70
    dem = stepped_dem(R, Cc, 2)
    w = np.zeros((R, Cc))
    dem[2:7, 60:67] = MISS                             # a ring of NODATA over the first seam ...
    dem[3:6, 61:66] = 100.0
    w[3:6, 61:66] = 0.5                                # ... filled to the brim
    w[7, 3] = 0.5                                      # and an ordinary pond beside it
    _, t = check(hip, w, dem=dem)
    assert len(t) == 2
    assert (t["rim_cells"][0], t["wall_cells"][0], t["rim_row"][0], t["rim_col"][0]) == (0, 20, -1, -1)
    assert t["rim_level"][0] == np.inf and (t["rim_cells"][1], t["wall_cells"][1]) == (8, 0)


# ---- ties -------------------------------------------------------------------------------------------------------------------
def test_ties_on_a_flat_dem_go_to_the_smallest_index(hip):
    R, Cc = 40, 140
    w, _ = noise(R, Cc, 0.35, 3)
    labels, t = check(hip, w, dem=np.full((R, Cc), 100.0))
    assert len(t) > 20 and (t["rim_level"] == 100.0).all()
    # the first dry cell beside a pond in row-major order lies in the row above its first cell, or left of it
    for k in range(len(t)):
        rr, cc = np.nonzero(labels == k + 1)
        first_r, first_c = rr[0], cc[rr == rr[0]].min()
        if first_r > 1:
            assert (t["rim_row"][k], t["rim_col"][k]) == (first_r - 1, first_c - 1 if first_c > 1 else first_c)


def test_minus_zero_sorts_below_plus_zero(hip):
    R, Cc = 20, 140
    rng = np.random.default_rng(9)
    w, _ = noise(R, Cc, 0.35, 4)
    dem = np.where(rng.random((R, Cc)) < 0.9, 0.0, -0.0)
    dem[w > 0] = -5.0                                  # ponds below, rims at either zero
    _, t = check(hip, w, dem=dem)
    neg = np.signbit(t["rim_level"])
    assert (t["rim_level"] == 0).all() and neg.any() and (~neg).any()


# ---- the handle -------------------------------------------------------------------------------------------------------------
def test_handle_state(hip):
    import wdpm_amd
    from wdpm_amd.ponds import RIM_DTYPE, Ponds, bind
    R, Cc = 64, 130
    w = lattice(R, Cc)
    bd, bw = pad(stepped_dem(R, Cc, 6), w, MISS)
    dll = bind(hip)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):      # nothing labelled yet
                p.n = 0
                p.rims(capacity=10)
            n = p.label(WET)
            plain_labels, plain_table = p.labels(), p.table()
            with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):      # a plain label leaves none
                p.rims()
            assert p.label_rims(WET) == n == 32 * 65
            assert (p.labels() == plain_labels).all() and p.table().tobytes() == plain_table.tobytes()
            want = rims(plain_labels, device_dem(bd, MISS), bw, n)
            buf = np.full(n * RIM_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_rims_table(p._h, buf.ctypes.data, n - 1) != 0       # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_rims_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                          # ... and writes nothing
            assert dll.wdpm_rims_table(p._h, buf.ctypes.data, n) == 0
            assert_same_rims(buf.view(RIM_DTYPE), want)
            assert_same_rims(p.rims(capacity=n + 7), want)
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_rims_label"):
                p.label_rims(float("nan"))
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_rims_label"):
                p.label_rims(-1.0)
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.rims_phase_ms()
            assert p.label_rims(0.6) < n                                       # a smaller table in the same buffer
            assert_same_rims(p.rims(), rims(p.labels(), device_dem(bd, MISS), bw, p.n))
            assert p.label(WET) == n                                           # and a plain label takes the rim table away again
            with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):
                p.rims()
            assert p.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import RIM_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    w, _ = noise(70, 200, 0.41, 5)
    bd, bw = pad(stepped_dem(70, 200, 5), w, MISS)
    with hip.context(module="add", nrows=70, ncols=200, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            p.label_rims(WET)
            ms = p.rims_phase_ms()
            assert tuple(ms) == RIM_PHASES == ("rims", "locate") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.phase_ms()) == {"mask", "merge", "flatten", "scan", "table", "finish"}


# ---- real water, and the context is left as it was -------------------------------------------------------------------------
def real_case(hip, module):
    dem = hip.synth_dem(700, 300)[:300, :].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    kw = dict(module=module, nrows=300, ncols=700, missingvalue=MISS)
    if module == "drain":
        dr, dc = find_drain(bd)
        kw.update(drainrow=dr, draincol=dc)
    return bd, bw, kw


@pytest.mark.parametrize("module", ["add", "drain"])
def test_state_neutrality(hip, module):
    """Two blocks; rims (the owed drain() of the drain module applied by the call); a third block with another rim call between
    begin_block and its first iteration (the owed threshold flush applied by the call).  The third block is, bit for bit, what a
    twin context computes that never took an inventory (tests/test_ponds.py holds the twin against the oracle)."""
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    bd, bw, kw = real_case(hip, module)
    dem = device_dem(bd, MISS)
    with hip.context(**kw) as a, hip.context(**kw) as b:
        for c in (a, b):
            c.upload(bd, bw)
            c.totaldrain = 0.0
            c.run_block(100, THRES)
            c.run_block(100, THRES)
        with Ponds(a) as p:
            n = p.label_rims(WET)
            labels, table, got = p.labels(), p.table(), p.rims()
            water = a.download_water()
            assert_same(labels, table, *inventory(bd > MISS, water, WET))
            assert_same_rims(got, rims(labels, dem, water, n))
            assert n >= 1 and int(got["rim_cells"].sum()) > 0
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label_rims(0.0)
            labels, got = p.labels(), p.rims()
            flushed = a.download_water()
            a.iterate(100)
            md_a = a.max_diff()
            assert_same_rims(got, rims(labels, dem, flushed, n2))
            assert p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        assert md_a == md_b
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
        assert a.totaldrain == b.totaldrain
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0


def test_basin5(hip, basin5):
    """the water of tests/golden/basin5_state.npz (add 300 mm, 1000 iterations; the file keeps every seventh row, which is
    enough to know that this is that water): the whole rim table against the model"""
    import os

    from conftest import GOLDEN
    from helpers import bits_equal
    from wdpm_amd.ponds import Ponds
    dem, hdr = basin5
    miss = hdr["NODATA_value"] if "NODATA_value" in hdr else hdr[[k for k in hdr if k.lower().startswith("nodata")][0]]
    R, Cc = dem.shape
    bd, _ = pad(dem, np.zeros_like(dem), miss)
    bw = np.where(bd > miss, 0.3, 0.0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=miss) as ctx:
        ctx.upload(bd, bw)
        ctx.run_block(1000, THRES)
        with Ponds(ctx) as p:
            n = p.label_rims(WET)
            labels, table, got = p.labels(), p.table(), p.rims()
            water = ctx.download_water()
            assert bits_equal(water[::7], np.load(os.path.join(GOLDEN, "basin5_state.npz"))["add300_k1000_rows"])
            assert_same(labels, table, *inventory(bd > miss, water, WET))
            assert_same_rims(got, rims(labels, device_dem(bd, miss), water, n))
            assert n >= 1 and p.guard_bad() == 0
