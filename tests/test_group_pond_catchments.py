"""The pond catchments over row blocks on the device (include/wdpm_group_pond_catchments.h, wdpm_amd.ponds.GroupPonds.label_catchments):
N ranks on one GPU (devices = [0] * N), every rank taking the receivers, the jump rounds and the tally of its own rows, the host
following the descents that cross row blocks.  Basin raster, catchment table and counts are held against the host model
(tests/pond_catchments_model.catchments) on the labels the group returns, the water it downloads and the device's DEM; labels, pond
table and rim table of the same call against a twin group's label_rims(), bit for bit; the whole-raster identity and the guard bands
after every call (tests/group_pond_catchments_cases.check_catchments).  Every comparison is equality.  exchange_every = 1 unless
stated.  Shapes are those of tests/test_group_pond_rims.py: one, three and six 64-column segments per row."""
import numpy as np
import pytest

import group_pond_catchments_cases as cc
import group_pond_rims_cases as rc
from group_pond_catchments_cases import CatchCase, check_catchments
from group_ponds_cases import MISS, WET, slabs_of
from helpers import find_drain, n_bit_diff, pad
from pond_catchments_model import assert_same_catchments
from ponds_model import assert_same

pytestmark = pytest.mark.gpu
SHAPES = [(46, 70), (67, 193), (131, 385)]
RANKS = [2, 3, 8]


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_ramps_in_the_eight_directions_across_every_boundary(hip, R, Cc, n):
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_ramps(case)


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_a_receiver_that_is_a_pond_cell_of_the_neighbours_row(hip, R, Cc, n):
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_pond_cell_across(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_zigzag_along_a_boundary_and_ties_across_it(hip, R, Cc, n):
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_zigzag(case, slabs_of(hip, R, n))
        cc.run_ties(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_a_channel_through_every_rank_and_back(hip, R, Cc, n):
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_snake(case, slabs_of(hip, R, n))


def test_a_long_descent_within_one_rank_next_to_one_that_exits(hip):
    """a serpentine channel of more than 100 000 cells over three ranks: more than 20 000 hops inside each before the descent exits"""
    R, Cc = 46, 5000
    dem, water, cells = cc.serpentine(R, Cc)
    with CatchCase(hip, R, Cc, [0] * 3) as case:
        _, table, basin, catch, stats = case.check(water, dem)
        assert cells > 100000 and len(table) == 1 and catch["catch_cells"][0] == R * Cc - 1 and stats["rounds"] > cc.BATCH, (stats, catch)
        assert stats["exits"] > 40000 and stats["remote"] == 2, stats      # the pond lies deep in the last rank's rows


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_levels_on_the_seam_rows_and_a_nodata_wall(hip, R, Cc, n):
    """signed zeros, films at or below the threshold and NaN water on both rows of every boundary - the neighbour's level comes
    from its owner's key; flats and pits there; NODATA all along every boundary"""
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_seam_levels(case, slabs_of(hip, R, n))
        cc.run_nodata_wall(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_odd_ranks_a_cone_and_shared_slots(hip, R, Cc, n):
    with CatchCase(hip, R, Cc, [0] * n) as case:
        cc.run_odd_ranks(case, slabs_of(hip, R, n))
        cc.run_cone(case, slabs_of(hip, R, n))
        cc.run_shared_slots(case)


@pytest.mark.parametrize("n", RANKS)
def test_noise(hip, n):
    with CatchCase(hip, 131, 385, [0] * n) as case:
        cc.run_noise(case)


@pytest.mark.parametrize("n", [2, 5])
def test_noise_at_the_default_exchange_interval(hip, n):
    with CatchCase(hip, 257, 515, [0] * n, every=None) as case:
        cc.run_noise(case)


@pytest.mark.parametrize("rpw", [1, 2, 7, 64])
def test_rows_per_wave_forced(hip, monkeypatch, rpw):
    """WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made: strips of rpw rows cut over each rank's owned rows"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    for n in (2, 8):
        with CatchCase(hip, 46, 70, [0] * n) as case:
            cc.run_ramps(case, directions=[(1, 1), (-1, 0)], pits=())
            cc.run_zigzag(case, slabs_of(hip, 46, n))
            got = case.ponds.rank_stats(1)["rows_per_wave"]
            assert got == rpw or (rpw == 64 and 3 <= got < 64), got      # never more rows than the rank's view holds
    with CatchCase(hip, 131, 385, [0] * 3) as case:
        cc.run_noise(case, densities=(0.41,))
        cc.run_cone(case, slabs_of(hip, 131, 3))


@pytest.mark.parametrize("R,Cc,n", [(60, 1, 8), (46, 5000, 3)])
def test_thin_rasters(hip, R, Cc, n):
    rng = np.random.default_rng(R * Cc)
    with CatchCase(hip, R, Cc, [0] * n) as case:
        _, table, basin, catch, stats = case.check(np.full((R, Cc), 0.5))
        assert len(table) == 1 and stats["slope_cells"] == 0, stats
        case.check(np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))


def test_against_the_whole_raster_answer_of_the_device(hip):
    """Ponds.label_catchments on a context given the same DEM and the water the group downloads; and a group of one rank"""
    from wdpm_amd.ponds import Ponds
    R, Cc = 67, 193
    w, nodata = rc.noise(R, Cc, 0.41, 5)
    with CatchCase(hip, R, Cc, [0] * 3) as case, CatchCase(hip, R, Cc, [0]) as one:
        labels, table, basin, catch, stats = case.check(w, nodata=nodata)
        labels1, table1, basin1, catch1, stats1 = one.check(w, nodata=nodata)
        assert stats1["ranks"] == 1 and stats["exits"] > 0
        water = case.grp.download_water()
        with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
            ctx.upload(case.bd, water)
            with Ponds(ctx) as p:
                assert p.label_catchments(WET) == len(table) == len(table1)
                whole = p.basins(), p.catchments(), p.catchment_stats()
                assert_same(labels, table, p.labels(), p.table())
                assert p.guard_bad() == 0
        for got in ((basin, catch, stats), (basin1, catch1, stats1)):
            assert_same_catchments(*got, whole[0], whole[1], {k: v for k, v in whole[2].items() if k != "rounds"})
        assert (labels == labels1).all()


def test_handle_states(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import CATCH_PHASES
    R, Cc = 46, 70
    w, nodata = rc.noise(R, Cc, 0.41, 9)
    with CatchCase(hip, R, Cc, [0, 0]) as case:
        p = case.ponds
        with pytest.raises(wdpm_amd.WdpmError):
            p.catchments()
        p.n = 0
        for call in (p.catchments, p.basins, p.catchment_stats):
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):
                call()
        labels, table, basin, catch, stats = case.check(w, nodata=nodata)
        rims = p.rims()
        for lesser in (p.label, p.label_rims):                 # a lesser label call takes the catchment table away again
            assert lesser(WET) == len(table)
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):
                p.catchments()
            with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):
                p.basins()
            assert_same(labels, table, p.labels(), p.table())  # ... and answers as the catchment call did
        assert p.rims().tobytes() == rims.tobytes()
        assert p.label_catchments(WET) == len(table)
        assert_same_catchments(p.basins(), p.catchments(), p.catchment_stats(), basin, catch, {k: v for k, v in stats.items() if k not in ("resolve_ms", "rounds")})
        out = np.full(len(table) - 1, 7, dtype=catch.dtype)
        with pytest.raises(wdpm_amd.WdpmError, match="capacity"):
            p.lib.check(p.dll.wdpm_group_catch_table(p._h, out.ctypes.data, len(out)))
        assert (out == np.full(len(out), 7, dtype=catch.dtype)).all()      # capacity < N writes nothing
        with pytest.raises(wdpm_amd.WdpmError, match="WDPM_PONDS_TIMING"):
            p.catchment_phase_ms(0)
        with pytest.raises(wdpm_amd.WdpmError):
            p.label_catchments(float("inf"))
        # a call that fails - a pond cell of 512 m, which the pond table refuses - leaves the handle usable
        deep = w.copy()
        deep[3, 3] = 600.0
        bd, bw = pad(rc.ramp_dem(R, Cc, nodata=nodata), deep, MISS)
        case.grp.upload(bd, bw)
        with pytest.raises(wdpm_amd.WdpmError, match="512 m"):
            p.label_catchments(WET)
        with pytest.raises(wdpm_amd.WdpmError):
            p.catchments()
        case.check(w, nodata=nodata)
        assert p.guard_bad() == 0
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    with CatchCase(hip, R, Cc, [0, 0]) as case:
        case.check(w, nodata=nodata)
        for i in range(2):
            ms = case.ponds.catchment_phase_ms(i)
            assert list(ms) == list(CATCH_PHASES) and all(v >= 0 for v in ms.values())
        with pytest.raises(wdpm_amd.WdpmError, match="rank"):
            case.ponds.catchment_phase_ms(2)
        case.ponds.label_rims(WET)
        with pytest.raises(wdpm_amd.WdpmError, match="no catchment table"):
            case.ponds.catchment_phase_ms(0)


def test_the_whole_raster_call_still_refuses_a_row_block(hip):
    """wdpm_catch_label is for handles of wdpm_ponds_create, and no such handle views a rank's slab context"""
    import types

    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    with CatchCase(hip, 46, 70, [0, 0]) as case:
        ctx = types.SimpleNamespace(lib=hip, _h=case.grp.rank_ctx(0), shape=case.grp.shape)
        with pytest.raises(wdpm_amd.WdpmError, match="slab context"):
            Ponds(ctx)


@pytest.mark.parametrize("module", ["add", "drain"])
def test_state_neutrality(hip, module):
    """After a block of iterations (a drain group then owes the last iteration's drain()) the catchments equal the model on the water
    the group downloads, and a further block is bit for bit that of a twin group that took no inventory."""
    from wdpm_amd.ponds import GroupPonds
    from wdpm_amd.rowblock import Group
    thres = 0.005 / 1000
    dem = hip.synth_dem(700, 300)[:300, :].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    kw = {}
    if module == "drain":
        dr, dc = find_drain(bd)
        kw = dict(drainrow=dr, draincol=dc)
    with Group(hip, module, 300, 700, MISS, [0, 0, 0], **kw) as a, Group(hip, module, 300, 700, MISS, [0, 0, 0], **kw) as b:
        for g in (a, b):
            g.upload(bd, bw)
            if module == "drain":
                g.set_totaldrain(0.0)
            g.run_block(100, thres)
        with GroupPonds(a) as p:
            _, table, basin, catch, stats = check_catchments(a, p, bd, WET)
            assert len(table) >= 1 and int(table["cells"].sum()) == a.count_stats()[1], stats
        md_a, md_b = a.run_block(100, thres), b.run_block(100, thres)
        assert md_a == md_b and a.totaldrain() == b.totaldrain()
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
