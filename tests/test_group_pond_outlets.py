"""The pond outlets over row blocks on the device (include/wdpm_group_pond_outlets.h, wdpm_amd.ponds.GroupPonds.label_outlets): N ranks
on one GPU (devices = [0] * N), every rank taking the passes of its own rows, the host making the pour levels final between the two
device passes.  Outlet table and counts are held against the host model (tests/pond_outlets_model.outlets) on the labels the group
returns, the water it downloads and the device's DEM, and against Ponds.label_outlets on a twin whole-raster context; everything else
the call leaves against a twin group's label_catchments(), bit for bit; the two statements of include/wdpm_pond_outlets.h and the
guard bands after every call (tests/group_pond_outlets_cases.check_outlets).  Every comparison is equality.  exchange_every = 1
unless stated.  Shapes are those of tests/test_group_pond_catchments.py: two, four and seven 64-column segments per row.

The row-block partition gives no rank fewer than five owned rows, so a rank of ONE owned row cannot be made here: strips of one row
run in tests/test_group_outlets_merge.py, on the kernels' own source; the smallest slabs the partition allows run below."""
import numpy as np
import pytest

import group_pond_outlets_cases as oc
import group_pond_rims_cases as rc
from group_pond_outlets_cases import NONE, OutletCase, check_outlets, row
from group_ponds_cases import MISS, WET, slabs_of
from helpers import find_drain, n_bit_diff, pad

pytestmark = pytest.mark.gpu
SHAPES = [(46, 70), (67, 193), (131, 385)]
RANKS = [2, 3, 8]


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_the_outlet_pair_across_every_boundary(hip, R, Cc, n):
    """three upward and three downward directions, from pond cells and from cells of the catchment, at lanes 63 | 0 and at columns 1
    and ncp - 2"""
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_lines_across(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_ties_across_a_boundary_go_to_the_lower_rank(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_ties_across(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", [3, 8])
def test_a_basin_over_every_rank_with_its_only_outlet_in_the_second(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_long_basin(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_a_remote_pond_whose_outlet_another_rank_finds(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_remote(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_mutual_outlets_land_and_pond_cells_across_a_boundary(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_columns(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_barriers_one_basin_no_pond(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_barriers(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_a_quiet_row_that_is_not_quiet(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_not_quiet(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc,n", [(8, 70, 2), (15, 70, 3), (21, 130, 4)])
def test_the_smallest_slabs(hip, R, Cc, n):
    """five and six owned rows per rank: every row of a middle rank is within three rows of both its boundaries"""
    with OutletCase(hip, R, Cc, [0] * n) as case:
        w, nodata = rc.noise(R, Cc, 0.41, R)
        table, stats, _, _ = case.check(w, nodata=nodata, thresholds=(WET, 0.0))
        assert len(table) > 3 and stats["seam_outlets"] > 0, stats
        oc.run_not_quiet(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_signed_zeros_and_films_on_seam_rows(hip, R, Cc, n):
    with OutletCase(hip, R, Cc, [0] * n) as case:
        oc.run_seam_levels(case, slabs_of(hip, R, n))


def test_a_600_m_pit_on_one_rank_fails_the_whole_call(hip):
    import wdpm_amd
    R, Cc = 67, 193
    with OutletCase(hip, R, Cc, [0] * 3) as case:
        slabs = slabs_of(hip, R, 3)
        w, nodata = rc.noise(R, Cc, 0.41, 5)
        dem = rc.ramp_dem(R, Cc, nodata=nodata)
        deep = dem.copy()
        r = slabs[2].own_lo + 2                                # in the last rank's rows: a pit of one cell 600 m down, a pond in it
        deep[r - 1, 21] = -500.0
        wet = w.copy()
        wet[r - 1, 21] = 0.5
        case.upload(wet, deep)
        p = case.ponds
        with pytest.raises(wdpm_amd.WdpmError, match="512 m"):
            p.label_outlets(WET)
        for call in (p.outlets, p.outlet_stats, p.table, p.rims, p.catchments, p.basins, p.labels):
            with pytest.raises(wdpm_amd.WdpmError):
                call()
        assert p.guard_bad() == 0
        n = p.label_catchments(WET)                            # the handle stays usable: the lesser call on the same water ...
        assert n > 3 and len(p.catchments()) == n
        with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
            p.outlets()
        case.check(w, dem)                                     # ... and the whole call on shallower water
        assert p.guard_bad() == 0


def test_handle_states(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import OUTLET_PHASES
    R, Cc = 46, 70
    w, nodata = rc.noise(R, Cc, 0.41, 9)
    with OutletCase(hip, R, Cc, [0, 0]) as case:
        p = case.ponds
        with pytest.raises(wdpm_amd.WdpmError):
            p.outlets()
        p.n = 0
        for call in (p.outlets, p.outlet_stats):
            with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
                call()
        table, stats, basin, labels = case.check(w, nodata=nodata)
        catch = p.catchments()
        for lesser in (p.label, p.label_rims, p.label_catchments):       # every lesser label call takes the outlet table away
            assert lesser(WET) == len(table)
            for call in (p.outlets, p.outlet_stats):
                with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
                    call()
            assert p.labels().tobytes() == labels.tobytes()              # ... and answers as the outlet call did
        assert p.catchments().tobytes() == catch.tobytes() and p.basins().tobytes() == basin.tobytes()
        assert p.label_outlets(WET) == len(table)
        assert p.outlets().tobytes() == table.tobytes()
        assert {k: v for k, v in p.outlet_stats().items() if k != "merge_ms"} == {k: v for k, v in stats.items() if k != "merge_ms"}
        out = np.full(len(table) - 1, 7, dtype=table.dtype)
        with pytest.raises(wdpm_amd.WdpmError, match="capacity"):
            p.lib.check(p.dll.wdpm_group_outlets_table(p._h, out.ctypes.data, len(out)))
        assert (out == np.full(len(out), 7, dtype=table.dtype)).all()    # capacity < N writes nothing
        with pytest.raises(wdpm_amd.WdpmError, match="WDPM_PONDS_TIMING"):
            p.outlet_phase_ms(0)
        with pytest.raises(wdpm_amd.WdpmError):
            p.label_outlets(float("inf"))
        assert p.guard_bad() == 0
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    with OutletCase(hip, R, Cc, [0, 0]) as case:
        case.check(w, nodata=nodata)
        for i in range(2):
            ms = case.ponds.outlet_phase_ms(i)
            assert list(ms) == list(OUTLET_PHASES) and all(v >= 0 for v in ms.values())
        with pytest.raises(wdpm_amd.WdpmError, match="rank"):
            case.ponds.outlet_phase_ms(2)
        case.ponds.label_catchments(WET)
        with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
            case.ponds.outlet_phase_ms(0)


@pytest.mark.parametrize("n", RANKS)
def test_noise_at_three_densities(hip, n):
    with OutletCase(hip, 131, 385, [0] * n) as case:
        oc.run_noise(case)


@pytest.mark.parametrize("R,Cc,n", [(60, 1, 8), (46, 5000, 3)])
def test_thin_rasters(hip, R, Cc, n):
    rng = np.random.default_rng(R * Cc)
    with OutletCase(hip, R, Cc, [0] * n) as case:
        table, stats, _, _ = case.check(np.full((R, Cc), 0.5))
        assert len(table) == 1 and row(table, 0) == NONE, table
        table, stats, _, _ = case.check(np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))
        assert len(table) > 3 and stats["seam_outlets"] > 0, stats


@pytest.mark.parametrize("rpw", [1, 2, 7, 64])
def test_rows_per_wave_forced(hip, monkeypatch, rpw):
    """WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made: strips of rpw rows cut over each rank's owned rows"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    for n in (2, 8):
        with OutletCase(hip, 46, 70, [0] * n) as case:
            oc.run_lines_across(case, slabs_of(hip, 46, n), directions=[(1, 1), (-1, 0)])
            oc.run_ties_across(case, slabs_of(hip, 46, n))
            got = case.ponds.rank_stats(1)["rows_per_wave"]
            assert got == rpw or (rpw == 64 and 3 <= got < 64), got      # never more rows than the rank's view holds
    with OutletCase(hip, 131, 385, [0] * 3) as case:
        oc.run_noise(case, densities=(0.41,))
        oc.run_long_basin(case, slabs_of(hip, 131, 3))


def test_a_group_of_one_rank(hip):
    R, Cc = 67, 193
    w, nodata = rc.noise(R, Cc, 0.41, 5)
    with OutletCase(hip, R, Cc, [0]) as one:
        table, stats, _, _ = one.check(w, nodata=nodata)
        assert len(table) > 10 and stats["ranks"] == 1 and stats["seam_outlets"] == 0 and stats["split_ponds"] == 0, stats


@pytest.mark.parametrize("module", ["add", "drain"])
def test_real_water_after_blocks_of_iterations(hip, module):
    """After a block of iterations (a drain group then owes the last iteration's drain()) the outlets equal the model on the water
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
            table, stats, _, _ = check_outlets(a, p, bd, WET)
            assert len(table) >= 1 and int(p.table()["cells"].sum()) == a.count_stats()[1], stats
        md_a, md_b = a.run_block(100, thres), b.run_block(100, thres)
        assert md_a == md_b and a.totaldrain() == b.totaldrain()
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
