"""The pond stage curves over row blocks on the device (include/wdpm_group_pond_curves.h, wdpm_amd.ponds.GroupPonds.label_stage_curves):
N ranks on one GPU (devices = [0] * N), every rank taking the bed and the stage counts of its own rows, the host making the beds final
between the two device passes.  Curve table and counts are held against the host model (tests/pond_curves_model.py, imported and not
changed) on the water the group downloads, against Ponds.label_curves on a twin whole-raster context holding that water, and
everything else the call leaves against a twin group's label_outlets(), under the suite's guard bands
(tests/group_pond_curves_cases.check_curves).  Every comparison is equality; doubles are compared by bit pattern.  Shapes are those of
tests/test_group_pond_outlets.py: 2, 3 and 8 ranks at two, four and seven 64-column segments per row; 8 ranks at 46 rows are the
smallest slabs the partition allows, five owned rows."""
import numpy as np
import pytest

import group_pond_curves_cases as cc
from group_pond_curves_cases import CurveCase, check_curves
from group_ponds_cases import MISS, WET, slabs_of
from helpers import pad

pytestmark = pytest.mark.gpu
CASES = [(2, 46, 70), (3, 67, 193), (8, 131, 385), (8, 46, 70)]
ids = lambda c: "%d-ranks-%dx%d" % c if isinstance(c, tuple) else None


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_a_bed_in_the_rank_next_door(hip, case):
    n, R, Cc = case
    with CurveCase(hip, R, Cc, [0] * n) as k:
        cc.run_remote_bed(k, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", [(46, 70), (131, 385)])
def test_one_basin_over_eight_ranks_bed_in_rank_5_pass_in_rank_0(hip, R, Cc):
    with CurveCase(hip, R, Cc, [0] * 8) as k:
        cc.run_skipped_rank(k, slabs_of(hip, R, 8))


@pytest.mark.parametrize("rpw", [0, 1, 2, 3, 64])
def test_wave_and_strip_edges(hip, monkeypatch, rpw):
    """WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made: strips of rpw rows cut over each rank's owned rows (0: the library's
    choice); beds on every rank's first and last owned row, on lanes 0 and 63 and on columns 1 and ncp - 2, bands of basin across
    lanes 63 | 0; and a raster whose basin changes in every lane of every row"""
    if rpw:
        monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    else:
        monkeypatch.delenv("WDPM_PONDS_ROWS_PER_WAVE", raising=False)
    for n, R, Cc in ((8, 46, 70), (3, 67, 193)):
        with CurveCase(hip, R, Cc, [0] * n) as k:
            cc.run_edges(k, slabs_of(hip, R, n))
            cc.run_stripes(k)
            got = k.ponds.rank_stats(1)["rows_per_wave"]
            assert got == rpw or rpw == 0 or (rpw == 64 and 3 <= got < 64), got


@pytest.mark.parametrize("case", [(2, 67, 193), (3, 67, 193), (8, 131, 385)], ids=ids)
def test_the_stage_rule_on_a_boundary(hip, case):
    n, R, Cc = case
    with CurveCase(hip, R, Cc, [0] * n) as k:
        cc.run_stage_rule(k, slabs_of(hip, R, n))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_degenerate_curves(hip, case):
    n, R, Cc = case
    with CurveCase(hip, R, Cc, [0] * n) as k:
        slabs = slabs_of(hip, R, n)
        cc.run_degenerate(k, slabs)
        cc.run_no_outlet(k, slabs)
        cc.run_beside(k, slabs)
        cc.run_films(k)


def test_a_600_m_pit_with_its_floor_in_one_rank_and_its_way_out_in_another(hip):
    """tests/test_pond_curves.test_a_600_m_pit_fails_and_the_handle_stays_usable stood on end across the boundary: label_outlets()
    succeeds, label_stage_curves() fails with the message, leaves no table of any kind and the handle usable"""
    import wdpm_amd
    from test_pond_curves import cones_scene
    R, Cc = 46, 70
    with CurveCase(hip, R, Cc, [0, 0]) as k:
        hi = cc.boundaries(slabs_of(hip, R, 2))[0]
        dem, water, _ = cones_scene(R, Cc, [(10, 20), (36, 50)])
        deep = dem.copy()
        deep[hi - 2:hi + 3, 39:42] = 1700.0                        # walls
        deep[hi - 1:hi + 2, 40] = [1000.0, 1600.0, 1001.0]         # the floor on the last row above the boundary, the way out below it
        pit_w = water.copy()
        pit_w[hi - 1, 40] = 500.0
        k.upload(pit_w, deep)
        p = k.ponds
        n = p.label_outlets(WET)                                   # the lesser call succeeds
        assert n == 3 and 1600.0 in p.outlets()["pour_level"].tolist()
        with pytest.raises(wdpm_amd.WdpmError, match="wdpm_group_curves_label.*512 m"):
            p.label_stage_curves(WET)
        with pytest.raises(wdpm_amd.WdpmError, match="label_stage_curves\\(\\) has not succeeded"):
            p.stage_curves()
        p.n = n
        for ask in (p.stage_curves, p.stage_curve_stats):
            with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
                ask()
        for ask in (p.table, p.rims, p.catchments, p.outlets, p.labels, p.basins):      # no table of any kind
            with pytest.raises(wdpm_amd.WdpmError):
                ask()
        assert p.guard_bad() == 0
        assert p.label_outlets(WET) == n and len(p.outlets()) == n
        k.check(water, dem)                                        # the next call, on other water, succeeds
        assert p.guard_bad() == 0


def test_handle_states(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import CURVE_PHASES
    from group_pond_rims_cases import noise
    R, Cc = 46, 70
    w, nodata = noise(R, Cc, 0.41, 9)
    monkeypatch.delenv("WDPM_PONDS_TIMING", raising=False)
    with CurveCase(hip, R, Cc, [0, 0]) as k:
        p = k.ponds
        with pytest.raises(wdpm_amd.WdpmError, match="GroupPonds.stage_curves: label_stage_curves\\(\\) has not succeeded"):
            p.stage_curves()
        k.upload(w, nodata=nodata)
        n = p.label_outlets(WET)                                   # a handle whose last label call was label_outlets: named
        assert n > 3
        with pytest.raises(wdpm_amd.WdpmError, match="wdpm_group_curves_table: no curve table.*wdpm_group_curves_label"):
            p.stage_curves()
        with pytest.raises(wdpm_amd.WdpmError, match="wdpm_group_curves_stats: no curve table"):
            p.stage_curve_stats()
        table, stats, basin = k.check(w, nodata=nodata, thresholds=(0.01, WET))          # two thresholds on one handle
        left = cc.older(p)
        for lesser in (p.label, p.label_rims, p.label_catchments, p.label_outlets):     # every lesser label call takes the table away
            assert lesser(WET) == len(table)
            for ask in (p.stage_curves, p.stage_curve_stats):
                with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
                    ask()
            assert p.labels().tobytes() == left[0].tobytes() and p.table().tobytes() == left[1].tobytes()
        for mine, theirs in zip(cc.older(p), left):                # after label_outlets: everything the curve call had left
            assert mine.tobytes() == theirs.tobytes()
        assert p.label_stage_curves(WET) == len(table)
        assert p.stage_curves().tobytes() == table.tobytes()
        assert cc.plain(p.stage_curve_stats(), ("merge_ms",)) == cc.plain(stats, ("merge_ms",))
        out = np.full(len(table) - 1, 7, dtype=table.dtype)
        with pytest.raises(wdpm_amd.WdpmError, match="capacity"):
            p.lib.check(p.dll.wdpm_group_curves_table(p._h, out.ctypes.data, len(out)))
        assert out.tobytes() == np.full(len(out), 7, dtype=table.dtype).tobytes()      # capacity < N writes nothing
        assert p.stage_curves(capacity=len(table) + 5).tobytes() == table.tobytes()
        with pytest.raises(wdpm_amd.WdpmError, match="WDPM_PONDS_TIMING"):
            p.stage_curve_phase_ms(0)
        for bad in (float("inf"), float("nan"), -1.0):
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_group_curves_label"):
                p.label_stage_curves(bad)
        assert p.label_stage_curves(400.0) == 0 and len(p.stage_curves()) == 0 and p.stage_curve_stats()["ponds"] == 0
        assert p.guard_bad() == 0
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    with CurveCase(hip, R, Cc, [0, 0]) as k:
        k.check(w, nodata=nodata)
        for i in range(2):
            ms = k.ponds.stage_curve_phase_ms(i)
            assert tuple(ms) == CURVE_PHASES and all(v >= 0 for v in ms.values()), ms
            assert set(k.ponds.outlet_phase_ms(i)) == {"passes", "locate"}
        with pytest.raises(wdpm_amd.WdpmError, match="rank"):
            k.ponds.stage_curve_phase_ms(2)
        k.ponds.label_outlets(WET)
        with pytest.raises(wdpm_amd.WdpmError, match="no curve table"):
            k.ponds.stage_curve_phase_ms(0)


def test_a_group_of_one_rank(hip):
    R, Cc = 67, 193
    with CurveCase(hip, R, Cc, [0]) as one:
        cc.run_noise(one, densities=(0.41,))
        cc.run_stripes(one)
        t, s, _ = one.check(*cc.cones(R, Cc, [(1, 20), (R, 30), (30, 63), (40, 64)])[1::-1])
        assert len(t) == 4 and s["ranks"] == 1


@pytest.mark.parametrize("n", [2, 3, 8])
def test_noise_at_three_densities(hip, n):
    with CurveCase(hip, 131, 385, [0] * n) as k:
        cc.run_noise(k)


@pytest.mark.parametrize("n", [3, 8])
def test_smooth_bowls_cut_by_the_ranks(hip, n):
    with CurveCase(hip, 131, 385, [0] * n) as k:
        cc.run_smooth_bowls(k)


def test_real_water_after_add_iterations_on_the_group(hip):
    from wdpm_amd.ponds import GroupPonds, Ponds
    from wdpm_amd.rowblock import Group
    thres = 0.005 / 1000
    dem = hip.synth_dem(385, 131)[:131, :385].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    with Group(hip, "add", 131, 385, MISS, [0, 0, 0]) as g, hip.context(module="add", nrows=131, ncols=385, missingvalue=MISS) as ctx:
        g.upload(bd, bw)
        g.run_block(100, thres)
        g.run_block(100, thres)
        with GroupPonds(g) as p, Ponds(ctx) as q:
            t, s, _ = check_curves(g, p, bd, WET, whole=(ctx, q))
            assert len(t) >= 1 and s["stage_cells"] > 0


def test_basin5_in_three_ranks(hip, basin5):
    """basin5 after an add of 300 mm and 300 iterations on the group"""
    from pond_curves_model import assert_same_curves
    from test_pond_curves import reference
    from wdpm_amd.ponds import GroupPonds, Ponds
    from wdpm_amd.rowblock import Group
    dem, hdr = basin5
    miss = hdr["NODATA_value"] if "NODATA_value" in hdr else hdr[[h for h in hdr if h.lower().startswith("nodata")][0]]
    R, Cc = dem.shape
    bd, _ = pad(dem, np.zeros_like(dem), miss)
    bw = np.where(bd > miss, 0.3, 0.0)
    with Group(hip, "add", R, Cc, miss, [0, 0, 0]) as g, hip.context(module="add", nrows=R, ncols=Cc, missingvalue=miss) as ctx:
        g.upload(bd, bw)
        g.run_block(300, 0.005 / 1000)
        with GroupPonds(g) as p, Ponds(ctx) as q:
            n = p.label_stage_curves(WET)
            t, s = p.stage_curves(), p.stage_curve_stats()
            water = g.download_water()
            _, _, ref_table, ref_stats = reference(bd, miss, water, WET)
            assert_same_curves(t, s, ref_table, ref_stats)
            ctx.upload(bd, water)
            assert q.label_curves(WET) == n >= 1 and q.curves().tobytes() == t.tobytes()
            assert s["stage_cells"] > 0 and p.guard_bad() == 0 and q.guard_bad() == 0
