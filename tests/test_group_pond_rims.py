"""The pond rims over row blocks on the device (include/wdpm_group_pond_rims.h, wdpm_amd.ponds.GroupPonds.label_rims): N ranks on one
GPU (devices = [0] * N), every rank taking the rims of its own rows, against the host model (tests/pond_rims_model.rims) on the
labels the group returns, the water it downloads and the device's DEM.  Every comparison is equality - integers by value, doubles by
bit pattern - next to the labels and the pond table of the same call; guard bands are looked at after every call (the suite runs
with WDPM_GUARD_KB).  exchange_every = 1 unless stated.  Shapes are those of tests/test_group_ponds.py: one, three and six
64-column segments per row, widths that are no multiple of 64."""
import numpy as np
import pytest

import group_pond_rims_cases as rc
import group_ponds_cases as gc
from group_pond_rims_cases import RimCase, check_rims, ramp_dem
from group_ponds_cases import MISS, WET, slabs_of
from helpers import find_drain, n_bit_diff, pad
from pond_rims_model import assert_same_rims
from ponds_model import assert_same

pytestmark = pytest.mark.gpu
SHAPES = [(46, 70), (67, 193), (131, 385)]
RANKS = [2, 3, 8]


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_foreign_pond_with_its_lowest_rim_cell_across_the_boundary(hip, R, Cc, n):
    with RimCase(hip, R, Cc, [0] * n) as case:
        rc.run_foreign(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_counted_once_and_four_ponds_at_one_cell(hip, R, Cc, n):
    with RimCase(hip, R, Cc, [0] * n) as case:
        rc.run_counted_once_and_four_ponds(case, slabs_of(hip, R, n))


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_ties_across_ranks_signed_zeros_and_walls_only(hip, R, Cc, n):
    with RimCase(hip, R, Cc, [0] * n) as case:
        rc.run_ties(case, slabs_of(hip, R, n))
        rc.run_border_walls(case)


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_local_ponds_joined_through_another_rank_share_a_slot(hip, R, Cc, n):
    with RimCase(hip, R, Cc, [0] * n) as case:
        rc.run_shared_slots(case)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_one_pond_through_all_eight_ranks(hip, R, Cc):
    with RimCase(hip, R, Cc, [0] * 8) as case:
        rc.run_serpentine(case, slabs_of(hip, R, 8))


@pytest.mark.parametrize("n", RANKS)
def test_noise(hip, n):
    with RimCase(hip, 131, 385, [0] * n) as case:
        rc.run_noise(case)


@pytest.mark.parametrize("n", [2, 5])
def test_noise_at_the_default_exchange_interval(hip, n):
    with RimCase(hip, 257, 515, [0] * n, every=None) as case:
        rc.run_noise(case)


@pytest.mark.parametrize("R,Cc,n", [(60, 1, 8), (46, 5000, 3)])
def test_thin_rasters(hip, R, Cc, n):
    rng = np.random.default_rng(R * Cc)
    with RimCase(hip, R, Cc, [0] * n) as case:
        _, t, s, _ = case.check(np.full((R, Cc), 0.5))
        assert s["ponds"] == 1 and t["rim_cells"][0] == 0 and t["wall_cells"][0] == 2 * (R + Cc) + 4, (s, t)
        case.check(np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))


def test_an_empty_raster(hip):
    with RimCase(hip, 46, 70, [0] * 3) as case:
        _, t, s, rs = case.check(np.zeros((46, 70)))
        assert s["ponds"] == 0 and len(t) == 0 and rs["foreign"] == 0 and rs["slots"] == 0
        assert len(case.ponds.rims(capacity=0)) == 0
        _, t, s, _ = case.check(np.full((46, 70), 0.5))       # and the handle works on
        assert s["ponds"] == 1


@pytest.mark.parametrize("rpw", [2, 7])
def test_rows_per_wave_forced(hip, monkeypatch, rpw):
    """WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made: strips of rpw rows cut over each rank's owned rows, carries down them"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    for n in (2, 8):
        with RimCase(hip, 46, 70, [0] * n) as case:
            rc.run_shared_slots(case)
            rc.run_foreign(case, slabs_of(hip, 46, n))
            assert case.ponds.rank_stats(1)["rows_per_wave"] == rpw
    with RimCase(hip, 131, 385, [0] * 3) as case:
        rc.run_noise(case, densities=(0.41,))
        rc.run_counted_once_and_four_ponds(case, slabs_of(hip, 131, 3))


def test_against_the_whole_raster_answer_of_the_device(hip):
    """Ponds.label_rims on a context given the same DEM and the water the group downloads; and a group of one rank"""
    from wdpm_amd.ponds import Ponds
    R, Cc = 67, 193
    w, nodata = rc.noise(R, Cc, 0.41, 5)
    with RimCase(hip, R, Cc, [0] * 3) as case, RimCase(hip, R, Cc, [0]) as one:
        labels, t, s, rs = case.check(w, nodata=nodata)
        labels1, t1, s1, rs1 = one.check(w, nodata=nodata)
        assert s1["ranks"] == 1 and rs1["foreign"] == 0 and rs["foreign"] > 0
        water = case.grp.download_water()
        with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
            ctx.upload(case.bd, water)
            with Ponds(ctx) as p:
                assert p.label_rims(WET) == s["ponds"] == s1["ponds"]
                whole = p.rims()
                assert_same(labels, case.ponds.table(), p.labels(), p.table())
                assert p.guard_bad() == 0
        assert_same_rims(t, whole)
        assert_same_rims(t1, whole)
        assert (labels == labels1).all()


def test_handle_states(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import RIM_PHASES
    R, Cc = 46, 70
    w, nodata = rc.noise(R, Cc, 0.41, 9)
    with RimCase(hip, R, Cc, [0, 0]) as case:
        p = case.ponds
        with pytest.raises(wdpm_amd.WdpmError):
            p.rims()
        p.n = 0
        with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):
            p.rims()
        with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):
            p.rims_stats()
        labels, t, s, _ = case.check(w, nodata=nodata)
        table = p.table()
        assert p.label(WET) == s["ponds"]                      # a plain label takes the rim table away again
        with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):
            p.rims()
        assert_same(labels, table, p.labels(), p.table())      # ... and answers as the rim call did
        assert p.stats()["ponds"] == s["ponds"] and p.stats()["merged"] == s["merged"]
        assert p.label_rims(WET) == s["ponds"]
        assert_same_rims(p.rims(), t)
        with pytest.raises(wdpm_amd.WdpmError, match="capacity"):
            p.rims(capacity=s["ponds"] - 1)
        with pytest.raises(wdpm_amd.WdpmError, match="WDPM_PONDS_TIMING"):
            p.rims_phase_ms(0)
        with pytest.raises(wdpm_amd.WdpmError):
            p.label_rims(float("inf"))
        assert p.guard_bad() == 0
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    with RimCase(hip, R, Cc, [0, 0]) as case:
        case.check(w, nodata=nodata)
        for i in range(2):
            ms = case.ponds.rims_phase_ms(i)
            assert list(ms) == list(RIM_PHASES) and all(v >= 0 for v in ms.values())
        with pytest.raises(wdpm_amd.WdpmError, match="rank"):
            case.ponds.rims_phase_ms(2)
        case.ponds.label(WET)
        with pytest.raises(wdpm_amd.WdpmError, match="no rim table"):
            case.ponds.rims_phase_ms(0)


def test_the_whole_raster_call_still_refuses_a_row_block(hip):
    """wdpm_rims_label on a rank's context of a group of two: that context is a slab, and no handle of wdpm_ponds_create views it"""
    import types

    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    with RimCase(hip, 46, 70, [0, 0]) as case:
        ctx = types.SimpleNamespace(lib=hip, _h=case.grp.rank_ctx(0), shape=case.grp.shape)
        with pytest.raises(wdpm_amd.WdpmError, match="slab context"):
            Ponds(ctx)


@pytest.mark.parametrize("module", ["add", "drain"])
def test_state_neutrality(hip, module):
    """After a block of iterations (a drain group then owes the last iteration's drain()) the rims equal the model on the water the
    group downloads, and a further block is bit for bit that of a twin group that took no inventory."""
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
            _, t, s, _ = check_rims(a, p, bd, WET)
            assert s["ponds"] >= 1 and int(p.table()["cells"].sum()) == a.count_stats()[1], s
        md_a, md_b = a.run_block(100, thres), b.run_block(100, thres)
        assert md_a == md_b and a.totaldrain() == b.totaldrain()
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
