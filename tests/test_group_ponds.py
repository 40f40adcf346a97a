"""The pond inventory over row blocks on the device (include/wdpm_group_ponds.h, wdpm_amd.ponds.GroupPonds): N ranks on one GPU
(devices = [0] * N, peer-copy halos), every rank labelled where its rows lie, against the host model
(tests/ponds_model.inventory) on the water the group itself downloads.  Every comparison is equality of the whole label raster
and the whole table; guard bands around every rank's buffers are looked at after every label call (the suite runs with
WDPM_GUARD_KB).  exchange_every = 1 unless stated: its halos are 2 and 4 rows, so eight ranks fit in 46 rows.  Shapes: one,
three and six 64-column segments per row, widths that are no multiple of 64."""
import numpy as np
import pytest

import group_ponds_cases as gc
from group_ponds_cases import MISS, WET, GroupCase, slabs_of
from helpers import find_drain, n_bit_diff, pad
from ponds_model import assert_same

pytestmark = pytest.mark.gpu
SHAPES = [(46, 70), (67, 193), (131, 385)]
RANKS = [2, 3, 8]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_lines_across_every_boundary(hip, R, Cc, n):
    with GroupCase(hip, R, Cc, [0] * n) as case:
        gc.run_lines(case, slabs_of(hip, R, n))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_joined_only_far_below_or_above(hip, R, Cc, n):
    """two arms and a comb joined by a bar in the last rank (then in rank 0): two, or many, local ponds per rank everywhere else,
    one pond in the whole; isolated cells after them in every rank, so every later number has to shift"""
    with GroupCase(hip, R, Cc, [0] * n) as case:
        gc.run_joined_far_away(case)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_in_and_out_of_a_rank(hip, R, Cc, n):
    """the transposed serpentine: one pond that crosses each boundary many times and joins different local ponds of one rank"""
    with GroupCase(hip, R, Cc, [0] * n) as case:
        s = case.check(gc.serpentine_transposed(R, Cc))
        teeth = (Cc + 1) // 2
        assert s["ponds"] == 1 and s["stitch_unions"] == (n - 1) * teeth and s["merged"] == s["local_ponds"] - 1, s
        assert s["local_ponds"] > n            # middle ranks see the columns as ponds of their own


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("n", RANKS)
def test_nothing_to_join(hip, R, Cc, n):
    slabs = slabs_of(hip, R, n)
    with GroupCase(hip, R, Cc, [0] * n) as case:
        s = case.check(gc.lattice(R, Cc))
        assert s["merged"] == 0 and s["stitch_unions"] == 0 and s["ponds"] == s["local_ponds"] == ((R + 1) // 2) * ((Cc + 1) // 2), s
        s = case.check(np.zeros((R, Cc)))
        assert s["ponds"] == 0 and not case.ponds.labels().any() and len(case.ponds.table()) == 0
        s = case.check(0.05 + np.random.default_rng(R).random((R, Cc)))
        assert s["ponds"] == 1 and s["local_ponds"] == n and s["merged"] == n - 1, s
        w = np.zeros((R, Cc))                                  # water only in the last rank
        w[slabs[-1].own_lo - 1 + 1:, 3:Cc - 2] = 0.2
        w[R - 1, 0] = 0.7
        s = case.check(w)
        assert s["ponds"] == 2 and s["merged"] == 0 and case.ponds.rank_stats(n - 1)["ponds"] == 2, s
        assert case.ponds.rank_stats(0)["ponds"] == 0
        # a NODATA band across the first boundary, with water on it that must be ignored: the ponds either side stay apart
        hi = slabs[0].own_hi - 1                               # file row of rank 0's last owned row
        nodata = np.zeros((R, Cc), dtype=bool)
        nodata[hi:hi + 2, :] = True
        s = case.check(np.full((R, Cc), 0.3), nodata)
        assert s["ponds"] == 2 and s["stitch_unions"] == s["merged"] == n - 2, s      # the other boundaries still join
        # a pond that ends in the seam row without crossing
        w = np.zeros((R, Cc))
        w[hi - 2:hi + 1, 5:Cc - 5] = 0.4
        w[hi + 2:hi + 4, 7:20] = 0.6
        s = case.check(w)
        assert s["ponds"] == 2 and s["stitch_unions"] == 0 and s["merged"] == 0, s


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RANKS)
def test_noise(hip, n):
    with GroupCase(hip, 131, 385, [0] * n) as case:
        gc.run_noise(case)


@pytest.mark.parametrize("n", [2, 5])
def test_noise_at_the_default_exchange_interval(hip, n):
    with GroupCase(hip, 257, 515, [0] * n, every=None) as case:
        gc.run_noise(case)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc,n", [(60, 1, 8), (46, 5000, 3)])
def test_thin_rasters(hip, R, Cc, n):
    rng = np.random.default_rng(R * Cc)
    with GroupCase(hip, R, Cc, [0] * n) as case:
        s = case.check(np.full((R, Cc), 0.5))
        assert s["ponds"] == 1 and s["merged"] == n - 1, s
        case.check(np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_one_handle_several_thresholds(hip):
    """the table and the maps have to grow and shrink"""
    w, nodata = gc.noise(131, 385, 0.41, 77)
    with GroupCase(hip, 131, 385, [0] * 3) as case:
        counts = [case.check(w, nodata, thresholds=(md,))["ponds"] for md in (0.05, 0.0, 0.001, 0.05, 0.0)]
        assert counts[0] == counts[3] and counts[1] == counts[4] and len(set(counts[:3])) == 3, counts


@pytest.mark.parametrize("rpw", [2, 7])
def test_rows_per_wave_forced(hip, monkeypatch, rpw):
    """WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made: the table kernel's carry down the rows, with the map in place"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    for n in (2, 8):
        with GroupCase(hip, 46, 70, [0] * n) as case:
            gc.run_joined_far_away(case)
            assert case.ponds.rank_stats(1)["rows_per_wave"] == rpw        # rank 1 labels 8 rows or more; rank 0 of eight only 6
    with GroupCase(hip, 131, 385, [0] * 3) as case:
        gc.run_noise(case, densities=(0.41,))
        assert all(case.ponds.rank_stats(i)["rows_per_wave"] == rpw for i in range(3))


def test_a_depth_beyond_the_volume_range_fails_the_call(hip):
    import wdpm_amd
    R, Cc, n = 46, 70, 3
    slabs = slabs_of(hip, R, n)
    w = np.full((R, Cc), 0.1)
    w[slabs[1].own_lo + 1, 66] = 600.0                         # in rank 1
    with GroupCase(hip, R, Cc, [0] * n) as case:
        bd, bw = pad(gc.flat_dem(R, Cc), w, MISS)
        case.grp.upload(bd, bw)
        p = case.ponds
        with pytest.raises(wdpm_amd.WdpmError, match="512 m"):
            p.label(WET)
        with pytest.raises(wdpm_amd.WdpmError):
            p.table()
        with pytest.raises(wdpm_amd.WdpmError, match="no inventory"):
            p.labels()
        with pytest.raises(wdpm_amd.WdpmError):
            p.label(float("inf"))
        assert p.label(700.0) == 0 and not p.labels().any()    # above it the cell is dry, and the handle works on
        assert p.guard_bad() == 0
        w[slabs[1].own_lo + 1, 66] = 0.1
        assert case.check(w)["ponds"] == 1


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def test_a_group_of_one_rank_equals_the_context_handle(hip):
    import types

    from wdpm_amd.ponds import Ponds
    w, nodata = gc.noise(67, 193, 0.41, 5)
    with GroupCase(hip, 67, 193, [0]) as case:
        s = case.check(w, nodata)
        assert s["ranks"] == 1 and s["merged"] == 0 and s["stitch_unions"] == 0
        labels, table = case.ponds.labels(), case.ponds.table()
        ctx = types.SimpleNamespace(lib=hip, _h=case.grp.rank_ctx(0), shape=case.grp.shape)
        with Ponds(ctx) as p:
            assert p.label(WET) == s["ponds"]
            assert_same(labels, table, p.labels(), p.table())
            assert p.stats()["unions"] == case.ponds.rank_stats(0)["unions"]


def test_closing_the_group_first_takes_its_handles_along(hip):
    import wdpm_amd
    from wdpm_amd.ponds import GroupPonds
    from wdpm_amd.rowblock import Group
    bd, bw = pad(gc.flat_dem(46, 70), np.full((46, 70), 0.5), MISS)
    grp = Group(hip, "add", 46, 70, MISS, [0, 0], exchange_every=1)
    grp.upload(bd, bw)
    p = GroupPonds(grp)
    assert p.label(WET) == 1
    grp.close()
    assert p._h is None
    with pytest.raises(wdpm_amd.WdpmError):
        p.table()
    p.close()


def test_phase_times_need_the_variable(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import PHASES
    with GroupCase(hip, 46, 70, [0, 0]) as case:
        case.check(np.full((46, 70), 0.5))
        with pytest.raises(wdpm_amd.WdpmError, match="WDPM_PONDS_TIMING"):
            case.ponds.phase_ms(0)
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    with GroupCase(hip, 46, 70, [0, 0]) as case:
        case.check(np.full((46, 70), 0.5))
        for i in range(2):
            ms = case.ponds.phase_ms(i)
            assert list(ms) == list(PHASES) and all(v >= 0 for v in ms.values())
        with pytest.raises(wdpm_amd.WdpmError, match="rank"):
            case.ponds.phase_ms(2)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------
def test_drain_module_owed_drain_and_state_neutrality(hip):
    """After one block of a drain group the last iteration's drain() is owed: the inventory equals the model on the water the group
    downloads, and a further block is bit for bit that of a twin group that took no inventory."""
    from wdpm_amd.ponds import GroupPonds
    from wdpm_amd.rowblock import Group
    thres = 0.005 / 1000
    dem = hip.synth_dem(700, 300)[:300, :].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    dr, dc = find_drain(bd)
    kw = dict(drainrow=dr, draincol=dc)
    with Group(hip, "drain", 300, 700, MISS, [0, 0, 0], **kw) as a, Group(hip, "drain", 300, 700, MISS, [0, 0, 0], **kw) as b:
        for g in (a, b):
            g.upload(bd, bw)
            g.set_totaldrain(0.0)
            g.run_block(100, thres)
        with GroupPonds(a) as p:
            s = gc.check_handle(a, p, bd > MISS, WET)
            assert s["ponds"] >= 1 and int(p.table()["cells"].sum()) == a.count_stats()[1], s
        md_a, md_b = a.run_block(100, thres), b.run_block(100, thres)
        assert md_a == md_b and a.totaldrain() == b.totaldrain()
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
