"""The pond spills on the device (include/wdpm_pond_spills.h, wdpm_amd/csrc/wdpm_pond_spills.hip) against the host model
(tests/pond_spills_model.py: sequential walks, itself held against hand-written answers and a brute-force walk in
tests/test_pond_spills_model.py).

Every case compares the WHOLE spill table and the counts for equality - every result is an integer, there is no tolerance; asserts
the invariants of tests/pond_spills_model.assert_invariants on the device's own tables; holds labels, pond table, rim table, basin
raster, catchment table, outlet table and curve table of the same call, bit for bit, against a label_curves() of a twin context; and
asserts that no guard byte around the handle's buffers changed.  Each family first asserts ON THE MODEL that its ground gives the graph
it is named after - a DEM that fails to produce a ring cannot pass silently.  The kernels run one lane per pond: 64 ponds are one
wave, 256 one block.
"""
import hashlib

import numpy as np
import pytest

import pond_spill_scenes as scenes
from helpers import find_drain, n_bit_diff, pad, rough_dem
from pond_spills_model import assert_invariants, assert_same_spills, rounds_of, spills_of_water

pytestmark = pytest.mark.gpu
MISS = scenes.MISS
WET = 0.001
THRES = 0.005 / 1000
_REFERENCES = {}


def reference(bd, miss, water, md, tol):
    """(spill table, counts, the four older tables) of the model: computed once per water, threshold and tolerance"""
    key = hashlib.sha1(bd.tobytes() + np.ascontiguousarray(water).tobytes() + repr((bd.shape, miss, md, tol)).encode()).hexdigest()
    if key not in _REFERENCES:
        _REFERENCES[key] = spills_of_water(bd, miss, water, md, tol)
    return _REFERENCES[key]


def older(p):
    """what a label_curves() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.outlets(), p.curves()


def hold_against_model(bd, miss, water, md, tol, p, n):
    """the spill table and its counts of handle p against the model of the same water; returns (table, stats)"""
    table, stats = p.spills(), p.spill_stats()
    ref_table, ref_stats, ref = reference(bd, miss, water, md, tol)
    assert n == len(ref_table) == stats["ponds"] == len(table)
    ponds, rims, catch, out = p.table(), p.rims(), p.catchments(), p.outlets()
    # the inputs first, so that a difference below is the spill pass's own
    assert (ponds["cells"] == ref["ponds"]["cells"]).all() and (catch["catch_cells"] == ref["catchments"]["catch_cells"]).all()
    assert (out["to_basin"] == ref["outlets"]["to_basin"]).all() and (out["fill_q"] == ref["outlets"]["fill_q"]).all()
    assert out["pour_level"].view(np.uint64).tolist() == ref["outlets"]["pour_level"].view(np.uint64).tolist()
    assert rims["surface_max"].view(np.uint64).tolist() == ref["rims"]["surface_max"].view(np.uint64).tolist()
    assert_same_spills(table, stats, ref_table, ref_stats)
    assert_invariants(table, ponds["cells"] + catch["catch_cells"], out["fill_q"], out["pour_level"])
    assert stats["rounds"] == rounds_of(n) and stats["ends_ring"] == stats["rings"]
    return table, stats


def spills_on_device(hip, bd, bw, calls=((WET, 0.0),)):
    """Upload padded rasters, label with spills at each (threshold, tolerance) on ONE handle, hold the spill table against the model
    and everything else the call leaves against the label_curves() of a twin context.  Returns what the last call left."""
    from wdpm_amd.ponds import SPILL_DTYPE, Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    kw = dict(module="add", nrows=R, ncols=Cc, missingvalue=MISS)
    with hip.context(**kw) as ctx, hip.context(**kw) as twin:
        ctx.upload(bd, bw)
        twin.upload(bd, bw)
        with Ponds(ctx) as p, Ponds(twin) as q:
            for md, tol in calls:
                n = p.label_spills(md, tol)
                assert p.spills().dtype == SPILL_DTYPE
                got = hold_against_model(bd, MISS, ctx.download_water(), md, tol, p, n)
                assert q.label_curves(md) == n
                for mine, theirs in zip(older(p), older(q)):
                    assert mine.tobytes() == theirs.tobytes()
                assert p.catchment_stats() == q.catchment_stats() and p.outlet_stats() == q.outlet_stats() and p.curve_stats() == q.curve_stats()
            assert p.guard_bad() == 0
    return got


def padded(dem, water):
    return pad(np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(water, dtype=np.float64)), MISS)


def check(hip, dem, water, claim=None, **kw):
    """`claim(table, stats, tables)` is asserted on the model before the device is asked"""
    bd, bw = padded(dem, water)
    if claim is not None:
        for md, tol in kw.get("calls", ((WET, 0.0),)):
            claim(*reference(bd, MISS, bw, md, tol))
    return spills_on_device(hip, bd, bw, **kw)


# ---- chains -------------------------------------------------------------------------------------------------------------------------
def test_a_staircase_of_bowls(hip):
    """5 x 285: a chain of 95 ponds, across two waves of the table; two in three stand at their pass"""
    def claim(t, s, tables):
        assert s["ponds"] == 95 and s["max_hops"] >= 70 and s["rings"] == 0 and 0 < s["spilling"] < 95
        assert (t["next"][:94] == np.arange(2, 96)).all() and t["hops"][0] == 94 and t["up_ponds"][94] == 95
        assert t["rest_hops"].max() >= 2 and t["live_ponds"].max() >= 3
    dem, water = scenes.staircase()
    assert dem.shape == (5, 285)
    t, s = check(hip, dem, water, claim)
    assert t["sink"].tolist() == [95] * 95 and s["rounds"] == 3 * 8


def test_a_column_of_6667_ponds(hip):
    """3 columns x 20001 rows, one pond every three rows down the slope: one chain of 6666 hops, 14 rounds to a pass"""
    def claim(t, s, tables):
        assert s["ponds"] >= 5000 and s["max_hops"] >= 5000 and s["rounds"] >= 3 * 13 and s["rings"] == 0
        assert s["max_hops"] == s["ponds"] - 1 and 0 < s["spilling"] < s["ponds"]
    dem, water = scenes.column()
    assert dem.shape == (20001, 3)
    t, s = check(hip, dem, water, claim)
    assert s["rounds"] == 42 and t["hops"][0] == 6666 and t["up_ponds"][-1] == 6667


def test_a_hub(hip):
    """5 x 385: 384 pits spill over their rims into one lake, every second one already does; the lake leaves onto land"""
    def claim(t, s, tables):
        lake = int(np.argmax(tables["ponds"]["cells"])) + 1
        assert int((t["next"] == lake).sum()) >= 130 and t["next"][lake - 1] == 0
        assert t["up_ponds"][lake - 1] >= 131 and 65 <= t["live_ponds"][lake - 1] < t["up_ponds"][lake - 1]
    t, s = check(hip, *scenes.hub(), claim)
    assert s["max_hops"] == 1 and s["ends_land"] >= 1


# ---- rings ----------------------------------------------------------------------------------------------------------------------------
def test_a_mutual_pair(hip):
    def claim(t, s, tables):
        assert tables["outlets"]["to_basin"].tolist() == [2, 1] and s["rings"] == 1 and s["ring_ponds"] == 2
    t, s = check(hip, *scenes.pair(), claim)
    assert t["next"].tolist() == [-2, 1] and t["end"].tolist() == [-2, -2] and t["up_ponds"].tolist() == [2, 1]


def test_a_ring_of_three_made_with_tied_passes(hip):
    def claim(t, s, tables):
        out = tables["outlets"]
        assert out["to_basin"].tolist() == [2, 3, 1] and len(set(out["pour_level"].tolist())) == 1
        assert s["rings"] == 1 and s["ring_ponds"] == 3
    t, s = check(hip, *scenes.ring_of_three(), claim)
    assert t["next"].tolist() == [-2, 3, 1] and t["sink"].tolist() == [1, 1, 1] and t["hops"].tolist() == [0, 2, 1]
    assert t["up_ponds"].tolist() == [3, 1, 2]


def test_bowls_with_tied_passes(hip):
    """131 x 385, ground in steps of 1/8 m: 348 ponds in two blocks of the table, mutual pairs among them, chains of eight, about
    half of the ponds spilling"""
    def claim(t, s, tables):
        assert s["ponds"] > 256 and s["rings"] >= 3 and s["max_hops"] >= 5 and s["ponds"] // 4 < s["spilling"] < 3 * s["ponds"] // 4
        assert (t["rest_hops"] >= 2).any() and (t["live_ponds"] < t["up_ponds"]).any() and (t["live_ponds"] > 1).any()
    check(hip, *scenes.bowls(131, 385, 3), claim)


# ---- ends, one pond, no pond ------------------------------------------------------------------------------------------------------------
def test_ends_on_land_and_without_an_outlet(hip):
    def claim(t, s, tables):
        assert tables["outlets"]["to_basin"].tolist() == [0, -1] and s["ends_land"] == 1 and s["ends_none"] == 1
    t, s = check(hip, *scenes.ends(), claim)
    assert t["end"].tolist() == [0, -1] and t["sink"].tolist() == [1, 2] and t["spilling"].tolist() == [0, 0]


def test_one_pond_and_no_pond(hip):
    none = dict(ponds=0, rings=0, ring_ponds=0, spilling=0, ends_land=0, ends_none=0, ends_ring=0, max_hops=0, rounds=0)
    dem = 50.0 + np.add.outer(np.arange(20.0) - 10, np.arange(30.0) - 15) ** 2 / 64.0
    t, s = check(hip, dem, np.zeros((20, 30)))
    assert len(t) == 0 and s == none
    water = np.where(dem < 50.2, 0.01, 0.0)
    t, s = check(hip, dem, water, lambda t, s, tables: s["ponds"] == 1 or pytest.fail("one pond"))
    assert len(t) == 1 and t["next"][0] in (0, -1) and t["up_ponds"][0] == 1 and s["rounds"] == 3


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("below,tol,spilling", [(0, 0.0, 1), (1, 0.0, 0), (0, 0.001, 1), (1, 0.001, 1), (2 ** 15, 0.001, 0)])
def test_filled_to_the_pour_level_and_one_quantum_below(hip, below, tol, spilling):
    """a pond filled exactly to its pour level, one quantum of 2^-24 m below it, and 2 mm below it, under tolerances of 0 and 1 mm"""
    def claim(t, s, tables):
        assert tables["outlets"]["pour_level"].tolist() == [12.0] and tables["rims"]["surface_max"].tolist() == [12.0 - below * 2.0 ** -24]
        assert s["spilling"] == spilling
    t, s = check(hip, *scenes.brim(below), claim, calls=((WET, tol),))
    assert t["spilling"].tolist() == [spilling] and t["rest"].tolist() == [1]


# ---- noise, real water ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, density):
    """water at three densities on rough ground, 3 % NODATA with water on it: from thousands of ponds down to forty as they merge;
    short chains, many ends, nearly every pond above its pass"""
    R, Cc = 131, 385
    rng = np.random.default_rng(int(density * 100))
    dem = rough_dem(R, Cc, int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    t, s = check(hip, dem, water, lambda t, s, tables: s["ponds"] > (256 if density < 0.5 else 32) or pytest.fail("too few ponds"))
    assert s["max_hops"] >= 1 and s["ends_land"] + s["ends_none"] + s["ends_ring"] > 5


def test_two_thresholds_and_two_tolerances_on_one_handle(hip):
    bd, bw = padded(*scenes.bowls(67, 193, 12))
    calls = ((WET, 0.0), (WET, 0.25), (0.3, 0.0), (0.3, 0.25), (WET, 0.0))
    stats = [reference(bd, MISS, bw, md, tol)[1] for md, tol in calls[:3]]
    assert stats[0]["spilling"] < stats[1]["spilling"] < stats[1]["ponds"] and stats[2]["ponds"] != stats[0]["ponds"]
    spills_on_device(hip, bd, bw, calls=calls)


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
    """Two blocks of real iterations; spills against the model; a third block with another spill call between begin_block and its
    first iteration.  The third block is, bit for bit, what a twin context computes that never took an inventory."""
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
            n = p.label_spills(WET, 0.001)
            t, s = hold_against_model(bd, MISS, a.download_water(), WET, 0.001, p, n)
            assert n >= 1
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label_spills(0.0, 0.0)
            flushed = a.download_water()
            a.iterate(100)
            md_a = a.max_diff()
            hold_against_model(bd, MISS, flushed, 0.0, 0.0, p, n2)
            assert p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        assert md_a == md_b
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
        assert a.totaldrain == b.totaldrain
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0


def test_basin5(hip, basin5):
    """basin5 after an add of 300 mm and 300 iterations: the spill table against the model"""
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
            n = p.label_spills(WET, 0.001)
            t, s = hold_against_model(bd, miss, ctx.download_water(), WET, 0.001, p, n)
            assert n >= 1 and p.guard_bad() == 0


# ---- the handle -----------------------------------------------------------------------------------------------------------------------
def test_handle_state(hip):
    import wdpm_amd
    from wdpm_amd.ponds import SPILL_DTYPE, Ponds, bind
    R, Cc = 46, 70
    dem = rough_dem(R, Cc, 5)
    water = np.where(np.random.default_rng(5).random((R, Cc)) < 0.3, 0.3, 0.0)
    bd, bw = pad(dem, water, MISS)
    dll = bind(hip)
    none = dict(ponds=0, rings=0, ring_ponds=0, spilling=0, ends_land=0, ends_none=0, ends_ring=0, max_hops=0, rounds=0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="Ponds.spills: label_spills\\(\\) has not succeeded"):
                p.spills()
            with pytest.raises(wdpm_amd.WdpmError, match="no spill table"):             # nothing labelled yet
                p.n = 0
                p.spills(capacity=10)
            n = p.label_spills(WET, 0.01)
            want, stats = hold_against_model(bd, MISS, bw, WET, 0.01, p, n)
            assert n >= 4
            curves = p.curves().tobytes()
            for call in (p.label, p.label_rims, p.label_catchments, p.label_outlets, p.label_curves):
                assert call(WET) == n                                                   # each lesser label call takes the table away
                for ask in (p.spills, p.spill_stats):
                    with pytest.raises(wdpm_amd.WdpmError, match="no spill table"):
                        ask()
                assert p.label_spills(WET, 0.01) == n and p.spills().tobytes() == want.tobytes() and p.spill_stats() == stats
            assert p.curves().tobytes() == curves
            buf = np.full(n * SPILL_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_spill_table(p._h, buf.ctypes.data, n - 1) != 0              # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_spill_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                                  # ... and writes nothing
            assert dll.wdpm_spill_table(p._h, buf.ctypes.data, n) == 0
            assert buf.tobytes() == want.tobytes() and p.spills(capacity=n + 7).tobytes() == want.tobytes()
            for md, tol in ((float("nan"), 0.0), (-1.0, 0.0), (WET, float("nan")), (WET, -1.0), (WET, float("inf"))):
                with pytest.raises(wdpm_amd.WdpmError, match="wdpm_spill_label"):
                    p.label_spills(md, tol)
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.n = n
                p.spill_phase_ms()
            assert p.label_spills(5.0) == 0                                             # no pond at this threshold: an empty table
            assert len(p.spills()) == 0 and p.spill_stats() == none
            assert p.label_spills(WET, 0.01) == n and p.spills().tobytes() == want.tobytes()
            ctx.run_block(1, THRES)                                                     # the water moves on: a label call of the new
            assert p.label_curves(WET) >= 0                                             # water leaves no spill table either
            with pytest.raises(wdpm_amd.WdpmError, match="no spill table"):
                p.spills()
            n2 = p.label_spills(WET)
            hold_against_model(bd, MISS, ctx.download_water(), WET, 0.0, p, n2)
            assert p.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import SPILL_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    bd, bw = padded(*scenes.staircase())
    with hip.context(module="add", nrows=5, ncols=285, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            assert p.label_spills(WET) == 95
            ms = p.spill_phase_ms()
            assert tuple(ms) == SPILL_PHASES == ("rings", "chains", "sums") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.curve_phase_ms()) == {"bed", "stages"} and len(p.phase_ms()) == 6
            assert p.guard_bad() == 0
