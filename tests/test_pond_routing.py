"""The pond routing on the device (include/wdpm_pond_routing.h, wdpm_amd/csrc/wdpm_pond_routing.hip) against the host model
(tests/pond_routing_model.py: the ponds one after another in decreasing hops, itself held against hand-written answers and a brute
force in tests/test_pond_routing_model.py).

Every case compares the WHOLE routing table and the totals for equality - every result is an integer, there is no tolerance; asserts
the invariants of tests/pond_routing_model.assert_invariants on the device's own tables; holds the launches the call reports against
the level sizes; holds every older table of the same call, the spill table included, bit for bit against a label_spills() of a twin
context; and asserts that no guard byte around the handle's buffers changed.  The grounds are those of tests/pond_spill_scenes.py;
each family first asserts ON THE MODEL that its ground gives the level sizes it is named for.

A run of narrow levels is one workgroup that reads, after a block barrier, words other waves have added to: only these exact
comparisons show that it reads them fresh.  WDPM_ROUTE_NARROW and WDPM_ROUTE_RUN_LEVELS, read when a handle is made, bring every
path within reach of few ponds."""
import numpy as np
import pytest

import pond_spill_scenes as scenes
from helpers import find_drain, pad, rough_dem
from pond_routing_model import (PLAN_STATS, STATS, assert_invariants, assert_same_routing, level_sizes, plan_of, routing_of_tables,
                                runoff_q_of)
from pond_spills_model import assert_same_spills
from test_pond_spills import reference as spill_reference

pytestmark = pytest.mark.gpu
MISS = scenes.MISS
WET = 0.001
THRES = 0.005 / 1000
MM = 0.001
TOP = 255.0
_ROUTES = {}


def model(bd, miss, water, md, tol, runoff_m):
    """(routing table, totals, spill table, spill counts, the four older tables) of the model: computed once per case"""
    spill_table, spill_stats, tables = spill_reference(bd, miss, water, md, tol)
    key = (id(spill_table), runoff_m)
    if key not in _ROUTES:
        _ROUTES[key] = routing_of_tables(spill_table, tables, runoff_q_of(runoff_m))
    return _ROUTES[key] + (spill_table, spill_stats, tables)


def bounds(env):
    return int(env.get("WDPM_ROUTE_NARROW", 256)), int(env.get("WDPM_ROUTE_RUN_LEVELS", 65536))


def hold_against_model(bd, miss, water, md, tol, runoff_m, p, n, env, whole=True):
    """the routing table and its totals of handle p against the model of the same water; `whole` False: a table whose model would
    walk for minutes is held against the invariants alone, which leave one table only.  Returns (table, stats)."""
    table, stats = p.routing(), p.routing_stats()
    spills, ponds, catch, out = p.spills(), p.table(), p.catchments(), p.outlets()
    values = ponds["cells"] + catch["catch_cells"]
    assert n == len(table) == stats["ponds"] and stats["runoff_q"] == runoff_q_of(runoff_m) >= 0
    if whole:
        ref_table, ref_stats, ref_spills, ref_spill_stats, ref = model(bd, miss, water, md, tol, runoff_m)
        # the inputs first, so that a difference below is the routing pass's own
        assert_same_spills(spills, p.spill_stats(), ref_spills, ref_spill_stats)
        assert (values == ref["ponds"]["cells"] + ref["catchments"]["catch_cells"]).all() and (out["fill_q"] == ref["outlets"]["fill_q"]).all()
        assert_same_routing(table, stats, ref_table, ref_stats)
    assert_invariants(table, stats, spills, values, out["fill_q"])
    launches = plan_of(level_sizes(spills), *bounds(env))
    assert stats["levels"] == (int(spills["hops"].max()) + 1 if n else 0)
    assert stats["launches"] == len(launches) and stats["wide_levels"] == sum(l[0] == "wide" for l in launches)
    assert set(stats) == set(STATS) | set(PLAN_STATS)
    return table, stats


def older(p):
    """what a label_spills() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.outlets(), p.curves(), p.spills()


def routing_on_device(hip, monkeypatch, bd, bw, runoffs, md=WET, tol=0.0, env=None, whole=None):
    """Upload padded rasters, label with routing at runoffs[0] and rerun at the others on ONE handle made under `env`; hold every
    table against the model and everything else the call leaves against the label_spills() of a twin context.  Returns the
    (table, stats) of every runoff."""
    from wdpm_amd.ponds import ROUTE_DTYPE, Ponds
    env = env or {}
    whole = whole or [True] * len(runoffs)
    for name in ("WDPM_ROUTE_NARROW", "WDPM_ROUTE_RUN_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    kw = dict(module="add", nrows=R, ncols=Cc, missingvalue=MISS)
    got = []
    with hip.context(**kw) as ctx, hip.context(**kw) as twin:
        ctx.upload(bd, bw)
        twin.upload(bd, bw)
        water = ctx.download_water()
        with Ponds(ctx) as p, Ponds(twin) as q:
            for i, runoff_m in enumerate(runoffs):
                if i == 0:
                    n = p.label_routing(md, runoff_m, tol)
                else:
                    p.route(runoff_m)
                assert p.routing().dtype == ROUTE_DTYPE
                got.append(hold_against_model(bd, MISS, water, md, tol, runoff_m, p, n, env, whole[i]))
            assert q.label_spills(md, tol) == n
            for mine, theirs in zip(older(p), older(q)):
                assert mine.tobytes() == theirs.tobytes()
            assert p.spill_stats() == q.spill_stats() and p.curve_stats() == q.curve_stats() and p.outlet_stats() == q.outlet_stats()
            assert p.guard_bad() == 0 and q.guard_bad() == 0
    return got


def padded(dem, water):
    return pad(np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(water, dtype=np.float64)), MISS)


def check(hip, monkeypatch, dem, water, runoffs, claim=None, **kw):
    """`claim(sizes, spill table, {runoff: (table, stats)})` is asserted on the model before the device is asked"""
    bd, bw = padded(dem, water)
    if claim is not None:
        md, tol = kw.get("md", WET), kw.get("tol", 0.0)
        whole = kw.get("whole") or [True] * len(runoffs)
        routes = {r: model(bd, MISS, bw, md, tol, r)[:2] for r, w in zip(runoffs, whole) if w}
        spill_table = spill_reference(bd, MISS, bw, md, tol)[0]
        claim(level_sizes(spill_table), spill_table, routes)
    return routing_on_device(hip, monkeypatch, bd, bw, runoffs, **kw)


def kinds(sizes, narrow=256, run_levels=65536):
    return [l[0] for l in plan_of(sizes, narrow, run_levels)]


# ---- chains -------------------------------------------------------------------------------------------------------------------------
def test_a_staircase_of_bowls_at_three_runoffs(hip, monkeypatch):
    """5 x 285: a chain of 95 ponds, 95 levels in one run of one workgroup; 1 mm overflows only the bowls that stand at their pass"""
    def claim(sizes, spills, routes):
        assert sizes == [1] * 95 and kinds(sizes) == ["run"]
        over = [routes[r][1]["overflowing"] for r in (MM, 0.05, 1.0)]
        assert 0 < over[0] < over[1] <= over[2] and over[0] < 94 <= over[2]
        assert routes[1.0][0]["reach_ponds"].max() >= 94 and 1 < routes[MM][0]["reach_ponds"].max() < 10
    got = check(hip, monkeypatch, *scenes.staircase(), (MM, 0.05, 1.0), claim)
    assert [s["launches"] for _, s in got] == [1, 1, 1] and got[0][1]["levels"] == 95


@pytest.mark.parametrize("env,launches", [({}, 1), ({"WDPM_ROUTE_RUN_LEVELS": 100}, 67)])
def test_a_column_of_6667_ponds(hip, monkeypatch, env, launches):
    """3 columns x 20001 rows: one chain of 6667 levels - one run, or 67 runs of at most 100 levels.  At 10 mm every fifth pond holds
    what the four above it pass on; at 1 m every pond overflows and the last one carries the whole column: that table is held
    against the invariants alone (the model's upstream walks would take 22 million steps)."""
    def claim(sizes, spills, routes):
        assert sizes == [1] * 6667 and len(plan_of(sizes, *bounds(env))) == launches
        t, s = routes[0.01]
        assert 4000 < s["overflowing"] < 6000 and t["reach_ponds"].max() == 5 and (t["in_q"] > 0).sum() > 4000
    got = check(hip, monkeypatch, *scenes.column(), (0.01, 1.0), claim, env=env, whole=[True, False])
    t, s = got[1]
    assert s["launches"] == launches and s["overflowing"] >= 6666 and t["reach_ponds"].max() >= 6666
    assert int(t["in_q"].max()) > 6000 * int(t["own_q"].min()) > 0


# ---- hubs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,plan", [({}, ["wide", "run"]), ({"WDPM_ROUTE_NARROW": 8}, ["wide", "run"])])
def test_a_hub_at_runoffs_that_let_none_some_and_all_pits_overflow(hip, monkeypatch, env, plan):
    """5 x 385: 384 pits round one lake, a level wider than one workgroup before a narrow one"""
    def claim(sizes, spills, routes):
        assert sizes[1] >= 384 > 256 and sizes[0] < 8 and kinds(sizes, *bounds(env)) == plan
        lake = int(np.argmax(spills["up_ponds"]))
        pits = spills["next"] == lake + 1
        over = [int(routes[r][0]["overflows"][pits].sum()) for r in (0.0, MM, TOP)]
        assert over[0] == 0 and 100 < over[1] < over[2] == int(pits.sum()) >= 384
        assert routes[MM][0]["reach_ponds"][lake] == 1 + over[1] and routes[TOP][1]["out_land_q"] > 0
    check(hip, monkeypatch, *scenes.hub(), (0.0, MM, TOP), claim, env=env)


@pytest.mark.parametrize("scene,sizes_are,narrow,plan", [
    ("cascade", [2, 96, 71, 70], 8, ["wide", "wide", "wide", "run"]), ("cascade", [2, 96, 71, 70], 80, ["run", "wide", "run"]),
    ("cascade", [2, 96, 71, 70], 256, ["run"]), ("ring_through_a_hub", [2, 11, 121], 8, ["wide", "wide", "run"]),
    ("ring_through_a_hub", [2, 11, 121], 16, ["wide", "run"]), ("ring_through_a_hub", [2, 11, 121], 256, ["run"])])
def test_hubs_of_hubs_with_small_workgroups(hip, monkeypatch, scene, sizes_are, narrow, plan):
    """pits into lakes into lakes.  WDPM_ROUTE_NARROW=8 makes every level of pits and lakes a launch of its own: a hub's words are
    read in the launch after its feeders'.  A bound between the level sizes puts wide and narrow levels in turn - the cascade's two
    levels of 70 and 71 ponds become one run in front of the wide level of 96 - and the default walks every level in one run: then a
    hub's words are read in the same launch as its feeders, behind a block barrier."""
    env = {"WDPM_ROUTE_NARROW": narrow} if narrow != 256 else {}
    def claim(sizes, spills, routes):
        assert sizes == sizes_are and kinds(sizes, narrow) == plan
        if scene == "cascade":
            assert routes[TOP][0]["reach_ponds"].max() > 200 and (routes[MM][0]["in_q"] > 0).sum() >= 4
        else:
            assert (spills["next"] == -2).sum() == 2 and routes[TOP][1]["out_ring_q"] > 0
        assert 0 < routes[MM][1]["overflowing"] < routes[TOP][1]["overflowing"]
    check(hip, monkeypatch, *getattr(scenes, scene)(), (MM, 0.3, TOP), claim, env=env)


# ---- rings, ends, one pond, no pond -----------------------------------------------------------------------------------------------------
def test_a_mutual_pair_and_a_ring_of_three_leave_at_the_head(hip, monkeypatch):
    def claim(sizes, spills, routes):
        assert spills["next"][0] == -2 and routes[1.0][1]["out_ring_q"] > 0 and routes[1.0][1]["out_land_q"] == 0
        assert routes[1.0][0]["out_q"][0] == routes[1.0][1]["out_ring_q"]
    got = check(hip, monkeypatch, *scenes.pair(), (1.0,), claim)
    assert got[0][0]["level"].tolist() == [0, 1] and got[0][0]["reach_ponds"].tolist() == [2, 1]
    got = check(hip, monkeypatch, *scenes.ring_of_three(), (1.0, 0.0), claim)
    assert got[0][0]["level"].tolist() == [0, 2, 1] and got[0][0]["reach_ponds"].tolist() == [3, 1, 2] and got[1][1]["out_ring_q"] == 0


def test_ends_on_land_and_without_an_outlet(hip, monkeypatch):
    def claim(sizes, spills, routes):
        t, s = routes[TOP]
        assert spills["next"].tolist() == [0, -1] and s["out_land_q"] == int(t["out_q"][0]) > 0 and s["out_ring_q"] == 0
        assert t["out_q"][1] == 0 and t["kept_q"][1] == t["own_q"][1] > 0 and t["full"].tolist() == [1, 0]
    check(hip, monkeypatch, *scenes.ends(), (TOP, MM), claim)


def test_one_pond_and_no_pond(hip, monkeypatch):
    dem = 50.0 + np.add.outer(np.arange(20.0) - 10, np.arange(30.0) - 15) ** 2 / 64.0
    (t, s), = check(hip, monkeypatch, dem, np.zeros((20, 30)), (0.01,))
    assert len(t) == 0 and s == dict(ponds=0, runoff_q=runoff_q_of(0.01), levels=0, wide_levels=0, launches=0, overflowing=0, full=0, own_q=0,
                                     kept_q=0, out_land_q=0, out_ring_q=0)
    water = np.where(dem < 50.2, 0.01, 0.0)
    (t, s), (t2, s2) = check(hip, monkeypatch, dem, water, (0.01, TOP), lambda sizes, sp, r: sizes == [1] or pytest.fail("one pond"))
    assert len(t) == 1 and s["levels"] == s["launches"] == 1 and t["reach_ponds"][0] == 1 and s2["own_q"] == 255 * 2 ** 24 * int(t["reach_cells"][0])


# ---- the threshold --------------------------------------------------------------------------------------------------------------------
def test_a_leaf_pond_filled_exactly_and_one_quantum_more(hip, monkeypatch):
    """the first bowl of the staircase, which nothing feeds: runoff_q = fill_q // area keeps everything, one quantum more overflows"""
    bd, bw = padded(*scenes.staircase())
    spill_table, _, tables = spill_reference(bd, MISS, bw, WET, 0.0)
    area = int(tables["ponds"]["cells"][0] + tables["catchments"]["catch_cells"][0])
    fill = int(tables["outlets"]["fill_q"][0])
    q = fill // area
    assert spill_table["hops"][0] == 94 and spill_table["up_ponds"][0] == 1 and fill > area and 0 < q < 2 ** 32 - 1
    runoffs = (q * 2.0 ** -24, (q + 1) * 2.0 ** -24)
    assert [runoff_q_of(r) for r in runoffs] == [q, q + 1]
    (t0, _), (t1, _) = routing_on_device(hip, monkeypatch, bd, bw, runoffs)
    assert t0["overflows"][0] == 0 and t0["out_q"][0] == 0 and t0["full"][0] == int(q * area == fill)
    assert t1["overflows"][0] == 1 and int(t1["out_q"][0]) == (q + 1) * area - fill and t1["full"][0] == 1


# ---- noise, real water ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, monkeypatch, density):
    """the three waters of tests/test_pond_spills.py, each at 1 mm and at 255 m"""
    R, Cc = 131, 385
    rng = np.random.default_rng(int(density * 100))
    dem = rough_dem(R, Cc, int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    def claim(sizes, spills, routes):
        assert sum(sizes) > (256 if density < 0.5 else 32) and len(sizes) >= 2
        assert routes[MM][1]["overflowing"] <= routes[TOP][1]["overflowing"] == int((spills["next"] != -1).sum())
        assert (routes[TOP][0]["reach_ponds"] == spills["up_ponds"]).all() and (routes[TOP][0]["reach_cells"] == spills["up_cells"]).all()
    check(hip, monkeypatch, dem, water, (MM, TOP), claim)


@pytest.mark.parametrize("module", ["add", "drain"])
def test_real_water(hip, monkeypatch, module):
    """two blocks of real iterations, then the routing of that water against the model, with reruns"""
    from wdpm_amd.ponds import Ponds
    for name in ("WDPM_ROUTE_NARROW", "WDPM_ROUTE_RUN_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    dem = hip.synth_dem(385, 131)[:131, :385].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    kw = dict(module=module, nrows=131, ncols=385, missingvalue=MISS)
    if module == "drain":
        dr, dc = find_drain(bd)
        kw.update(drainrow=dr, draincol=dc)
    with hip.context(**kw) as ctx:
        ctx.upload(bd, bw)
        ctx.totaldrain = 0.0
        ctx.run_block(100, THRES)
        ctx.run_block(100, THRES)
        water = ctx.download_water()
        with Ponds(ctx) as p:
            n = p.label_routing(WET, 0.01, 0.001)
            assert n >= 1
            hold_against_model(bd, MISS, water, WET, 0.001, 0.01, p, n, {})
            p.route(0.1)
            hold_against_model(bd, MISS, water, WET, 0.001, 0.1, p, n, {})
            assert p.guard_bad() == 0
        assert (ctx.download_water() == water).all()                                     # the water is not the routing's to change


def test_basin5(hip, monkeypatch, basin5):
    """basin5 after an add of 300 mm and 300 iterations: 10 mm and 100 mm of runoff against the model"""
    from wdpm_amd.ponds import Ponds
    for name in ("WDPM_ROUTE_NARROW", "WDPM_ROUTE_RUN_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    dem, hdr = basin5
    miss = hdr["NODATA_value"] if "NODATA_value" in hdr else hdr[[k for k in hdr if k.lower().startswith("nodata")][0]]
    R, Cc = dem.shape
    bd, _ = pad(dem, np.zeros_like(dem), miss)
    bw = np.where(bd > miss, 0.3, 0.0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=miss) as ctx:
        ctx.upload(bd, bw)
        ctx.run_block(300, THRES)
        water = ctx.download_water()
        with Ponds(ctx) as p:
            n = p.label_routing(WET, 0.01, 0.001)
            hold_against_model(bd, miss, water, WET, 0.001, 0.01, p, n, {})
            p.route(0.1)
            hold_against_model(bd, miss, water, WET, 0.001, 0.1, p, n, {})
            assert n >= 1 and p.guard_bad() == 0


# ---- the handle -----------------------------------------------------------------------------------------------------------------------
def test_handle_state(hip, monkeypatch):
    import wdpm_amd
    from wdpm_amd.ponds import ROUTE_DTYPE, Ponds, bind
    for name in ("WDPM_ROUTE_NARROW", "WDPM_ROUTE_RUN_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    bd, bw = padded(*scenes.bowls(67, 193, 12))
    dll = bind(hip)
    kw = dict(module="add", nrows=67, ncols=193, missingvalue=MISS)
    runoffs = (0.05, 2.0, MM, 0.0, 0.3)
    with hip.context(**kw) as ctx, hip.context(**kw) as other:
        ctx.upload(bd, bw)
        other.upload(bd, bw)
        with Ponds(ctx) as p, Ponds(other) as fresh:
            with pytest.raises(wdpm_amd.WdpmError, match="Ponds.routing: label_routing\\(\\) has not succeeded"):
                p.routing()
            with pytest.raises(wdpm_amd.WdpmError, match="no routing table"):           # nothing labelled yet
                p.route(0.01)
            n = p.label_spills(WET, 0.01)
            for ask in (p.routing, p.routing_stats, lambda: p.route(0.01)):             # a spill table is no routing table
                with pytest.raises(wdpm_amd.WdpmError, match="no routing table"):
                    ask()
            assert p.label_routing(WET, runoffs[0], 0.01) == n >= 8
            spills = p.spills().tobytes()
            # five reruns in non-monotone order: each is the model's table, and a fresh handle's label call at that depth
            for r in runoffs[1:] + runoffs[:1]:
                p.route(r)
                table, stats = hold_against_model(bd, MISS, bw, WET, 0.01, r, p, n, {})
                assert fresh.label_routing(WET, r, 0.01) == n
                assert fresh.routing().tobytes() == table.tobytes() and fresh.routing_stats() == stats
                assert p.spills().tobytes() == spills
            want, stats = table, stats
            assert stats["overflowing"] > 0
            # a refused depth leaves every table in place
            for bad in (-0.001, float("nan"), 256.0, float("inf")):
                with pytest.raises(wdpm_amd.WdpmError, match="wdpm_route_rerun: runoff_m"):
                    p.route(bad)
                assert p.routing().tobytes() == want.tobytes() and p.routing_stats() == stats and p.spills().tobytes() == spills
                with pytest.raises(wdpm_amd.WdpmError, match="wdpm_route_label: runoff_m"):
                    p.label_routing(WET, bad, 0.01)
                p.n = n                                                                 # the binding forgets n when a label call fails
                assert p.routing().tobytes() == want.tobytes() and p.spills().tobytes() == spills
            for md, tol in ((float("nan"), 0.0), (-1.0, 0.0), (WET, float("nan")), (WET, -1.0)):
                with pytest.raises(wdpm_amd.WdpmError, match="wdpm_route_label"):
                    p.label_routing(md, 0.01, tol)
            p.n = n
            buf = np.full(n * ROUTE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_route_table(p._h, buf.ctypes.data, n - 1) != 0              # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_route_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                                  # ... and writes nothing
            assert dll.wdpm_route_table(p._h, buf.ctypes.data, n) == 0 and buf.tobytes() == want.tobytes()
            assert p.routing(capacity=n + 7).tobytes() == want.tobytes()
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.routing_phase_ms()
            # every lesser label call takes the routing table away, and a rerun has nothing to stand on
            for call in (p.label, p.label_curves, lambda md: p.label_spills(md, 0.01)):
                assert call(WET) == n
                for ask in (p.routing, p.routing_stats, lambda: p.route(0.01)):
                    with pytest.raises(wdpm_amd.WdpmError, match="no routing table"):
                        ask()
                assert p.label_routing(WET, runoffs[0], 0.01) == n and p.routing().tobytes() == want.tobytes() and p.routing_stats() == stats
            assert p.label_routing(5.0, 0.01) == 0 and len(p.routing()) == 0            # no pond at this threshold: an empty table
            p.route(0.5)
            assert len(p.routing()) == 0 and p.routing_stats()["runoff_q"] == runoff_q_of(0.5)
            assert p.guard_bad() == 0 and fresh.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import ROUTE_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    bd, bw = padded(*scenes.staircase())
    with hip.context(module="add", nrows=5, ncols=285, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            assert p.label_routing(WET, 0.05) == 95
            ms = p.routing_phase_ms()
            assert tuple(ms) == ROUTE_PHASES == ("order", "sweep", "finish") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.spill_phase_ms()) == {"rings", "chains", "sums"} and len(p.phase_ms()) == 6
            p.route(1.0)
            ms = p.routing_phase_ms()
            assert ms["order"] == 0 and 0 < ms["sweep"] < 1000 and 0 < ms["finish"] < 1000, ms
            assert p.guard_bad() == 0
