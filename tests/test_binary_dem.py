"""DEMs that were binary all along - Float32 rasters written with all their digits, float -> double through the C ABI - stream as
verified 32-bit codes on the grid 2^-s of their lowest set bit (wdpm_dem_codes.hip::encode_dem, after the decimal grids 10^-e have
failed).  Results can never depend on the codes, so every case here also proves from the options (WDPM_OPT_DEM32, _DEM_GRID,
_DEM_GRID_EXP) and from the launch ledger - the third template argument of fused_iteration_kernel, the relay kernel's last - that
a code-streaming instantiation ran; what the device must find comes from the numpy model (tests/binary_dem_model.py,
held against exact arithmetic by tests/test_binary_dem_model.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import wdpm_amd
from binary_dem_model import MISS, edge_cases, f32, f32_keep_nodata, largest_group_span, model_grid
from conftest import ROOT
from helpers import find_drain, n_bit_diff, pad, random_case
from test_pair_iterations import FORCED, expected_launches, iter2_launches

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import strip_timing  # noqa: E402

OPT_DEM16 = wdpm_amd.capi.OPT_DEM16
MARCH, RELAY, TRI = "fused_iteration_kernel", "relay_iteration_kernel", "tri_iteration_kernel"
ORACLE_CLI = os.path.join(ROOT, "oracle", "_build", "WDPMCL_oracle")
HIP_CLI = os.path.join(ROOT, "wdpm_amd", "bin", "WDPMCL")


def template_args(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")]


def dem_levels(delta, family=MARCH, arg=2):
    """the DEM argument of the iteration kernels of `family` among the ledger entries `delta` names"""
    return {template_args(n)[arg] for n in delta if n.startswith(family + "<")}


def ledger_delta(lib, before):
    after, _ = lib.launch_ledger()
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


class Oracle:
    """the oracle's answers, computed once per key and left alone"""

    def __init__(self):
        self.kept = {}

    def get(self, key, make):
        if key not in self.kept:
            self.kept[key] = make()
        return self.kept[key]


@pytest.fixture(scope="module")
def answers():
    return Oracle()


@pytest.fixture(scope="module")
def table():
    return edge_cases()


def play(ctx, bd, bw, td0, script):
    ctx.upload(bd, bw)
    ctx.totaldrain = td0
    out = []
    for kind, n in script:
        out.append(ctx.run_block(n, 1e-5) if kind == "block" else ctx.iterate(n))
    return out, ctx


def on_the_marching_kernel(hip, oracle, answers, key, module, dem, water, script, dem32, dem16=0, chunk=12):
    """one module on the marching kernel (a chunk height of the caller's keeps every launch on it) against the oracle: 0 differing
    bits, the grid the model names, and the ledger's word on which DEM the launches streamed.  Returns the ledger's levels."""
    bd, bw = pad(dem, water, MISS)
    R, C = dem.shape
    kw = dict(module=module, nrows=R, ncols=C, missingvalue=MISS)
    td0 = 0.0
    if module == "drain":
        dr, dc = find_drain(bd)
        td0 = max(bw[dr, dc], 0.0)
        kw.update(drainrow=dr, draincol=dc)

    def reference():
        with oracle.context(**kw) as o:
            obs, _ = play(o, bd, bw, td0, script)
            return obs, o.download_water(), o.totaldrain, o.drain_stats() if module == "drain" else None
    want = answers.get(key, reference)
    grid, exp, info = model_grid(dem[dem > MISS])
    before, _ = hip.launch_ledger()
    with hip.context(kernel=wdpm_amd.KERNEL_FUSED, chunk_rows=chunk, **kw) as g:
        g.upload(bd, bw)
        found = (g.get_option(wdpm_amd.OPT_DEM_GRID), g.get_option(wdpm_amd.OPT_DEM_GRID_EXP))
        assert found == (grid, exp), (key, found, (grid, exp), info)
        assert g.get_option(wdpm_amd.OPT_DEM32) == int(grid != 0)
        g.set_option(wdpm_amd.OPT_DEM32, dem32)                       # 2: the codes on launches of any size, honoured only after the check
        g.set_option(OPT_DEM16, dem16)
        assert g.get_option(wdpm_amd.OPT_DEM32) == int(grid != 0 and dem32 != 0)
        assert (g.get_option(wdpm_amd.OPT_DEM_GRID), g.get_option(wdpm_amd.OPT_DEM_GRID_EXP)) == found      # what upload found, not what runs
        have16 = g.get_option(OPT_DEM16)
        g.totaldrain = td0
        obs = [g.run_block(n, 1e-5) if kind == "block" else g.iterate(n) for kind, n in script]
        got = (obs, g.download_water(), g.totaldrain, g.drain_stats() if module == "drain" else None)
    nd = n_bit_diff(got[1], want[1])
    assert nd == 0, f"{key}: {nd} cells differ from the oracle"
    assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3], key
    levels = dem_levels(ledger_delta(hip, before))
    streaming = grid != 0 and dem32 != 0
    assert levels == ({"2"} if streaming and have16 else {"1"} if streaming else {"0"}), (key, levels, have16)
    return levels, have16


# ---------------------------------------------------------------------------------------------------------------------------------
# which DEMs the device accepts on a binary grid (40 x 230, 4 % NODATA) - and that results never depend on it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dem32", [2, 0])
@pytest.mark.parametrize("name", list(edge_cases()))
def test_binary_grid_edge_cases(hip, oracle, answers, table, name, dem32):
    dem = table[name]
    rng = np.random.default_rng(6)
    water = np.where(dem > MISS, 0.2 * rng.random(dem.shape), 0.0)
    on_the_marching_kernel(hip, oracle, answers, name, "add", dem, water, [("iter", 12)], dem32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the modules and the kernel families on a Float32-sourced DEM, 60 x 400
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("module", ["add", "subtract", "drain"])
def test_modules_on_the_marching_kernel_with_codes_on_a_binary_grid(hip, oracle, answers, module):
    dem, water, _ = random_case(77, 60, 400)
    if module == "drain":                                             # NODATA above, below and to the right of the outlet
        r0, c0 = 30, 200
        dem[r0, c0] = 480.0
        dem[r0 - 1, c0] = MISS
        dem[r0 + 1, c0 - 1:c0 + 2] = MISS
        dem[r0 - 1:r0 + 2, c0 + 1] = MISS
        dem[r0, c0 - 1], dem[r0 - 1, c0 - 1] = 485.5, 485.6
        water = np.where(dem > MISS, water, 0.0)
    dem = f32_keep_nodata(dem)
    grid, exp, _ = model_grid(dem[dem > MISS])
    assert grid == 2                                                  # the four-decimal DEM went through Float32: no decimal grid holds it
    if module == "drain":
        assert find_drain(pad(dem, water, MISS)[0]) == (31, 201)
    levels, _ = on_the_marching_kernel(hip, oracle, answers, "modules-" + module, module, dem, water, [("iter", 9), ("block", 16)], 2)
    assert levels == {"1"}


CHILD_CASES = {
    # the relay kernel, eight-wave workgroups: the only ones of its instantiations that stream codes
    "relay-add": dict(module="add", shape=(60, 400), level="codes32", source="random", seed=77,
                      script=[("block", 1), ("block", 4), ("iter", 3)]),
    # the triangle kernel reads the fp64 DEM whatever upload found: the grid must be reported, the bits must be the oracle's
    "tri-add": dict(module="add", shape=(60, 400), level="codes32", source="random", seed=77,
                    script=[("block", 1), ("block", 4), ("iter", 3)]),
    # two-iteration launches, as tests/test_pair_iterations.py's block scripts
    "iter2-one-group": dict(module="add", shape=(300, 678), level="codes16", tiles=0,
                            script=[("block", 2), ("block", 3), ("block", 4), ("block", 5), ("iter", 3), ("block", 20)]),
    "iter2-group-and-a-half": dict(module="add", shape=(301, 1010), level="codes32", tiles=0, patches=True,
                                   script=[("block", 2), ("block", 3), ("block", 4), ("block", 5), ("block", 21)]),
}
RELAY_ENV = dict(WDPM_RELAY="2", WDPM_RELAY_DEM32="1", WDPM_RELAY_NW="8")
TRI_ENV = dict(WDPM_TRI="2", WDPM_RELAY="0")


def run_child(env, names, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(HERE, "binary_dem_worker.py"), *names], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, f"{env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for n in names:
        assert n in out, f"no result for {n}\n{p.stderr[-3000:]}"
        assert out[n]["ok"], f"{n} {env}: {out[n]['error']}"
        assert out[n]["grids"] and all(g[0] == 2 and 1 <= g[1] <= 52 and g[2] == 1 for g in out[n]["grids"]), (n, out[n]["grids"])
    return out


@pytest.mark.gpu
def test_relay_kernel_streams_codes_of_a_binary_grid(hip):
    r = run_child(RELAY_ENV, ["relay-add"])["relay-add"]
    assert dem_levels(r["delta"], RELAY, 4) == {"true"}, sorted(r["delta"])
    assert r["grids"][0][:2] == [2, 15]


@pytest.mark.gpu
def test_triangle_kernel_on_a_dem_with_a_binary_grid(hip):
    r = run_child(TRI_ENV, ["tri-add"])["tri-add"]
    assert any(n.startswith(TRI + "<") for n in r["delta"]) and not any(n.startswith(RELAY + "<") for n in r["delta"]), sorted(r["delta"])
    assert r["grids"][0][:2] == [2, 15]


# ---------------------------------------------------------------------------------------------------------------------------------
# 16-bit offsets on a binary grid, 60 x 400
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("terrain", ["gentle", "rough"])
def test_16_bit_offsets_on_a_binary_grid(hip, oracle, answers, terrain):
    import coverage_worker as cw
    R, C = 60, 400
    if terrain == "gentle":
        dem, water = cw.make_case(R, C, R * 7 + C)
        dem = f32_keep_nodata(dem)
    else:
        rng = np.random.default_rng(11)
        dem = f32(500 + rng.normal(0, 3, (R, C)))
        water = 0.2 * rng.random((R, C))
    grid, exp, _ = model_grid(dem[dem > MISS])
    assert (grid, exp) == (2, 15)
    span = largest_group_span(pad(dem, water, MISS)[0], grid, exp)
    fits = span <= 65534                                              # dem16_encode_kernel's bound: 0xFFFF is NODATA
    assert fits == (terrain == "gentle"), span
    for want16 in (1, 0):
        levels, have16 = on_the_marching_kernel(hip, oracle, answers, "dem16-" + terrain, "add", dem, water, [("iter", 7), ("block", 5)], 2,
                                                dem16=want16)
        assert have16 == int(bool(want16) and fits)
        assert levels == ({"2"} if want16 and fits else {"1"})


# ---------------------------------------------------------------------------------------------------------------------------------
# two iterations per launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_iteration_launches_on_a_binary_grid(hip):
    names = ["iter2-one-group", "iter2-group-and-a-half"]
    res = run_child(FORCED, names, timeout=400)
    for n in names:
        two, one = iter2_launches(res[n])
        assert two > 0 and (two, one) == expected_launches(CHILD_CASES[n]["script"]), (n, two, one)


# ---------------------------------------------------------------------------------------------------------------------------------
# row blocks: every slab finds its own grid
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_row_blocks_each_find_a_binary_grid(hip, oracle):
    import ctypes as C

    from wdpm_amd.rowblock import Group, partition

    def accepted(n):
        try:
            partition(oracle, n, 3, 2)
            return True
        except ValueError:
            return False
    R = next(n for n in range(1, 2000) if accepted(n))                # the smallest raster three ranks take at exchange_every = 2
    Cc = 230
    dem, water, _ = random_case(41, R, Cc)
    dem = f32_keep_nodata(dem)
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as g:
        g.upload(bd, bw)
        assert g.get_option(wdpm_amd.OPT_DEM_GRID) == 2
        one = [g.run_block(n, 1e-5) for n in (7, 6)], g.download_water()
    with Group(hip, "add", R, Cc, MISS, [0, 0, 0], exchange_every=2) as grp:
        assert grp.size == 3 and grp.halo_kind == wdpm_amd.HALO_PEER
        grp.upload(bd, bw)
        slabs = partition(hip, R, 3, 2)
        for i in range(3):
            v = [C.c_int64(), C.c_int64(), C.c_int64()]
            for key, out in zip((wdpm_amd.OPT_DEM_GRID, wdpm_amd.OPT_DEM_GRID_EXP, wdpm_amd.OPT_DEM32), v):
                hip.check(hip.dll.wdpm_get_option(grp.rank_ctx(i), key, C.byref(out)))
            rows = bd[slabs[i].row0:slabs[i].row0 + slabs[i].rows]
            assert (v[0].value, v[1].value) == model_grid(rows[rows > MISS])[:2] and v[0].value == 2 and v[2].value == 1, (i, [x.value for x in v])
        mds = [grp.run_block(n, 1e-5) for n in (7, 6)]
        w = grp.download_water()
    assert mds == one[0] and n_bit_diff(w, one[1]) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def write_f32_dem(path, R=60, Cc=400):
    dem, _, _ = random_case(77, R, Cc)
    dem = f32_keep_nodata(dem)
    with open(path, "w") as f:
        f.write(f"ncols {Cc}\nnrows {R}\nxllcorner 0\nyllcorner 0\ncellsize 10\nNODATA_value -99999\n")
        np.savetxt(f, dem, fmt="%.17g")                               # more than 15 digits go to strtod: read back exactly
    return dem


def cli(exe, args, cwd, **env):
    p = subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stderr
    return p


ADD = ["add", "dem.asc", "NULL", "a.asc", "NULL", "100", "1.0", "1.0", "0", "0", "0.005", "1000"]
DRAIN = ["drain", "dem.asc", "a.asc", "d.asc", "NULL", "1.0", "1.0", "0", "0", "0.005", "1000"]


def test_cli_says_how_the_dem_is_streamed_only_when_asked(tmp_path):
    """host plumbing on the oracle back-end (no codes there): one line per row block on stderr with WDPM_REPORT_BACKEND=1, nothing new
    without it, and stdout keeps exactly one extra line"""
    write_f32_dem(tmp_path / "dem.asc", 60, 60)
    quiet = cli(ORACLE_CLI, ADD, tmp_path)
    assert "DEM:" not in quiet.stderr and "Computation back-end" not in quiet.stdout
    loud = cli(ORACLE_CLI, ADD, tmp_path, WDPM_REPORT_BACKEND="1", WDPM_DEVICES="0,0", WDPM_EXCHANGE_EVERY="2")
    assert [ln for ln in loud.stderr.splitlines() if " DEM: " in ln] == ["WDPMCL: block 0 DEM: fp64", "WDPMCL: block 1 DEM: fp64"]
    extra = [ln for ln in loud.stdout.splitlines() if ln not in quiet.stdout.splitlines()]
    assert len([ln for ln in extra if "Computation back-end:" in ln]) == 1
    assert strip_timing("\n".join(ln for ln in loud.stdout.splitlines() if "Computation back-end:" not in ln)) == strip_timing(quiet.stdout)


@pytest.mark.gpu
def test_hip_cli_on_a_float32_dem_written_with_all_digits(tmp_path, hip):
    dem = write_f32_dem(tmp_path / "dem.asc")
    grid, s, _ = model_grid(dem[dem > MISS])
    assert grid == 2
    # forced onto every launch, the codes travel as 16-bit offsets wherever the terrain allows them: the model says whether it does
    bits = 16 if largest_group_span(pad(dem, np.zeros_like(dem), MISS)[0], grid, s) <= 65534 else 32
    hdir, odir = tmp_path / "hip", tmp_path / "oracle"
    for d in (hdir, odir):
        d.mkdir()
        shutil.copy(tmp_path / "dem.asc", d / "dem.asc")
    marching = dict(WDPM_REPORT_BACKEND="1", WDPM_RELAY="0", WDPM_TRI="0", WDPM_DEM32="2")     # a raster this small: the codes forced
    for args, out in ((ADD, "a.asc"), (DRAIN, "d.asc")):
        h = cli(HIP_CLI, args, hdir, **marching)
        o = cli(ORACLE_CLI, args, odir, WDPM_REPORT_BACKEND="1")
        lines = [ln for ln in h.stderr.splitlines() if " DEM: " in ln]
        assert lines == [f"WDPMCL: block 0 DEM: {bits}-bit codes on the grid 2^-{s} m"], h.stderr
        assert len([ln for ln in h.stdout.splitlines() if "Computation back-end:" in ln]) == 1
        body = lambda p: strip_timing("\n".join(ln for ln in p.stdout.splitlines() if "Computation back-end:" not in ln))  # noqa: E731
        assert body(h) == body(o), args[0]
        assert open(hdir / out, "rb").read() == open(odir / out, "rb").read(), args[0]
    h = cli(HIP_CLI, ADD, hdir, **dict(marching, WDPM_DEM_BINARY="0"))
    assert [ln for ln in h.stderr.splitlines() if " DEM: " in ln] == ["WDPMCL: block 0 DEM: fp64"], h.stderr
    assert open(hdir / "a.asc", "rb").read() == open(odir / "a.asc", "rb").read()
    quiet = cli(HIP_CLI, ADD, hdir)
    assert " DEM: " not in quiet.stderr and "Computation back-end" not in quiet.stdout
