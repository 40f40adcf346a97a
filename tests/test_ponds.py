"""The pond inventory on the device (include/wdpm_ponds.h, wdpm_amd/csrc/wdpm_ponds.hip) against the host model
(tests/ponds_model.py, itself held against hand-written answers and scipy in tests/test_ponds_model.py).

Every case compares the WHOLE label raster and the WHOLE table for equality - the definition is exact, there is no tolerance -
and asserts that no guard byte around the handle's buffers changed and that the cells of all ponds at min_depth = 0.001 add up to
the wet count of Context.count_stats.  Shapes are the smallest at which each mechanism can fail: a wave owns a 64-column
segment of one row and a block four of them; widths are file columns, so the padded width is two more.  The table kernel
carries sums down the rows one wave owns, but only rasters of more than 32 768 segments give a wave more than one row: the
cases up to 1000 x 1500 run it with one, and the tests under "rows per wave" below run it with more - by size, and forced
through WDPM_PONDS_ROWS_PER_WAVE on small patterns.

Run as a script (`python tests/test_ponds.py <oracle.npz>`) this file is the child process of the state-neutrality test: the same
flow under whatever switches the parent put into the environment.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

from helpers import find_drain, n_bit_diff, pad  # noqa: E402
from ponds_model import assert_same, inventory  # noqa: E402

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001          # the reference's wet threshold (m): what Context.count_stats counts


def inventory_on_device(hip, bd, bw, thresholds=(WET,), module="add", rows_per_wave=None, **kw):
    """Upload padded rasters, label at each threshold on ONE handle and hold everything against the model.  Returns the stats of
    the first threshold."""
    from wdpm_amd.ponds import Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    first = None
    with hip.context(module=module, nrows=R, ncols=Cc, missingvalue=MISS, **kw) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            for md in thresholds:
                n = p.label(md)
                labels, table, stats = p.labels(), p.table(), p.stats()
                water = ctx.download_water()
                ref_labels, ref_table = inventory(bd > MISS, water, md)
                assert n == len(ref_table) == stats["ponds"], (n, len(ref_table), stats)
                assert_same(labels, table, ref_labels, ref_table)
                assert stats["segments"] == (R + 2) * ((Cc + 2 + 63) // 64) and stats["passes"] == 0
                if rows_per_wave is not None:
                    assert stats["rows_per_wave"] == rows_per_wave, stats
                if md == WET:
                    assert int(table["cells"].sum()) == ctx.count_stats()[1]
                first = first or stats
            assert p.guard_bad() == 0
    return first


def flat_dem(R, Cc, nodata=None):
    dem = np.full((R, Cc), 100.0)
    if nodata is not None:
        dem[nodata] = MISS
    return dem


def check_pattern(hip, water, nodata=None, thresholds=(WET,), rows_per_wave=None):
    bd, bw = pad(flat_dem(*water.shape, nodata), water, MISS)
    return inventory_on_device(hip, bd, bw, thresholds, rows_per_wave=rows_per_wave)


# ---- seams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", [(70, 200), (67, 193), (131, 385)])
def test_lines_across_every_seam(hip, R, Cc):
    """A full row, a full column and a corner-to-corner staircase: straight and diagonal links over every lane, wave and block
    boundary; depths differ along them, so sums and maxima have to cross the seams too."""
    rng = np.random.default_rng(R)
    w = np.zeros((R, Cc))
    w[R // 3, :] = 1
    w[:, Cc // 3] = 1
    cols = [i * (Cc - 1) // (R - 1) for i in range(R)] + [Cc - 1]
    for i in range(R):
        w[i, cols[i]:cols[i + 1] + 1] = 1
    w *= 0.01 + rng.random((R, Cc))
    s = check_pattern(hip, w)
    assert s["seam_unions"] > 0 and s["unions"] > s["seam_unions"]
    # the same lines apart: a one-cell anti-diagonal that meets nothing else than diagonal neighbours
    w = np.zeros((R, Cc))
    for i in range(min(R, Cc)):
        w[i, Cc - 1 - i] = 0.5 + i
    assert check_pattern(hip, w)["ponds"] == 1


# ---- long chains ------------------------------------------------------------------------------------------------------------
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


def spiral(n):
    w = np.zeros((n, n))
    r = c = 0
    dr, dc = 0, 1
    w[0, 0] = 1
    while True:
        for _ in range(2):                       # straight on, else turn right once
            nr, nc, fr, fc = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < n and 0 <= nc < n and not w[nr, nc] and not (0 <= fr < n and 0 <= fc < n and w[fr, fc]):
                r, c = nr, nc
                w[r, c] = 1
                break
            dr, dc = dc, -dr
        else:
            return w


@pytest.mark.parametrize("name", ["serpentine", "comb", "spiral"])
def test_long_chains(hip, name):
    w = {"serpentine": lambda: serpentine(129, 130), "comb": lambda: comb(129, 130), "spiral": lambda: spiral(101)}[name]()
    assert w.sum() > 5000
    w *= 0.002 + np.arange(w.size).reshape(w.shape) * 1e-5
    assert check_pattern(hip, w)["ponds"] == 1


# ---- many runs, many ponds --------------------------------------------------------------------------------------------------
def test_checkerboard_is_one_pond(hip):
    i, j = np.mgrid[0:65, 0:67]
    assert check_pattern(hip, np.where((i + j) % 2 == 0, 0.25, 0.0))["ponds"] == 1


def lattice(R, Cc):
    w = np.zeros((R, Cc))
    w[::2, ::2] = 0.5 + np.arange(((R + 1) // 2) * ((Cc + 1) // 2)).reshape((R + 1) // 2, (Cc + 1) // 2) * 2.0 ** -10
    return w


def test_isolated_cells_are_numbered_in_order(hip):
    assert check_pattern(hip, lattice(64, 66))["ponds"] == 1056


def test_table_capacity(hip):
    from wdpm_amd.ponds import POND_DTYPE, Ponds, bind
    R, Cc = 600, 700
    w = lattice(R, Cc)
    bd, bw = pad(flat_dem(R, Cc), w, MISS)
    dll = bind(hip)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            n = p.label(WET)
            assert n == 300 * 350
            ref_labels, ref_table = inventory(bd > MISS, bw, WET)
            buf = np.full(n * POND_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_ponds_table(p._h, buf.ctypes.data, n - 1) != 0          # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                              # ... and writes nothing
            assert dll.wdpm_ponds_table(p._h, buf.ctypes.data, n) == 0              # exact
            assert_same(p.labels(), buf.view(POND_DTYPE), ref_labels, ref_table)
            assert int(ref_table["cells"].sum()) == ctx.count_stats()[1]
            assert p.guard_bad() == 0


# ---- random noise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", [(257, 515), (1000, 1500)])
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, R, Cc, density):
    """below, in and above the 8-connected percolation region; 5 % NODATA with water on it; depths from subnormal to several metres, a few NaN"""
    rng = np.random.default_rng(int(density * 100) + R)
    depth = rng.random((R, Cc)) * 0.02
    kind = rng.random((R, Cc))
    depth[kind < 0.10] = 3.0 + 5.0 * rng.random(int((kind < 0.10).sum()))
    depth[kind > 0.95] = 5e-324 * rng.integers(1, 1 << 40, int((kind > 0.95).sum()))
    w = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    w[rng.random((R, Cc)) < 0.002] = np.nan                   # never a pond cell
    nodata = rng.random((R, Cc)) < 0.05
    # the second labelling on the same handle counts the subnormal depths in; at the small size only (the model is the slow side)
    s = check_pattern(hip, w, nodata, thresholds=(WET, 0.0) if R < 1000 else (WET,))
    assert s["ponds"] > 10
    if R >= 1000:
        assert s["seam_unions"] > 0


# ---- rows per wave: the table kernel's carry down the rows ----------------------------------------------------------------
def noise(R, Cc, density, seed):
    rng = np.random.default_rng(seed)
    w = np.where(rng.random((R, Cc)) < density, 0.002 + rng.random((R, Cc)) * 2.0, 0.0)
    return w, rng.random((R, Cc)) < 0.05


def test_rows_per_wave_by_size(hip):
    """More than 32 768 segments: the library itself gives a wave two rows.  Noise in the percolation region - labels change
    inside a wave's strip, so a carry is sent in mid-strip - and a tall all-wet raster: one label down every strip, whose row
    bounds and sums come from carries alone."""
    w, nodata = noise(1500, 1500, 0.41, 15)
    s = check_pattern(hip, w, nodata, rows_per_wave=2)
    assert s["segments"] == 1502 * 24 and s["ponds"] > 1000 and s["seam_unions"] > 0
    s = check_pattern(hip, 0.05 + np.random.default_rng(16).random((33000, 1)), rows_per_wave=2)
    assert s["segments"] == 33002 and s["ponds"] == 1


FORCED = {"all wet": lambda: 0.05 + np.random.default_rng(7).random((300, 700)),          # one label spans every strip
          "stripes": lambda: np.repeat(np.arange(1, 131)[:, None] % 2 * 0.5, 200, axis=1),   # a new pond on every other row
          "checkerboard": lambda: np.where(np.add.outer(np.arange(65), np.arange(67)) % 2 == 0, 0.25, 0.0),
          "lattice": lambda: lattice(64, 66),                                                # every run its own label
          "serpentine": lambda: serpentine(129, 130) * (0.002 + np.arange(129 * 130).reshape(129, 130) * 1e-5),
          "noise": lambda: noise(257, 515, 0.41, 8)}


@pytest.mark.parametrize("rpw", [2, 7, 64, 1000])
@pytest.mark.parametrize("name", list(FORCED))
def test_rows_per_wave_forced(hip, monkeypatch, name, rpw):
    """The same carry at sizes a test can afford: WDPM_PONDS_ROWS_PER_WAVE, read when the handle is made, gives every wave 2, 7
    (no divisor of any height here: the last strip is short), 64 or all rows (one strip per segment column).  Labels that
    alternate from row to row inside a strip, labels that alternate inside a row, and one label down the whole strip."""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    made = FORCED[name]()
    w, nodata = made if isinstance(made, tuple) else (made, None)
    s = check_pattern(hip, w, nodata, rows_per_wave=min(rpw, w.shape[0] + 2))
    assert s["rows_per_wave"] > 1


# ---- degenerate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cc", [(1, 1), (1, 300), (300, 1), (3, 5000)])
def test_thin_rasters(hip, R, Cc):
    rng = np.random.default_rng(R * Cc)
    assert check_pattern(hip, np.full((R, Cc), 0.5))["ponds"] == 1
    if R * Cc > 1:
        check_pattern(hip, np.where(rng.random((R, Cc)) < 0.5, rng.random((R, Cc)), 0.0), thresholds=(WET, 0.25))


def test_all_wet_and_all_dry(hip):
    from wdpm_amd.ponds import POND_DTYPE, Ponds
    R, Cc = 300, 700
    rng = np.random.default_rng(5)
    s = check_pattern(hip, 0.05 + rng.random((R, Cc)))
    assert s["ponds"] == 1 and s["unions"] >= (R - 1) * ((Cc + 2 + 63) // 64)
    bd, bw = pad(flat_dem(R, Cc), np.full((R, Cc), WET), MISS)        # exactly the threshold: dry
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            assert p.label(WET) == 0
            t = p.table()
            assert len(t) == 0 and t.dtype == POND_DTYPE
            assert not p.labels().any()
            assert ctx.count_stats()[1] == 0 and p.guard_bad() == 0
            assert p.label(0.0) == 1 and p.table()["cells"][0] == R * Cc


def test_a_depth_beyond_the_volume_range_fails_the_call(hip):
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    R, Cc = 20, 70
    w = np.full((R, Cc), 0.1)
    w[7, 66] = 600.0
    bd, bw = pad(flat_dem(R, Cc), w, MISS)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="512 m"):
                p.label(WET)
            with pytest.raises(wdpm_amd.WdpmError):
                p.table()
            with pytest.raises(wdpm_amd.WdpmError):
                p.label(float("inf"))
            assert p.label(700.0) == 0                 # above it the cell is dry, and the handle works on
            assert p.guard_bad() == 0


def test_slab_context_is_refused(hip):
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    with hip.context(module="add", nrows=40, ncols=50, missingvalue=MISS, slab_row0=0, slab_rows=21) as ctx:
        with pytest.raises(wdpm_amd.WdpmError, match="slab"):
            Ponds(ctx)


def test_a_context_closed_first_takes_its_handles_along(hip):
    """the C handle must go before its context: Context.close sees to it, and the late close of the handle is harmless"""
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    bd, bw = pad(flat_dem(5, 70), np.full((5, 70), 0.5), MISS)
    ctx = hip.context(module="add", nrows=5, ncols=70, missingvalue=MISS)
    ctx.upload(bd, bw)
    p = Ponds(ctx)
    assert p.label(WET) == 1
    ctx.close()
    assert p._h is None
    with pytest.raises(wdpm_amd.WdpmError):
        p.table()
    p.close()


# ---- real water, and the context is left as it was -------------------------------------------------------------------------
THRES = 0.005 / 1000


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


def oracle_third_block(oracle, hip, module):
    bd, bw, kw = real_case(hip, module)
    with oracle.context(**kw) as o:
        o.upload(bd, bw)
        o.totaldrain = 0.0
        o.run_block(100, THRES)
        o.run_block(100, THRES)
        md = o.run_block(100, THRES)
        return dict(max_diff=md, water=o.download_water(), totaldrain=o.totaldrain)


def neutrality(hip, module, want):
    """Two blocks; inventory (owed drain() of the drain module applied by the call); a third block with another inventory between
    begin_block and its first iteration (owed flush applied by the call).  The third block must be what a twin context computes that
    never took an inventory, and what the oracle computes."""
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
            n = p.label(WET)
            labels, table = p.labels(), p.table()
            water = a.download_water()
            assert_same(labels, table, *inventory(bd > MISS, water, WET))
            assert n >= 1 and int(table["cells"].sum()) == a.count_stats()[1]
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label(0.0)                          # every film counts: the block's threshold flush must have been applied
            labels, table = p.labels(), p.table()
            flushed = a.download_water()
            assert ((water > 0) & (flushed == 0)).any(), "no depth below the block's threshold: the flush would not show"
            a.iterate(100)
            md_a = a.max_diff()
            assert_same(labels, table, *inventory(bd > MISS, flushed, 0.0))
            assert n2 == len(table) and p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        wa, wb = a.download_water(), b.download_water()
        assert md_a == md_b == want["max_diff"], (md_a, md_b, want["max_diff"])
        assert n_bit_diff(wa, wb) == 0 and n_bit_diff(wa, want["water"]) == 0
        assert a.totaldrain == b.totaldrain == float(want["totaldrain"])
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0
    return n


@pytest.fixture(scope="module")
def oracle_add(oracle, hip):
    return oracle_third_block(oracle, hip, "add")


def test_state_neutrality_add(hip, oracle_add):
    neutrality(hip, "add", oracle_add)


def test_state_neutrality_marching_kernel(hip, oracle_add, tmp_path):
    """the same under WDPM_RELAY=0 WDPM_TRI=0: the marching kernel with its dry-tile flags, in a process of its own"""
    ref = tmp_path / "oracle_add.npz"
    np.savez(ref, **oracle_add)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(ref)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WDPM_RELAY="0", WDPM_TRI="0"))
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    assert json.loads(p.stdout.strip().splitlines()[-1])["ponds"] >= 1


def test_state_neutrality_drain(hip, oracle):
    neutrality(hip, "drain", oracle_third_block(oracle, hip, "drain"))


def test_basin5(hip, basin5):
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
            n = p.label(WET)
            labels, table = p.labels(), p.table()
            assert_same(labels, table, *inventory(bd > miss, ctx.download_water(), WET))
            assert n >= 1 and int(table["cells"].sum()) == ctx.count_stats()[1] and p.guard_bad() == 0


if __name__ == "__main__":
    import wdpm_amd
    os.environ.setdefault("WDPM_GUARD_KB", "64")
    z = np.load(sys.argv[1])
    n = neutrality(wdpm_amd.load_hip(), "add", dict(max_diff=float(z["max_diff"]), water=z["water"], totaldrain=float(z["totaldrain"])))
    print(json.dumps(dict(ponds=n)))
