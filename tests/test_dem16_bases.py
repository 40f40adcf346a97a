"""The 16-bit DEM codes and their group bases (wdpm_kernels.h::DemCode::h, ::gb) in the marching loops, whose decoder leaves the
NODATA select out on steps whose wave holds no NODATA offset and runs the full form on the others (wdpm_march.hip::decode_rows,
wdpm_stencil.h::dem16_decode_nan).  Everything that streams 16-bit codes goes through that decoder: both roles of the
two-iteration loop (forced onto small rasters with WDPM_ITER2=2) and the single marching loop (WDPM_ITER2=0), played in child processes
(the switches are read once per process) with the 16-bit codes forced on launches of any size.

Every result is compared bit for bit with the oracle: the raster after 1, 2, 3 and 5 iterations on fresh water and after one block
of six iterations, with the block's max diff.  The oracle's results are computed once per module and handed to both children.

Shapes: 24 - 40 rows; 46, 47 and 48 columns, whose padded widths 48, 49 and 50 put a boundary between groups of 48 columns at the
row's end, one before it and one past it; 96 columns (two full groups); 700 columns (two groups of strips: producers and consumers on
both sides of a group seam).  DEMs: see make_dem."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from binary_dem_model import f32_keep_nodata
from helpers import pad

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MISS = -99999.0
THRES = 1e-5
GROUP = 48                      # wdpm_kernels.h::kDemGroup
LEDGER_ITER2 = 16
ITERATIONS, BLOCK = (1, 2, 3, 5), 6
WIDTHS = (46, 47, 48, 96, 700)
DEMS = ("below-zero", "relief-65534", "relief-65535", "float32", "no-nodata", "one-nodata", "nodata-first-column", "nodata-group")
FORCED = dict(WDPM_RELAY="0", WDPM_TRI="0")
KERNEL16 = "fused_iteration_kernel<0, false, 2, false, false, true>"
KERNEL32 = "fused_iteration_kernel<0, false, 1, false, false, true>"


def case_names():
    return [f"{d}-{w}" for d in DEMS for w in WIDTHS]


def case_shape(name):
    d, w = name.rsplit("-", 1)
    return 24 + (2 * DEMS.index(d) + 3 * WIDTHS.index(int(w))) % 17, int(w)


def group_columns(C, g):
    """unpadded columns of padded group g (padded columns 48 g .. 48 g + 47) inside the raster"""
    lo, hi = max(GROUP * g, 1), min(GROUP * g + GROUP, C + 1)
    return np.arange(lo - 1, hi - 1)


def make_dem(kind, R, C, seed):
    """(dem, water, missingvalue, what the upload must find: (grid, exponent or None, 16-bit codes in use)).
    The DEMs are quotients k / 10^e of integers, so the decimal grid e holds by construction and no coarser one does.
      below-zero           elevations near -1.0737e9 m on the 1e-6 grid: k0 as large in magnitude as |dem| < 2^30 allows at e = 6
      relief-65534         one group of one row spans exactly 65534 quanta: still 16-bit
      relief-65535         ... 65535 quanta: the 16-bit form is refused, the 32-bit codes run
      float32              a DEM that went through Float32: a binary grid
      no-nodata            no NODATA cell inside the raster at all: every interior step takes the select-free decode
      one-nodata           one NODATA cell mid-raster: consecutive steps of one wave take different decode paths
                           (this and the next two check the geometry of the bases; whether the gate in front of the select-free
                           decode can MISS a NODATA offset is tests/test_wave_gates.py's: here a miss would change no cell)
      nodata-first-column  NODATA in the first column of every group, on two rows
      nodata-group         a group that is NODATA throughout, on three rows"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:R, 0:C]
    k = 5_000_000 + np.rint(3000 * np.sin(x / 5.1) * np.cos(y / 3.3)).astype(np.int64) + rng.integers(0, 1000, (R, C)) - 20 * (x + y)
    k |= 1                                                        # no coarser decimal grid
    miss, want = MISS, (10, 4, True)
    g = 1 if C + 2 > 2 * GROUP else 0
    if kind == "below-zero":
        k = k - 5_000_000 - 1_073_741_000_000_000
        dem, miss, want = k / 1e6, -2.0e9, (10, 6, True)
        assert np.abs(dem).max() < 2.0 ** 30 and dem.max() < 0
    elif kind in ("relief-65534", "relief-65535"):
        cols = group_columns(C, g)
        span = 65534 if kind == "relief-65534" else 65535
        vals = np.concatenate(([0, span], rng.integers(1, span, len(cols) - 2)))
        k[R // 2, cols] = 4_990_001 + rng.permutation(vals)
        dem, want = k / 1e4, (10, 4, span == 65534)
    elif kind == "float32":
        dem, want = f32_keep_nodata(k / 1e4), (2, None, True)
    else:
        dem = k / 1e4
        if kind == "one-nodata":
            dem[R // 2, C // 2] = miss
        elif kind == "nodata-first-column":
            for gg in range(1, (C + 1) // GROUP + 1):
                if GROUP * gg - 1 < C:
                    dem[[R // 3, R // 2], GROUP * gg - 1] = miss
        elif kind == "nodata-group":
            cols = group_columns(C, g)
            dem[R // 2 - 1:R // 2 + 2, cols[0]:cols[-1] + 1] = miss
    valid = dem > miss
    water = np.where(valid & (rng.random((R, C)) >= 0.25), 0.3 * rng.random((R, C)), 0.0)
    return dem, water, miss, want


def build_case(name):
    R, C = case_shape(name)
    dem, water, miss, want = make_dem(name.rsplit("-", 1)[0], R, C, 1000 + case_names().index(name))
    bd, bw = pad(dem, water, miss)
    return dict(R=R, C=C, miss=miss, want=want, bd=bd, bw=bw)


def play(ctx, bw):
    """{step: raster}, the block's max diff: every step starts from the uploaded water"""
    out = {}
    for n in ITERATIONS:
        ctx.upload_water(bw)
        ctx.iterate(n)
        out[f"iter{n}"] = ctx.download_water()
    ctx.upload_water(bw)
    out["maxdiff"] = np.array([ctx.run_block(BLOCK, THRES)])
    out["block"] = ctx.download_water()
    return out


def test_shapes_and_dems_are_what_the_cases_say():
    assert all(24 <= case_shape(n)[0] <= 40 for n in case_names()) and len({case_shape(n)[0] % 3 for n in case_names()}) == 3
    for w in WIDTHS:
        c = build_case(f"relief-65534-{w}")
        q = np.rint(c["bd"][c["R"] // 2 + 1] * 1e4).astype(np.int64)
        g = 1 if w + 2 > 2 * GROUP else 0
        grp = q[GROUP * g:GROUP * g + GROUP]
        grp = grp[grp > MISS * 1e4]
        assert grp.max() - grp.min() == 65534
        c = build_case(f"nodata-group-{w}")
        assert (c["bd"][c["R"] // 2 + 1, GROUP * g:GROUP * g + GROUP] == MISS).all()
        c = build_case(f"no-nodata-{w}")
        assert (c["bd"][1:-1, 1:-1] > MISS).all()
    c = build_case("below-zero-96")
    assert 1.0737e15 < -np.rint(c["bd"][1:-1, 1:-1].min() * 1e6) < 2.0 ** 30 * 1e6


@pytest.fixture(scope="module")
def reference(oracle, tmp_path_factory):
    """inputs and the oracle's results of every case, in one file the children read"""
    arrays = {}
    for name in case_names():
        c = build_case(name)
        with oracle.context(module="add", nrows=c["R"], ncols=c["C"], missingvalue=c["miss"]) as o:
            o.upload(c["bd"], c["bw"])
            for key, a in play(o, c["bw"]).items():
                arrays[f"{name}/{key}"] = a
    path = str(tmp_path_factory.mktemp("dem16_bases") / "reference.npz")
    np.savez(path, **arrays)
    return path


def expected_launches(iter2):
    """(two-iteration launches, single gate-free launches) of play(): a block's first launch flushes, its last folds the max diff"""
    steady = list(ITERATIONS) + [BLOCK - 2]
    return (sum(s // 2 for s in steady), sum(s % 2 for s in steady)) if iter2 else (0, sum(steady))


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["two-iteration", "single"])
def test_marching_loops_on_16_bit_codes_match_the_oracle(hip, reference, loop):
    env = dict(os.environ, **FORCED, WDPM_ITER2="2" if loop == "two-iteration" else "0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "dem16_bases_worker.py"), reference, *case_names()], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    res = json.loads(p.stdout.strip().splitlines()[-1])
    failures = []
    for name in case_names():
        r = res.get(name)
        if r is None or not r["ok"]:
            failures.append(f"{name}: {r['error'] if r else 'no result'}")
            continue
        on16 = build_case(name)["want"][2]
        if bool(r["dem16"]) != on16:
            failures.append(f"{name}: WDPM_OPT_DEM16 reports {r['dem16']}, the 16-bit form must be {'in use' if on16 else 'refused'}")
        kernel, other = (KERNEL16, KERNEL32) if on16 else (KERNEL32, KERNEL16)
        two = sum(n for b, n in r["switches"].get(kernel, {}).items() if int(b) & LEDGER_ITER2)
        one = sum(n for b, n in r["switches"].get(kernel, {}).items() if not int(b) & LEDGER_ITER2)
        if (two, one) != expected_launches(loop == "two-iteration") or other in r["switches"]:
            failures.append(f"{name}: {two} two-iteration and {one} single launches of {kernel}, expected {expected_launches(loop == 'two-iteration')}"
                            f"{' - and launches on the other codes' if other in r['switches'] else ''}")
    assert not failures, "\n".join(failures)
