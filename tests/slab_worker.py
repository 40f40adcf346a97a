"""Machinery and child process of tests/test_marching_slabs.py: ONE slab context (or one group of slabs through the C driver)
against the oracle on the whole raster, at the bound of the halo rule (include/wdpm.h, wdpm_amd.rowblock.halo_depth).

After T iterations without a refresh a slab whose first row is 0 mod 3 (and whose live last row is 2 mod 3) holds the whole
raster's bits on the rows exact_rows() names: from 3T-1 where the top edge is live, up to rows-1-(6T-2) where the bottom edge is
live, every row towards an edge that is the raster's own border.  play_slab() runs a call script on both contexts and, after
every op, counts the cells that differ on those rows; for `block` and `overlap` ops the max diff is announced and read over the
same rows on both sides (never from row 0 of a slab with a live top: the reference seeds its maximum with diff[0][0]).

The parent imports play_slab() for its CPU tests (an oracle slab against the oracle's whole raster); as a child process this file
plays the named cases on the HIP library inside guard bands, with the WDPM_* switches of its environment (they are read once per
process), and prints one JSON line: {case: {"ok", "error", "delta", "switches", "seconds", "figures"}}.

    python tests/slab_worker.py <case> [<case> ...]"""
import ctypes as C
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import coverage_worker as cw  # noqa: E402  (sets the guard bands before the library is loaded)
import pair_worker as pw  # noqa: E402  (coverage_worker's raster with NODATA blocks, dry regions and deep water)
import wdpm_amd  # noqa: E402
from wdpm_amd import capi  # noqa: E402
from wdpm_amd.rowblock import Group  # noqa: E402
from helpers import n_bit_diff, pad  # noqa: E402

MISS, THRES = cw.MISS, cw.THRES


def raster(spec):
    """the padded DEM and water of a case: coverage_worker.make_case(R, C, seed R*7+C) with pair_worker's additions"""
    R, Cc = spec["shape"]
    pw._spec.clear()
    pw._spec.update(patches=spec.get("patches", False), deep=spec.get("deep", False))
    try:
        dem, water = pw.make_case(R, Cc, R * 7 + Cc)
    finally:
        pw._spec.clear()
    return pad(dem, water, MISS)


def exact_rows(R, r0, rows, T):
    """(first, last) slab-local row that holds the whole raster's bits T iterations after the upload"""
    lo = 3 * T - 1 if r0 > 0 else 0
    hi = rows - 1 - (6 * T - 2) if r0 + rows < R + 2 else rows - 1
    return lo, hi


def bits(v):
    return int(np.float64(v).view(np.uint64))


def force_codes(lib, handle, level):
    """what run_case does after the upload: the DEM as codes on launches of any size, no dry-tile flags - and the level in use"""
    def set_option(key, value):
        lib.check(lib.dll.wdpm_set_option(handle, key, value))

    def get_option(key):
        v = C.c_int64()
        lib.check(lib.dll.wdpm_get_option(handle, key, C.byref(v)))
        return v.value
    set_option(capi.OPT_DEM32, 2)
    set_option(capi.OPT_DEM16, 1 if level == "codes16" else 0)
    set_option(capi.OPT_TILES, 0)
    assert get_option(capi.OPT_DEM32) == 1, "the DEM did not pass the 32-bit code check"
    assert get_option(capi.OPT_DEM16) == int(level == "codes16"), "the 16-bit offsets are not in use"


def play_slab(slab_lib, oracle, spec, on_device=False):
    """the case's script on a slab context of `slab_lib` and on the oracle's whole raster; one record per op:
    (op, T, first and last exact row, cells that differ on them, cells that differ on the row above the first (None where the top
    edge is the raster's border), rows from the last exact row to the nearest differing row below it (None: none differs), the
    two max diffs as bit patterns (None for an `iter` op))"""
    R, Cc = spec["shape"]
    r0, rows = spec["slab"]
    assert r0 % 3 == 0 and r0 + rows <= R + 2 and (r0 + rows == R + 2 or rows % 3 == 0), "not a slab the partition makes"
    bd, bw = raster(spec)
    kw = dict(module=spec["module"], nrows=R, ncols=Cc, missingvalue=MISS)
    extra = dict(kernel=wdpm_amd.KERNEL_FUSED) if on_device else {}
    records = []
    with oracle.context(**kw) as full, slab_lib.context(**kw, slab_row0=r0, slab_rows=rows, **extra) as slab:
        full.upload(bd, bw)
        slab.upload(bd[r0:r0 + rows], bw[r0:r0 + rows])
        if on_device:
            force_codes(slab_lib, slab._h, spec["level"])
        T = 0
        for op in spec["script"]:
            kind, n = op[0], op[1]
            T += n
            lo, hi = exact_rows(R, r0, rows, T)
            assert 0 <= lo <= hi <= rows - 1, f"no exact row is left after {T} iterations"
            md = None
            if kind == "iter":
                full.iterate(n)
                slab.iterate(n)
            elif kind == "overlap_plain":                  # the split last iteration outside a block: nothing flushed, nothing folded
                full.iterate(n)
                slab.iterate_overlapped(n, op[2], op[3])
            elif kind in ("block", "overlap"):
                full.begin_block(THRES)
                full.iterate(n)
                slab.begin_block(THRES)
                slab.expect_max_diff(lo, hi + 1)
                if kind == "block":
                    slab.iterate(n)
                else:
                    slab.iterate_overlapped(n, op[2], op[3])
                md = (bits(slab.max_diff(lo, hi + 1)), bits(full.max_diff(r0 + lo, r0 + hi + 1)))
            else:
                raise ValueError(kind)
            got, want = slab.download_water(), full.download_rows(r0, rows)
            differs = (got.view(np.uint64) != want.view(np.uint64)).any(axis=1)
            below = np.nonzero(differs[hi + 1:])[0]
            records.append(dict(op=list(op), T=T, lo=lo, hi=hi, inside=n_bit_diff(got[lo:hi + 1], want[lo:hi + 1]),
                                above=n_bit_diff(got[lo - 1], want[lo - 1]) if r0 > 0 else None,
                                below=int(below[0]) + 1 if len(below) else None, md=md))
        bad = cw.guard_bad(slab_lib, slab) if on_device else 0
        assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
    return records


def check_exact(records):
    """every row the halo rule promises is the whole raster's, and so is the max diff over those rows"""
    for r in records:
        assert r["inside"] == 0, f"{r['op']}: {r['inside']} cells of rows {r['lo']}..{r['hi']} differ from the whole raster's after {r['T']} iterations"
        if r["md"] is not None:
            assert r["md"][0] == r["md"][1], f"{r['op']}: max diff over rows {r['lo']}..{r['hi']} {r['md'][0]:#x}, the whole raster's {r['md'][1]:#x}"


def run_group(hip, oracle, spec):
    """blocks through the C driver (wdpm_group_*: n slabs on one device, a refresh every k iterations) against ONE oracle context:
    the whole raster and every block's max diff"""
    R, Cc = spec["shape"]
    n, k = spec["ranks"], spec["k"]
    bd, bw = raster(spec)
    with oracle.context(module=spec["module"], nrows=R, ncols=Cc, missingvalue=MISS) as full:
        full.upload(bd, bw)
        want_md = [bits(full.run_block(b, THRES)) for b in spec["blocks"]]
        want = full.download_water()
    with Group(hip, spec["module"], R, Cc, MISS, [0] * n, exchange_every=k, kernel=wdpm_amd.KERNEL_FUSED) as g:
        kk = C.c_int32()
        hip.check(hip.dll.wdpm_rank_info(C.c_void_p(hip.dll.wdpm_group_rank(g._h, 0)), None, C.byref(kk), None))
        assert (g.size, kk.value) == (n, k), f"the driver made {g.size} slabs with a refresh every {kk.value} iterations"
        g.upload(bd, bw)
        for i in range(n):
            force_codes(hip, g.rank_ctx(i), spec["level"])
        got_md = [bits(g.run_block(b, THRES)) for b in spec["blocks"]]
        got = g.download_water()
        bad = 0
        for i in range(n):
            v = C.c_int64()
            hip.check(hip.dll.wdpm_get_option(g.rank_ctx(i), capi.OPT_GUARD_BAD, C.byref(v)))
            bad += v.value
        assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
    nd = n_bit_diff(got, want)
    assert nd == 0, f"{nd} cells of the water raster differ from the oracle"
    assert got_md == want_md, f"max diff per block {got_md} vs {want_md}"
    return [dict(blocks=spec["blocks"], differ=nd)]


def main(names):
    from test_marching_slabs import CASES, GROUP_CASES
    hip = wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        before, t0, figures = hip.launch_ledger(), time.time(), []
        try:
            if name in GROUP_CASES:
                figures = run_group(hip, oracle, GROUP_CASES[name])
            else:
                figures = play_slab(hip, oracle, CASES[name], on_device=True)
                check_exact(figures)
            ok, err = True, ""
        except Exception as e:                            # noqa: BLE001 - reported per case, the parent fails on it
            ok, err = False, f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=3)
        d, ds = cw.delta(before, hip.launch_ledger())
        out[name] = dict(ok=ok, error=err, delta=d, switches=ds, seconds=round(time.time() - t0, 2), figures=figures)
        print(name, "ok" if ok else err, f"{out[name]['seconds']} s", figures, file=sys.stderr, flush=True)
        if not ok and ("guard bytes" in err or "hand-over" in err):
            break                                         # nothing more on this device
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
