"""Child process of tests/test_kernel_coverage.py: plays the named cases of one environment profile (the WDPM_* switches are read
once per process) on the HIP library and on the CPU oracle, compares every observation bit for bit and records what each case
added to the launch ledger (include/wdpm.h: wdpm_launch_ledger).  Prints one JSON line: {case: {"ok", "error", "delta", "switches"}}.

Runs without conftest.py, so it sets the guard bands itself and checks them before closing each context, as the `hip` fixture does.

    python tests/coverage_worker.py <case> [<case> ...]"""
import ctypes as C
import json
import os
import sys
import traceback

os.environ.setdefault("WDPM_GUARD_KB", "64")    # before the library is loaded: guard bands around the device buffers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import wdpm_amd  # noqa: E402
from wdpm_amd import capi  # noqa: E402
from helpers import find_drain, n_bit_diff, pad, sha  # noqa: E402

MISS = -99999.0
THRES = 1e-5


def make_case(R, C, seed, dem_kind="gentle", water="clean"):
    """a gentle encodable DEM (16-bit offsets pass) with NODATA on the first and last rows and columns and scattered inside;
    water of the given kind: clean, on NODATA cells too, with -0.0 depths, or with negative depths"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:R, 0:C]
    dem = np.round(500.0 + 0.3 * np.sin(x / 5.1) * np.cos(y / 3.3) + rng.normal(0, 0.05, (R, C)) - 0.002 * (x + y), 4)
    dem[rng.random((R, C)) < 0.03] = MISS
    if R > 2 and C > 2:
        dem[0, :] = dem[-1, :] = MISS
        dem[:, 0] = dem[:, -1] = MISS
    if dem_kind == "huge":                               # one elevation beyond 2^30 m: the exact (unclamped) neighbour step
        dem[R // 2, C // 2] = 1.5e9
    valid = dem > MISS
    depth = np.where(rng.random((R, C)) < 0.25, 0.0, 0.3 * rng.random((R, C)))
    if water == "nodata":                                # water the reference keeps on NODATA cells
        w = depth
    else:
        w = np.where(valid, depth, 0.0)
    if water == "negzero":
        w = np.where(valid & (rng.random((R, C)) < 0.2), -0.0, w)
    elif water == "negative":
        w = np.where(valid & (rng.random((R, C)) < 0.05), -0.01 * rng.random((R, C)), w)
    return dem, w


def negative_water(bw, seed):
    """the same raster with a few negative depths: the gated launches (no flush, no max change, water not plain)"""
    rng = np.random.default_rng(seed)
    w = bw.copy()
    sel = (rng.random(w.shape) < 0.05) & (w > 0)
    w[sel] = -w[sel] * 0.01
    return w


def delta(before, after):
    (c0, s0), (c1, s1) = before, after
    d = {k: v - c0.get(k, 0) for k, v in c1.items() if v != c0.get(k, 0)}
    ds = {}
    for k in d:
        states = {b: n - s0.get(k, {}).get(b, 0) for b, n in s1.get(k, {}).items() if n != s0.get(k, {}).get(b, 0)}
        ds[k] = {str(b): n for b, n in states.items()}
    return d, ds


def guard_bad(lib, ctx):
    v = C.c_int64()
    lib.check(lib.dll.wdpm_get_option(ctx._h, capi.OPT_GUARD_BAD, C.byref(v)))
    return v.value


def play(ctx, script, bw, seed):
    """the call script; returns the list of observations (compared bit for bit between the two libraries)"""
    obs = []
    for op in script:
        kind = op[0]
        if kind == "block":                              # begin_block + expect_max_diff + iterate + max_diff
            obs.append(("block", ctx.run_block(op[1], THRES)))
        elif kind == "iter":                             # plain iterate: no flush, no max change
            ctx.iterate(op[1])
        elif kind == "negative":                         # new water with negative depths
            ctx.upload_water(negative_water(bw, seed))
        elif kind == "overlap":                          # a block whose last iteration is split into three windows
            ctx.begin_block(THRES)
            ctx.expect_max_diff()
            ctx.iterate_overlapped(op[1], op[2], op[3])
            obs.append(("overlap", ctx.max_diff()))
        elif kind == "max_diff":
            obs.append(("max_diff", ctx.max_diff()))
        else:
            raise ValueError(kind)
    return obs


def unpadded(lib, ctx, dem, water):
    """the set-up and statistics entry points: upload_unpadded (add's set-up), count_stats, find_drain, download_unpadded"""
    R, Cc = dem.shape
    d = np.ascontiguousarray(dem, dtype=np.float64)
    w = np.ascontiguousarray(water, dtype=np.float64)
    su = capi.SetupStruct(op=1, add=0.05, rof=0.5, sub=0.0)
    lib.check(lib.dll.wdpm_upload_unpadded(ctx._h, d.ctypes.data, w.ctypes.data, C.byref(su)))
    nv, nw, mx = C.c_int64(), C.c_int64(), C.c_double()
    lib.check(lib.dll.wdpm_count_stats(ctx._h, 0, R + 2, C.byref(nv), C.byref(nw), C.byref(mx)))
    md, dr, dc = C.c_double(), C.c_int32(), C.c_int32()
    lib.check(lib.dll.wdpm_find_drain(ctx._h, 0, R + 2, C.byref(md), C.byref(dr), C.byref(dc)))
    out = np.empty((R, Cc), dtype=np.float64)
    lib.check(lib.dll.wdpm_download_unpadded(ctx._h, 0, R, 1, out.ctypes.data))
    return [("stats", nv.value, nw.value, mx.value), ("drain", md.value, dr.value, dc.value)], out


def run_case(hip, oracle, spec):
    R, Cc = spec["shape"]
    dem, water = make_case(R, Cc, spec.get("seed", R * 7 + Cc), spec.get("dem", "gentle"), spec.get("water", "clean"))
    bd, bw = pad(dem, water, MISS)
    module = spec["module"]
    kw = dict(module=module, nrows=R, ncols=Cc, missingvalue=MISS)
    td0 = 0.0
    if module == "drain":
        dr, dc = find_drain(bd)
        td0 = max(bw[dr, dc], 0.0)
        kw.update(drainrow=dr, draincol=dc)
    results = {}
    for name, lib in (("hip", hip), ("oracle", oracle)):
        extra = dict(kernel=spec.get("kernel", wdpm_amd.KERNEL_FUSED), chunk_rows=spec.get("chunk", 0)) if lib is hip else {}
        with lib.context(**kw, **extra) as ctx:
            obs = []
            if spec.get("unpadded"):
                o, _ = unpadded(lib, ctx, dem, water)
                obs += o
            ctx.upload(bd, bw)
            ctx.totaldrain = td0
            if lib is hip:
                level = spec.get("level", "codes32")
                ctx.set_option(wdpm_amd.OPT_DEM32, 0 if level == "fp64" else 2 if spec.get("force", True) else 1)
                ctx.set_option(capi.OPT_DEM16, 1 if level == "codes16" else 0)
                if level != "fp64" and spec.get("dem", "gentle") == "gentle":
                    assert ctx.get_option(wdpm_amd.OPT_DEM32) == 1, "the DEM did not pass the 32-bit code check"
                    assert ctx.get_option(capi.OPT_DEM16) == int(level == "codes16"), "the 16-bit offsets are not in use"
                if "tiles" in spec:
                    ctx.set_option(capi.OPT_TILES, spec["tiles"])
            obs += play(ctx, spec["script"], bw, spec.get("seed", 1))
            w = ctx.download_water()
            td = ctx.totaldrain
            stats = ctx.drain_stats() if module == "drain" else None
            if spec.get("unpadded"):
                o, out = unpadded(lib, ctx, dem, w[1:-1, 1:-1])
                obs += o
                obs.append(("unpadded", sha(out)))
            bad = guard_bad(lib, ctx) if lib is hip else 0
            assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
        results[name] = (obs, w, td, stats)
    (og, wg, tg, sg), (oo, wo, to, so) = results["hip"], results["oracle"]
    nd = n_bit_diff(wg, wo)
    assert nd == 0, f"{nd} cells of the water raster differ from the oracle"
    assert json.dumps(og) == json.dumps(oo), f"observations differ: {og} vs {oo}"
    assert np.float64(tg).view(np.uint64) == np.float64(to).view(np.uint64), f"totaldrain {tg!r} vs {to!r}"
    if sg is not None:
        assert np.array(sg, dtype=np.float64).view(np.uint64).tolist() == np.array(so, dtype=np.float64).view(np.uint64).tolist(), \
            f"drain_stats {sg!r} vs {so!r}"


def main(names):
    from test_kernel_coverage import CASES, GUARD_CASE
    hip = wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        spec = GUARD_CASE if name == "guard" else CASES[name]
        before = hip.launch_ledger()
        try:
            run_case(hip, oracle, spec)
            ok, err = True, ""
        except Exception as e:                            # noqa: BLE001 - reported per case, the parent fails on it
            ok, err = False, f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=3)
        d, ds = delta(before, hip.launch_ledger())
        out[name] = dict(ok=ok, error=err, delta=d, switches=ds)
        if not ok and "guard bytes" in err:
            break                                         # nothing more on this device
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
