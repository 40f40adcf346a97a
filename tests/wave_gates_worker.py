"""Child process of tests/test_wave_gates.py: plays every case of one variant (VARIANTS there) on the HIP library, one context per
group (DEM level, chunk height) of the variant, and compares each raster - with the block's max diff, with totaldrain - bit for bit with
the oracle's through the digests in the file the parent wrote.  A case that differs is played once more on the CPU oracle, here, to say
how many cells differ and where.  Records per group what the upload found and, per class of cases, what they added to the launch
ledger.  Guard bands are on; stops at the first guard-byte error or error of the library.  The WDPM_* switches come with the
environment (they are read once per process).  Prints one JSON line.

    python tests/wave_gates_worker.py <reference.npy> <variant>"""
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
import wdpm_amd  # noqa: E402
from wdpm_amd import capi  # noqa: E402
import wave_gates_model as wg  # noqa: E402

MAX_REPORTED = 20
_oracle = []


def oracle():
    if not _oracle:
        _oracle.append(wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so")))
    return _oracle[0]


def set_level(ctx, level):
    """the DEM form the group's launches stream; None: the library's own choice under the environment's switches"""
    if level is not None:
        ctx.set_option(wdpm_amd.OPT_DEM32, 0 if level == "fp64" else 2)
        ctx.set_option(capi.OPT_DEM16, 1 if level == "codes16" else 0)
        assert ctx.get_option(wdpm_amd.OPT_DEM32) == int(level != "fp64"), "the DEM did not pass the 32-bit code check"
        assert (ctx.get_option(capi.OPT_DEM16) == 1) == (level == "codes16"), "the 16-bit codes are not in use"
    ctx.set_option(capi.OPT_TILES, 0)
    return ctx.get_option(capi.OPT_DEM16)


def where_it_differs(kw, bd, bw, play, steps, got):
    """the case once more on the oracle: which step, how many cells, the first of them"""
    with oracle().context(**kw) as o:
        o.upload(bd, bw)
        want = play(o)
    for name, (a, sa), (b, sb) in zip(steps, got, want):
        differ = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        if len(differ) or np.array(sa).tobytes() != np.array(sb).tobytes():
            r, c = differ[0] if len(differ) else (0, 0)
            return f"{name}: {len(differ)} cells differ, first at {(int(r), int(c))}: {a[r, c]!r} vs the oracle's {b[r, c]!r}; scalars {sa} vs {sb}"
    return "the digests differ but the oracle, run again, agrees"


def run(ref, name):
    from test_wave_gates import VARIANTS, clamp_cases, clamp_classes, nodata_cases, nodata_rasters, outlet_of
    v = VARIANTS[name]
    hip = wdpm_amd.load_hip()
    out = dict(variant=name, groups=[], failures=[], cases=0, fatal="")
    drain = v["module"] == "drain"

    def check(label, i, steps, got, again):
        out["cases"] += 1
        if all((wg.digest(w, *s) == ref[i, k]).all() for k, (w, s) in enumerate(got)):
            return
        if len(out["failures"]) < MAX_REPORTED:
            out["failures"].append(f"{label}: {again(got)}")
        elif len(out["failures"]) == MAX_REPORTED:
            out["failures"].append("... and more")

    try:
        if v["kind"] == "nodata":
            rasters, cases = nodata_rasters(), nodata_cases()
            for level, chunk, _ in v["groups"]:
                g = dict(label=f"{level}-chunk{chunk}", level=level, chunk=chunk, dem16=None, classes={})
                out["groups"].append(g)
                for raster, (R, C, bd, bw) in rasters.items():
                    kw = dict(module=v["module"], nrows=R, ncols=C, missingvalue=wg.MISS)
                    before, n = hip.launch_ledger(), 0
                    with hip.context(kernel=wdpm_amd.KERNEL_FUSED, chunk_rows=chunk, **kw) as ctx:
                        for i, (rname, pos) in enumerate(cases):
                            if rname != raster:
                                continue
                            d, w = wg.with_nodata(bd, bw, pos)
                            ctx.upload(d, w)
                            g["dem16"] = set_level(ctx, level)
                            got = wg.play_nodata(ctx, w)
                            n += 1
                            check(f"{g['label']}/{raster}{pos}", i, wg.NODATA_STEPS, got,
                                  lambda got: where_it_differs(kw, d, w, lambda o: wg.play_nodata(o, w), wg.NODATA_STEPS, got))
                        bad = cw.guard_bad(hip, ctx)
                        assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
                    g["classes"][raster] = dict(cases=n, switches=cw.delta(before, hip.launch_ledger())[1])
        else:
            bd, bw = wg.clamp_raster(wg.R_MAIN, wg.C_MAIN)
            cases = clamp_cases()
            kw = dict(module=v["module"], nrows=wg.R_MAIN, ncols=wg.C_MAIN, missingvalue=wg.MISS)
            if drain:
                kw.update(zip(("drainrow", "draincol"), outlet_of(bd)))
            for level, chunk, replays in v["groups"]:
                g = dict(label=f"{level}-chunk{chunk}", level=level, chunk=chunk, dem16=None, classes={})
                out["groups"].append(g)
                with hip.context(kernel=wdpm_amd.KERNEL_FUSED, chunk_rows=chunk, **kw) as ctx:
                    ctx.upload(bd, bw)
                    g["dem16"] = set_level(ctx, level)
                    for cls, depth in clamp_classes(replays).items():
                        before, n = hip.launch_ledger(), 0
                        for i, (c, pos) in enumerate(cases):
                            if c != cls:
                                continue
                            w = wg.with_depth(bw, pos, depth)
                            got = wg.play_clamp(ctx, w, drain)
                            n += 1
                            check(f"{g['label']}/{cls}{pos}", i, wg.CLAMP_STEPS, got,
                                  lambda got: where_it_differs(kw, bd, w, lambda o: wg.play_clamp(o, w, drain), wg.CLAMP_STEPS, got))
                        g["classes"][cls] = dict(cases=n, switches=cw.delta(before, hip.launch_ledger())[1])
                    bad = cw.guard_bad(hip, ctx)
                    assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
    except Exception as e:                                # noqa: BLE001 - an error of the library or stray writes: nothing more on this device
        out["fatal"] = f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=4)
    return out


def main(ref_path, name):
    t0 = time.time()
    out = run(np.load(ref_path), name)
    out["seconds"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
