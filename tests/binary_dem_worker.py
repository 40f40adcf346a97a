"""Child process of tests/test_binary_dem.py: plays the named cases (CHILD_CASES there) on the HIP library and on the CPU oracle with
tests/coverage_worker.py's machinery - every observation and the final raster bit for bit - on DEMs that went through Float32, and
records what each case added to the launch ledger and which grid every upload found (WDPM_OPT_DEM_GRID, _EXP).  The WDPM_*
switches come with the environment (they are read once per process).  Prints one JSON line.

    python tests/binary_dem_worker.py <case> [<case> ...]"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pair_worker as pw  # noqa: E402  (coverage_worker's raster with the pair cases' patches; sets the guard bands before the library is loaded)
import wdpm_amd  # noqa: E402
from binary_dem_model import f32_keep_nodata  # noqa: E402
from helpers import random_case  # noqa: E402

cw = pw.cw
_pair_make_case = pw.make_case
_spec = {}


def make_case(R, C, seed, dem_kind="gentle", water="clean"):
    if _spec.get("source") == "random":
        dem, w, _ = random_case(seed, R, C)
    else:
        dem, w = _pair_make_case(R, C, seed, dem_kind, water)
    return f32_keep_nodata(dem), w


cw.make_case = make_case


class Spy:
    """the HIP library, with every context noting what its uploads found"""

    def __init__(self, lib):
        self._lib, self.grids = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def context(self, **kw):
        ctx = self._lib.context(**kw)
        upload = ctx.upload

        def noting_upload(bd, bw):
            upload(bd, bw)
            self.grids.append([ctx.get_option(wdpm_amd.OPT_DEM_GRID), ctx.get_option(wdpm_amd.OPT_DEM_GRID_EXP),
                               ctx.get_option(wdpm_amd.OPT_DEM32)])
        ctx.upload = noting_upload
        return ctx


def main(names):
    from test_binary_dem import CHILD_CASES
    hip = wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        spy = Spy(hip)
        before = hip.launch_ledger()
        try:
            for s in (_spec, pw._spec):
                s.clear()
                s.update(CHILD_CASES[name])
            cw.run_case(spy, oracle, CHILD_CASES[name])
            ok, err = True, ""
        except Exception as e:                            # noqa: BLE001 - reported per case, the parent fails on it
            ok, err = False, f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=3)
        d, ds = cw.delta(before, hip.launch_ledger())
        out[name] = dict(ok=ok, error=err, delta=d, switches=ds, grids=spy.grids)
        print(name, "ok" if ok else err, file=sys.stderr, flush=True)
        if not ok and ("guard bytes" in err or "hand-over" in err):
            break                                         # nothing more on this device
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
