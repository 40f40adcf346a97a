"""Child process of tests/test_dem16_bases.py: plays the named cases on the HIP library's marching kernel with the 16-bit DEM codes
forced on launches of any size, and compares every raster and the block's max diff bit for bit with the oracle's results in the
file the parent wrote.  Records what the upload found (grid, whether the 16-bit codes are in use) and what each case added to the
launch ledger.  The WDPM_* switches come with the environment (they are read once per process).  Prints one JSON line.

    python tests/dem16_bases_worker.py <reference.npz> <case> [<case> ...]"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import coverage_worker as cw  # noqa: E402  (sets the guard bands before the library is loaded)
import wdpm_amd  # noqa: E402
from wdpm_amd import capi  # noqa: E402
from helpers import n_bit_diff  # noqa: E402


def run_case(hip, ref, name):
    from test_dem16_bases import build_case, play
    c = build_case(name)
    grid, exp, _ = c["want"]
    with hip.context(module="add", nrows=c["R"], ncols=c["C"], missingvalue=c["miss"], kernel=wdpm_amd.KERNEL_FUSED) as ctx:
        ctx.upload(c["bd"], c["bw"])
        ctx.set_option(wdpm_amd.OPT_DEM32, 2)
        ctx.set_option(capi.OPT_DEM16, 2)
        ctx.set_option(capi.OPT_TILES, 0)
        assert ctx.get_option(wdpm_amd.OPT_DEM32) == 1, "the DEM did not pass the 32-bit code check"
        found = (ctx.get_option(wdpm_amd.OPT_DEM_GRID), ctx.get_option(wdpm_amd.OPT_DEM_GRID_EXP))
        assert found[0] == grid and exp in (None, found[1]), f"the upload found the grid {found}, expected {(grid, exp)}"
        dem16 = ctx.get_option(capi.OPT_DEM16)
        got = play(ctx, c["bw"])
        bad = cw.guard_bad(hip, ctx)
        assert bad == 0, f"{bad} guard bytes around the device buffers were overwritten"
    for key, a in got.items():
        want = ref[f"{name}/{key}"]
        nd = n_bit_diff(a, want)
        assert nd == 0, f"{key}: {nd} values differ from the oracle" + (f" ({a[0]!r} vs {want[0]!r})" if key == "maxdiff" else "")
    return dem16


def main(ref_path, names):
    hip = wdpm_amd.load_hip()
    ref = np.load(ref_path)
    out = {}
    for name in names:
        before = hip.launch_ledger()
        dem16 = None
        try:
            dem16 = run_case(hip, ref, name)
            ok, err = True, ""
        except Exception as e:                            # noqa: BLE001 - reported per case, the parent fails on it
            ok, err = False, f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=3)
        d, ds = cw.delta(before, hip.launch_ledger())
        out[name] = dict(ok=ok, error=err, dem16=dem16, switches=ds)
        print(name, "ok" if ok else err, file=sys.stderr, flush=True)
        if not ok and ("guard bytes" in err or not err.startswith("AssertionError")):
            break                                         # stray writes or an error of the library: nothing more on this device
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
