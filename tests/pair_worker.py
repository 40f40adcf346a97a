"""Child process of tests/test_pair_iterations.py: plays the named cases (CASES there) on the HIP library and on the CPU oracle
with tests/coverage_worker.py's machinery - every observation and the final raster bit for bit - and records what each case added
to the launch ledger.  The WDPM_* switches come with the environment (they are read once per process).  Prints one JSON line.

    python tests/pair_worker.py <case> [<case> ...]"""
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


_make_case = cw.make_case
_spec = {}


def make_case(R, C, seed, dem_kind="gentle", water="clean"):
    """coverage_worker's raster - and, where the case asks: NODATA blocks and dry regions that span strips, groups and chunks;
    depths of several metres in places (the unclamped neighbour step)"""
    dem, w = _make_case(R, C, seed, dem_kind, water)
    if _spec.get("patches"):
        dem[R // 5:R // 5 + 40, C // 3:C // 3 + 230] = cw.MISS
        dem[R // 2:R // 2 + 7, 5:C - 5:3] = cw.MISS
        w[:, 2 * C // 3 - 100:2 * C // 3 + 120] = 0.0
        w[R // 2 + 20:R // 2 + 60, :] = 0.0
        w[dem <= cw.MISS] = 0.0
    if _spec.get("deep"):
        rng = np.random.default_rng(seed + 1)
        sel = (rng.random((R, C)) < 0.01) & (dem > cw.MISS)
        w[sel] = 3.0 + 4.0 * rng.random((R, C))[sel]
    return dem, w


cw.make_case = make_case


def main(names):
    from test_pair_iterations import CASES
    hip = wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        before = hip.launch_ledger()
        try:
            _spec.clear()
            _spec.update(CASES[name])
            cw.run_case(hip, oracle, CASES[name])
            ok, err = True, ""
        except Exception as e:                            # noqa: BLE001 - reported per case, the parent fails on it
            ok, err = False, f"{type(e).__name__}: {e}\n" + traceback.format_exc(limit=3)
        d, ds = cw.delta(before, hip.launch_ledger())
        out[name] = dict(ok=ok, error=err, delta=d, switches=ds)
        print(name, "ok" if ok else err, file=sys.stderr, flush=True)
        if not ok and ("guard bytes" in err or "hand-over" in err):
            break                                         # nothing more on this device
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
