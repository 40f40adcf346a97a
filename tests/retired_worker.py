"""Child process of tests/test_iter2_retired_strips.py: plays the named cases (CASES there) on the HIP library and on the CPU oracle
with tests/pair_worker.py's rasters and tests/coverage_worker.py's machinery - every observation and the final raster bit for bit -
and records what each case added to the launch ledger.  The WDPM_* switches come with the environment (they are read once per
process).  Prints one JSON line.

    python tests/retired_worker.py <case> [<case> ...]"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pair_worker as pw  # noqa: E402  (coverage_worker with the NODATA patches and dry regions a case may ask for)
import wdpm_amd  # noqa: E402

cw = pw.cw


def main(names):
    from test_iter2_retired_strips import CASES
    hip = wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        before = hip.launch_ledger()
        try:
            pw._spec.clear()
            pw._spec.update(CASES[name])
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
