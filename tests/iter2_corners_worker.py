"""Child process of tests/test_iter2_corners.py: plays the named cases (CASES there) on the HIP library and on the CPU oracle with
tests/coverage_worker.py's machinery - guard bands, every observation, the final raster and totaldrain bit for bit - on the rasters the
case names (the operand pools, the elevations around 1.2e9 m, the gentle raster without its NODATA frame, tests/pair_worker.py's otherwise), and records what each case added to
the launch ledger.  A block may carry its own threshold: ("block", n, thres).  The WDPM_* switches come with the environment (they
are read once per process).  Stops at the first guard-byte or hand-over error.  Prints one JSON line.

    python tests/iter2_corners_worker.py <case> [<case> ...]"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pair_worker as pw  # noqa: E402  (coverage_worker with the deep cells a case may ask for; sets the guard bands before the library is loaded)
import wdpm_amd  # noqa: E402

cw = pw.cw
_spec = {}
_final = []            # the rasters the libraries were left with, in run_case's order: HIP, oracle


def make_case(R, C, seed, dem_kind="gentle", water="clean"):
    from test_iter2_corners import far_dem_case, live_edge_case, operand_case
    if _spec.get("raster") == "live-edges":
        return live_edge_case(pw._make_case, R, C, seed)
    if _spec.get("raster") == "operands":
        return operand_case(R, C, seed, _spec["pool"], _spec.get("subnormal", False))
    if _spec.get("raster") == "far":
        return far_dem_case(R, C, seed, _spec["grid_exp"], _spec["deep_cells"])
    return pw.make_case(R, C, seed, dem_kind, water)


def play(ctx, script, bw, seed):
    """coverage_worker.play with a threshold of the block's own where it names one"""
    obs = []
    for op in script:
        if op[0] == "block" and len(op) == 3:
            obs.append(("block", ctx.run_block(op[1], op[2])))
        else:
            obs += _play(ctx, [op], bw, seed)
    _final.append(ctx.download_water())
    return obs


_play = cw.play
cw.make_case = make_case
cw.play = play


def main(names):
    from test_iter2_corners import CASES, KERNEL16, KERNEL32
    hip =wdpm_amd.load_hip()
    oracle = wdpm_amd.load(os.path.join(cw.ROOT, "oracle", "_build", "libwdpm_oracle.so"))
    out = {}
    for name in names:
        before = hip.launch_ledger()
        try:
            for s in (_spec, pw._spec):
                s.clear()
                s.update(CASES[name])
            del _final[:]
            cw.run_case(hip, oracle, CASES[name])
            if CASES[name].get("subnormal"):
                w = _final[0]
                assert ((w > 0) & (w < 2.2e-308)).any(), "no subnormal depth survived the block"
            # the water stayed "plain" (scan_water_kernel): the steady launches were the gate-free instantiation on the case's codes
            d, _ = cw.delta(before, hip.launch_ledger())
            kernel = KERNEL16 if CASES[name]["level"] == "codes16" else KERNEL32
            assert d.get(kernel, 0) > 0, f"no launch of {kernel}: {sorted(d)}"
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
