#!/usr/bin/env python3
"""What a DEM on a binary grid gains from streaming as codes: blocks of 1000 add iterations on the synthetic DEM through the C ABI,
three set-ups interleaved on one box in one run, every measurement a process of its own under its own `timeout`:

    a  the synthetic DEM as generated (four decimals: the decimal reference)
    b  the same rounded to Float32 (codes on the grid 2^-s)
    c  b with WDPM_DEM_BINARY=0 (no binary attempt: the fp64 DEM, what the library did before)

    binary_dem_ab.py [rounds] [blocks per run] [sizes, comma separated]        default 2 3 16384,4096

Per run: ms per iteration of each block (host clock around wdpm_run_block, which ends in a device synchronise; the first block is
warm-up and is not counted), the level the DEM streamed at (options and launch ledger) and whether launches ran two iterations.
Then per size the medians, each set-up's own spread, and b against c and against a.  A run that ends abnormally ends the session."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MISS = -99999.0
SETUPS = {"a": ("decimal DEM", {}), "b": ("Float32 DEM", {}), "c": ("Float32 DEM, WDPM_DEM_BINARY=0", {"WDPM_DEM_BINARY": "0"})}


def child(n, setup, blocks):
    import numpy as np

    import wdpm_amd
    from wdpm_amd import capi
    lib = wdpm_amd.load_hip()
    dem = lib.synth_dem(n, n)
    if setup != "a":
        dem = dem.astype(np.float32).astype(np.float64)
    bd = np.full((n + 2, n + 2), MISS)
    bd[1:-1, 1:-1] = dem
    del dem
    bw = np.where(bd > MISS, 0.1, 0.0)
    with lib.context(module="add", nrows=n, ncols=n, missingvalue=MISS) as c:
        c.upload(bd, bw)
        del bd, bw
        ms = []
        for _ in range(blocks + 1):
            c.synchronize()
            t = time.perf_counter()
            c.run_block(1000, 0.005 / 1000)
            ms.append((time.perf_counter() - t))          # seconds per 1000 iterations = ms per iteration
        opts = {k: c.get_option(v) for k, v in (("dem32", capi.OPT_DEM32), ("dem16", capi.OPT_DEM16), ("grid", capi.OPT_DEM_GRID),
                                                ("exp", capi.OPT_DEM_GRID_EXP))}
    counts, switches = lib.launch_ledger()
    levels, two, one = {}, 0, 0
    for name, k in counts.items():
        if k and name.startswith("fused_iteration_kernel<"):
            lv = name.split(",")[2].strip()
            levels[lv] = levels.get(lv, 0) + k
            for bits, cnt in switches[name].items():
                if bits & capi.LEDGER_ITER2:
                    two += cnt
                else:
                    one += cnt
    print(json.dumps(dict(n=n, setup=setup, ms=ms[1:], warmup=ms[0], levels=levels, two=two, one=one, build=lib.dll.wdpm_build_info().decode(),
                          **opts)))


def describe(r):
    lv = max(r["levels"], key=r["levels"].get) if r["levels"] else "?"
    level = {"0": "fp64 DEM", "1": "32-bit codes", "2": "16-bit codes"}.get(lv, lv)
    grid = f" on {r['grid']}^-{r['exp']} m" if r["grid"] else ""
    offsets = "" if lv != "1" else {0: ", 16-bit offsets refused", 2: ", 16-bit offsets available but not in use"}.get(r["dem16"], "")
    return f"{level}{grid}{offsets}; {r['two']} launches of two iterations, {r['one']} of one"


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sizes = [int(s) for s in (sys.argv[3] if len(sys.argv) > 3 else "16384,4096").split(",")]
    res, said = {}, set()
    for r in range(rounds):
        for n in sizes:
            for setup, (what, env) in SETUPS.items():
                limit = 90 + blocks * 10 + (n // 4096) ** 2 * 12      # synthesis, upload and the blocks at a generous rate
                p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n), setup, str(blocks)],
                                   env=dict(os.environ, **env), capture_output=True, text=True)
                if p.returncode != 0:
                    print(f"{n} {setup}: exit status {p.returncode}; nothing more is started\n{p.stderr[-2000:]}", flush=True)
                    sys.exit(1)
                out = json.loads(p.stdout.strip().splitlines()[-1])
                if "build" not in said:
                    print(f"library: {out['build']}", flush=True)
                    said.add("build")
                res.setdefault((n, setup), []).extend(out["ms"])
                print(f"round {r + 1}  {n}^2  {setup} ({what}): " + " ".join(f"{m:.4f}" for m in out["ms"]) + f" ms per iteration  [{describe(out)}]", flush=True)
    print()
    for n in sizes:
        med = {s: statistics.median(res[(n, s)]) for s in SETUPS}
        for s in SETUPS:
            v = res[(n, s)]
            print(f"{n}^2  {s}: median {med[s]:.4f} ms per iteration over {len(v)} blocks, min {min(v):.4f}, max {max(v):.4f} (spread {(max(v) - min(v)) / med[s] * 100:.1f} %)")
        print(f"{n}^2  c / b = {med['c'] / med['b']:.3f} (the fp64 DEM against the codes of the binary grid)   b / a = {med['b'] / med['a']:.3f} (the binary grid against the decimal one)")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
    else:
        main()
