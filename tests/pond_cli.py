"""TEST INFRASTRUCTURE: what the GPU tests of the command line's pond files share - the product executable, one way to run it
with an environment that inherits nothing the files depend on, and the reader of the rasters they compare."""
import os
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
from make_golden import strip_timing  # noqa: E402

HIP_CLI = os.path.join(ROOT, "wdpm_amd", "bin", "WDPMCL")
ADD_MM, ITER = 300, 1000        # one block of the command line's 1000 iterations


def job_args(dem):
    """add ADD_MM of water to `dem`, no water file, no scratch file, ITER iterations"""
    return ["add", dem, "NULL", "out.asc", "NULL", str(ADD_MM), "1.0", "1.0", "0", "0", "0.005", str(ITER)]


def clean_env():
    """the caller's environment without anything that chooses pond files, devices or guard bands"""
    return {k: v for k, v in os.environ.items()
            if not k.startswith("WDPM_POND") and k not in ("WDPM_GPUS", "WDPM_DEVICES", "WDPM_GUARD_KB")}


def read_asc(path):
    """the raster and its cell size"""
    with open(path) as f:
        hdr = [f.readline().split() for _ in range(6)]
        vals = np.array(f.read().split(), dtype=np.float64)
    return vals.reshape(int(float(hdr[1][1])), int(float(hdr[0][1]))), float(hdr[4][1])


def run_cli(cwd, args, status=0, **env):
    """the product's command line on `args` in `cwd` with `env` set: the report without its wall-clock parts, the bytes of out.asc, stderr"""
    p = subprocess.run([HIP_CLI] + list(args), cwd=cwd, capture_output=True, text=True, timeout=600, env=dict(clean_env(), **env))
    assert p.returncode == status, p.stderr[-3000:]
    with open(os.path.join(cwd, "out.asc"), "rb") as f:
        return strip_timing(p.stdout), f.read(), p.stderr
