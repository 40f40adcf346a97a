"""Differential test of the WDPMCL command line against the UNMODIFIED reference executable on random small jobs with
oddly formatted input files (tests/cli_fuzz.py): same exit code, same report (minus wall clock), same bytes in the output
and scratch rasters.  CPU: the product's host code on the oracle back-end; GPU box: the shipped binary on the HIP path.
The reference's side of every job these tests run is stored in tests/golden/cli_fuzz_ref.json.gz (tests/golden/make_golden.py
clifuzz); other seeds (WDPM_FUZZ_SEEDS) run the reference executable itself, which oracle/Makefile `ref` builds where the
reference sources are."""
import gzip
import json
import os

import pytest

from cli_fuzz import first_difference, one
from conftest import GOLDEN, ROOT

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "WDPMCL_ref")
ORACLE_CLI = os.path.join(ROOT, "oracle", "_build", "WDPMCL_oracle")
HIP_CLI = os.path.join(ROOT, "wdpm_amd", "bin", "WDPMCL")


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(os.path.join(GOLDEN, "cli_fuzz_ref.json.gz"), "rt") as f:
        return json.load(f)


def differential(exe, seeds, tmp_path, recorded, vary_env=False):
    for seed in seeds:
        rec = recorded.get(str(seed))
        assert rec is not None or os.path.exists(REF_CLI), \
            f"seed {seed}: not in tests/golden/cli_fuzz_ref.json.gz, and there is no reference executable to run ({REF_CLI})"
        ok, ref, new, style, info = one(seed, str(tmp_path), REF_CLI, exe, vary_env, recorded=rec)
        if isinstance(ref[0], int) and ref[0] < 0:
            continue      # the reference itself died of a signal on this job (seen once in 10 000: a 4 x 1 drain job): nothing to equal
        assert ok, (f"seed {seed} {info} {style}: exit codes {ref[0]} / {new[0]}, files {ref[2]} / {new[2]}, "
                    f"{first_difference(ref[1], new[1])}, args {ref[3]}")
        assert ref[0] == 0 and ref[2]["out.asc"] is not None          # the jobs are valid ones: the reference ran them


def test_cli_equals_the_reference_executable_on_random_jobs(oracle, tmp_path, recorded):
    differential(ORACLE_CLI, range(0, 120), tmp_path, recorded)


def test_cli_knobs_never_show_in_the_results(oracle, tmp_path, recorded):
    """the same jobs with the raster spread over 2-5 row blocks, other exchange intervals, threaded ArcASCII I/O and the
    binary checkpoint sidecar switched on at random: still the reference's bytes"""
    differential(ORACLE_CLI, range(300, 420), tmp_path, recorded, vary_env=True)


@pytest.mark.gpu
def test_hip_cli_equals_the_reference_executable_on_random_jobs(tmp_path, recorded):
    lo, hi = (int(v) for v in os.environ.get("WDPM_FUZZ_SEEDS", "1000:1060").split(":"))
    differential(HIP_CLI, range(lo, hi), tmp_path, recorded)
    differential(HIP_CLI, range(lo + 300, hi + 300), tmp_path, recorded, vary_env=True)
