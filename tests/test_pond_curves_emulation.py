"""The curve kernels' own source (wdpm_amd/csrc/wdpm_pond_curves.hip) on the CPU: tests/curves_emu_main.cpp runs them as 256 host
threads per block under the address and undefined-behaviour sanitizers - a stand-alone program, nothing is loaded into Python - on
a basin raster from a flood fill and a walk down every descent, with buffers of exact size, and holds the whole table and the counts
against a plain double loop over all cells and stages."""
import pytest

import emu_build
from test_pond_outlets_emulation import CASES, RAMPS        # the same shapes and rows per wave: 1, 2, 3, 40 and the library's choice


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "curves_emu")


def run(emu, case):
    out = emu_build.run(emu, *case)
    assert "table mismatches 0 counts agree" in out, out
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:2])) + "rpw%d" % c[4])
def test_kernels_on_the_host_under_sanitizers(emu, case):
    out = run(emu, case)
    assert " N 0 " not in out, out
    if case[:2] != (1, 1) and case[2] < 1.0 and case[1] > 1:
        assert " stage cells 0 " not in out and " most steps 0 " not in out and " most steps 1 " not in out, out


@pytest.mark.parametrize("case", RAMPS, ids=lambda c: "rpw%d" % c[4])
def test_one_basin_has_no_curve(emu, case):
    out = run(emu, case)
    assert " N 1 without curve 1 flat 0 stage cells 0 " in out, out
