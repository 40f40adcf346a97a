"""The outlet kernels' own source (wdpm_amd/csrc/wdpm_pond_outlets.hip) on the CPU: tests/outlets_emu_main.cpp runs them as 256 host
threads per block under the address and undefined-behaviour sanitizers - a stand-alone program, nothing is loaded into Python - on
a basin raster from a flood fill and a walk down every descent, with buffers of exact size, and holds the whole table and the counts
against a plain double loop over all pairs of neighbouring cells."""
import pytest

import emu_build

# file rows, columns, density, seed, rows per wave (0: as the library chooses); the shapes of tests/test_pond_catchments_emulation.py
CASES = [(20, 70, 0.40, 1, 0),        # two segments, the second nearly empty; threshold 0.001 with films of 0.0005 m on the slopes
         (12, 200, 0.41, 2, 1),       # four segments = one block per row, threshold 0; every row a strip of its own
         (16, 130, 0.60, 3, 2),       # carried down two rows; the third segment holds the right border alone
         (17, 126, 0.30, 4, 3),       # the right border is lane 63 of the last segment; the last strip is short
         (3, 700, 0.50, 5, 3),        # wide and flat: one strip holds both border rows
         (40, 1, 0.70, 6, 2),         # one column
         (45, 130, 0.35, 7, 40),      # carried down forty rows, then a short strip
         (20, 190, 1.00, 8, 40),      # all wet but the NODATA cells: rows that read neither dem nor w
         (1, 1, 1.00, 2, 0)]          # one cell
# seed 0: a ramp into one pond, one basin over everything - every row is skipped and the one pond has no outlet
RAMPS = [(33, 200, 0, 0, rpw) for rpw in (1, 2, 3, 40)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "outlets_emu")


def run(emu, case):
    out = emu_build.run(emu, *case)
    assert "table mismatches 0 counts agree" in out, out
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:2])) + "rpw%d" % c[4])
def test_kernels_on_the_host_under_sanitizers(emu, case):
    out = run(emu, case)
    assert " N 0 " not in out, out
    if case[:2] != (1, 1) and case[2] < 1.0 and case[1] > 1:
        assert " divide 0 " not in out and " filled 0 " not in out, out


@pytest.mark.parametrize("case", RAMPS, ids=lambda c: "rpw%d" % c[4])
def test_one_basin_has_no_outlet(emu, case):
    out = run(emu, case)
    assert " N 1 without outlet 1 to land 0 divide 0 filled 0 " in out, out
