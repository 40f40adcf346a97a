"""The catchment kernels' own source (wdpm_amd/csrc/wdpm_pond_catchments.hip) on the CPU: tests/catch_emu_main.cpp runs them as 256
host threads per block under the address and undefined-behaviour sanitizers - a stand-alone program, nothing is loaded into
Python - on labels and masks from a flood fill and buffers of exact size, with the links of the jump rounds raced as relaxed host
atomics, and holds basin raster, table and counts against a plain loop that walks every cell's descent one step at a time."""
import pytest

import emu_build

# file rows, columns, density, seed, rows per wave (0: as the library chooses, 1000: all rows in one strip); the shapes of
# tests/test_pond_rims_emulation.py
CASES = [(20, 70, 0.40, 1, 0),        # two segments, the second nearly empty; threshold 0.001 with films of 0.0005 m on the slopes
         (12, 200, 0.41, 2, 1),       # four segments = one block per row, threshold 0
         (16, 130, 0.60, 3, 2),       # carried down two rows; the third segment holds the right border alone
         (17, 126, 0.30, 4, 7),       # the right border is lane 63 of the last segment; the last strip is short
         (3, 700, 0.50, 5, 7),        # wide and flat: every strip holds both border rows
         (40, 1, 0.70, 6, 2),         # one column
         (20, 190, 1.00, 8, 1000),    # all wet but the NODATA cells: rows that read neither dem nor w
         (1, 1, 1.00, 2, 0)]          # one cell
# seed 0: a channel that snakes through every other row of 33 x 200 into one pond cell, with every forced rows-per-wave value
SERPENTINE = [(33, 200, 0, 0, rpw) for rpw in (1, 2, 7, 64, 1000)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "catch_emu")


def run(emu, case):
    out = emu_build.run(emu, *case)
    assert "basin mismatches 0 table mismatches 0 counts agree identity holds" in out, out
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:2])))
def test_kernels_on_the_host_under_sanitizers(emu, case):
    out = run(emu, case)
    assert " N 0 " not in out, out
    if case[:2] != (1, 1) and case[2] < 1.0:
        assert " caught 0 " not in out and " pits 0 " not in out, out


@pytest.mark.parametrize("case", SERPENTINE, ids=lambda c: "rpw%d" % c[4])
def test_serpentine_channel(emu, case):
    out = run(emu, case)
    hops = int(out.split("longest descent ")[1].split()[0])
    rounds = int(out.split(" rounds ")[1].split()[0])
    assert hops > 3000 and " N 1 " in out and " unponded 0 " in out, out
    assert 4 <= rounds <= 40 and rounds % 4 == 0, out        # whole batches, under the cap
