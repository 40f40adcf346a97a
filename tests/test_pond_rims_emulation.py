"""The rim kernels' own source (wdpm_amd/csrc/wdpm_pond_rims.hip) on the CPU: tests/rims_emu_main.cpp runs them as 256 host threads
per block under the address and undefined-behaviour sanitizers, on labels and masks from a flood fill and buffers of exact size, and
holds the rim table against a plain loop over every cell's eight neighbours.  The halo reads - the rows above and below a wave's
strip, the cells beside a segment, column 0 and ncp - 1, row 0 and rows - 1 - are checked here, where a stray index harms nobody."""
import pytest

import emu_build

# file rows, columns, density, seed, rows per wave (0: as the library chooses, 1000: all rows in one strip)
CASES = [(20, 70, 0.40, 1, 0),        # two segments, the second nearly empty; threshold 0.001 with 0.0005 m on rim cells
         (12, 200, 0.41, 2, 1),       # four segments = one block per row, threshold 0
         (16, 130, 0.60, 3, 2),       # carried down two rows; the third segment holds the right border alone
         (17, 126, 0.30, 4, 7),       # the right border is lane 63 of the last segment; the last strip is short
         (3, 700, 0.50, 5, 7),        # wide and flat: every strip holds both border rows
         (40, 1, 0.70, 6, 2),         # one column
         (20, 190, 1.00, 8, 1000),    # all wet but the NODATA cells: one carry down every strip
         (1, 1, 1.00, 2, 0)]          # one cell: no rim, eight walls


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "rims_emu")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:2])))
def test_kernels_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, *case)
    assert "rim mismatches 0" in out, out
    assert " N 0 " not in out, out
