"""The pond outlets over row blocks on the CPU (include/wdpm_group_pond_outlets.h): tests/group_outlets_emu_main.cpp cuts a raster into
strips of rows, gives each strip the basins and the level keys of its neighbours' rows (and rubbish for their DEM and water), runs the
outlet kernels' own source (wdpm_amd/csrc/wdpm_pond_outlets.hip) per strip as host threads on buffers of exact size, makes the pour
levels final and merges the strips' tables with wdpm_amd/csrc/wdpm_outlets_merge.h, and holds table and counts against a plain double
loop over all pairs of the whole raster - all under the address and undefined-behaviour sanitizers, in a program of its own.  Both
merges are also called alone on hand-written slot tables."""
import re

import pytest

import emu_build

# file rows, columns, density, seed, owned rows per strip, rows per wave (0: as the library chooses)
NOISE = [(20, 70, 0.41, 1, 2, 1),         # strips of two rows: every owned row has a neighbour's row beside it
         (20, 70, 0.30, 2, 3, 2),         # a strip of three under waves of two rows: the last wave of a strip is short
         (30, 130, 0.60, 3, 7, 3),        # three segments, the third holds the right border alone
         (41, 126, 0.41, 4, 11, 0),       # the right border is lane 63 of the last segment; the last strip is short
         (40, 66, 0.10, 7, 40, 40),       # strips of 40 rows: two ranks, each one wave per segment; few ponds, wide basins
         (24, 200, 0.30, 8, 2, 0),
         (20, 70, 0.41, 5, 1, 1),         # strips of one row: a rank whose first owned row is its last, both its neighbours halo rows
         (38, 1, 0.30, 6, 5, 2)]          # one column


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "group_outlets_emu")


@pytest.mark.parametrize("case", NOISE, ids=lambda c: "x".join(map(str, c[:2])) + f"-strips-of-{c[4]}-rpw-{c[5]}")
def test_noise_in_strips_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, "noise", *case)
    assert "table mismatches 0 counts agree" in out and " N 0 " not in out, out
    ranks = int(re.search(r"\((\d+) ranks\)", out).group(1))
    assert ranks >= 2, out
    if case[1] > 1:      # the case crossed a boundary: ponds more than one strip worked on ...
        assert int(re.search(r" split ponds (\d+) ", out).group(1)) > 0, out
    if case[1] > 1 and case[4] <= 3:      # ... and, where every other row lies on a boundary, outlets whose pair lies in two strips
        assert int(re.search(r" seam outlets (\d+) ", out).group(1)) > 0, out


def test_pour_and_merge_alone_on_hand_written_slot_tables(emu):
    """a tie between two ranks (the lower rank's pair wins), a pond only one rank fills and the other finds the pass of, a pond
    without an outlet, a pass across a boundary into basin 0, -0.0 as a pour level, fill_q, fill_cells and divide_cells that
    overflow (a message), a pour level without a pair (a message), a label outside the table, no rank at all"""
    assert "merge checks ok" in emu_build.run(emu, "merge")
