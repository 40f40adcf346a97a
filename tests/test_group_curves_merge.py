"""The pond stage curves over row blocks on the CPU (include/wdpm_group_pond_curves.h): tests/group_curves_emu_main.cpp cuts a raster into
strips of rows, gives each strip the DEM and the basins of its owned rows (and rubbish for the rows beside them: ground far below every
bed, basins that name the strip's own slots), runs the curve kernels' own source (wdpm_amd/csrc/wdpm_pond_curves.hip) per strip as host
threads on buffers of exact size, makes the beds final and merges the strips' tables with wdpm_amd/csrc/wdpm_curves_merge.h, and holds
table and counts against a plain double loop over all cells and stages of the whole raster - all under the address and
undefined-behaviour sanitizers, in a program of its own.  Both merges are also called alone on hand-written slot tables."""
import re

import pytest

import emu_build

# file rows, columns, density, seed, owned rows per strip, rows per wave (0: as the library chooses)
NOISE = [(20, 70, 0.41, 1, 1, 1),         # strips of one row: a rank whose first owned row is its last, both its neighbours halo rows
         (20, 70, 0.41, 5, 2, 1),         # strips of two rows: every owned row has a neighbour's row beside it
         (20, 70, 0.30, 2, 3, 2),         # a strip of three under waves of two rows: the last wave of a strip is short
         (30, 130, 0.60, 3, 7, 3),        # three segments, the third holds the right border alone
         (41, 126, 0.41, 4, 11, 0),       # the right border is lane 63 of the last segment; the last strip is short
         (40, 66, 0.10, 7, 40, 40),       # strips of 40 rows: two ranks, each one wave per segment; few ponds, wide basins
         (80, 66, 0.30, 9, 40, 3),
         (24, 200, 0.30, 8, 2, 0),
         (23, 70, 0.41, 11, 7, 40),       # more rows per wave than a strip holds
         (38, 1, 0.30, 6, 1, 1),          # one column, at every strip height
         (38, 1, 0.30, 6, 2, 2),
         (38, 1, 0.30, 6, 3, 0),
         (38, 1, 0.30, 6, 7, 3),
         (38, 1, 0.30, 6, 11, 40),
         (80, 1, 0.30, 6, 40, 2)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "group_curves_emu")


@pytest.mark.parametrize("case", NOISE, ids=lambda c: "x".join(map(str, c[:2])) + f"-strips-of-{c[4]}-rpw-{c[5]}")
def test_noise_in_strips_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, "noise", *case)
    assert "table mismatches 0 counts agree" in out and " N 0 " not in out, out
    ranks = int(re.search(r"\((\d+) ranks\)", out).group(1))
    assert ranks >= 2, out
    if case[1] > 1:      # the case crossed a boundary: basins whose cells lie in more than one strip ...
        assert int(re.search(r" split basins (\d+) ", out).group(1)) > 0, out
        assert " stage cells 0 " not in out, out
    if case[1] > 1 and case[4] <= 11:      # ... and, where boundaries lie close (the basins of this noise are small), stage cells away from the bed
        assert int(re.search(r" remote beds (\d+) ", out).group(1)) > 0, out


def test_bed_and_merge_alone_on_hand_written_slot_tables(emu):
    """a bed in the last rank with stage cells in the first (remote), a tie at -0.0 between two ranks (the lower rank holds the bed), a
    rank that holds a slot and no cell, a pond without an outlet (its bed, and zeros whatever the slots hold), a flat pond through a
    remote slot, a split basin that is not remote; a q and a cell count that would leave 64 bits (a message), tops that differ, a pond
    nobody holds, a label outside the table, no rank at all"""
    assert "merge checks ok" in emu_build.run(emu, "merge")
