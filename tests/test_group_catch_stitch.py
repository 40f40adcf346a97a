"""The pond catchments over row blocks on the CPU (include/wdpm_group_pond_catchments.h): tests/group_catch_emu_main.cpp cuts a raster
into strips of rows, gives each strip the labels and the level keys of its neighbours' rows (and rubbish for their DEM and water), runs
the catchment kernels' own source (wdpm_amd/csrc/wdpm_pond_catchments.hip) per strip as host threads on buffers of exact size, follows
the exits and merges the strips' tables with wdpm_amd/csrc/wdpm_catch_stitch.h, and holds basins, table and counts against a plain
loop that walks every descent of the whole raster - all under the address and undefined-behaviour sanitizers, in a program of its
own.  Resolver and merge are also called alone on hand-written seam tables."""
import re

import pytest

import emu_build

# file rows, columns, density, seed, owned rows per strip, rows per wave (0: as the library chooses)
NOISE = [(20, 70, 0.41, 1, 2, 1),         # strips of two rows: every owned row has a neighbour's row beside it
         (20, 70, 0.30, 2, 3, 2),         # a strip of three under waves of two rows: the last wave of a strip is short
         (30, 130, 0.60, 3, 7, 3),        # three segments, the third holds the right border alone
         (41, 126, 0.41, 4, 11, 0),       # the right border is lane 63 of the last segment; the last strip is short
         (38, 1, 0.30, 6, 5, 2),          # one column
         (40, 66, 0.10, 7, 40, 40),       # strips of 40 rows: two ranks, each one wave per segment; few ponds, long descents
         (24, 200, 0.30, 8, 4, 0)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "group_catch_emu")


def agrees(out):
    return "basin mismatches 0 table mismatches 0 counts agree identity holds" in out


@pytest.mark.parametrize("case", NOISE, ids=lambda c: "x".join(map(str, c[:2])) + f"-strips-of-{c[4]}-rpw-{c[5]}")
def test_noise_in_strips_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, "noise", *case)
    assert agrees(out) and " N 0 " not in out, out
    if case[1] > 1:
        assert int(re.search(r" exits (\d+) ", out).group(1)) > 0 and int(re.search(r" crossings (\d+) ", out).group(1)) > 0, out


@pytest.mark.parametrize("R,C,strip,rpw", [(30, 9, 4, 0), (30, 9, 2, 1), (23, 70, 3, 2), (40, 5, 40, 40), (17, 4, 5, 3)])
def test_a_channel_down_and_up_the_columns_crosses_every_boundary_in_both_directions(emu, R, C, strip, rpw):
    out = emu_build.run(emu, "snake", R, C, strip, rpw)
    assert agrees(out) and " N 1 " in out, out
    ranks = int(re.search(r"\((\d+) ranks\)", out).group(1))
    columns = (C + 1) // 2                            # the channel runs along every other column, and crosses every boundary in each
    assert ranks >= 2 and int(re.search(r" crossings (\d+) ", out).group(1)) >= (ranks - 1) * columns, out
    # one pond at an end of the raster: every rank but its own drains to it through exits, and only the rank next to it can border it
    assert ranks - 2 <= int(re.search(r" remote (\d+) ", out).group(1)) <= ranks - 1, out
    assert int(re.search(r" longest descent (\d+) ", out).group(1)) >= (R - 2) * columns, out     # diagonal steps cut every turn short


def test_resolver_and_merge_alone_on_hand_written_seam_tables(emu):
    """a chain back and forth across one boundary three times, one through eight ranks and back, exits onto a pit, a pond and a
    remote pond, a rank of one row, a cycle (an error), an empty raster, counts that overflow (a message)"""
    assert "stitch checks ok" in emu_build.run(emu, "stitch")
