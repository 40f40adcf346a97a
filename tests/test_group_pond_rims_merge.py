"""The pond rims over row blocks on the CPU (include/wdpm_group_pond_rims.h): tests/group_rims_emu_main.cpp cuts a raster into strips
of rows, gives each strip the labels of its neighbours' rows (and rubbish for their DEM and water), runs the rim kernels' own source
(wdpm_amd/csrc/wdpm_pond_rims.hip) per strip as host threads on buffers of exact size, merges the strips' rim rows with
wdpm_amd/csrc/wdpm_rims_merge.h and holds the table against a plain loop over the whole raster - all under the address and
undefined-behaviour sanitizers, in a program of its own.  The merge is also called alone on hand-written rank tables."""
import pytest

import emu_build

# file rows, columns, density, seed, owned rows per strip, rows per wave (0: as the library chooses)
NOISE = [(20, 70, 0.41, 1, 2, 0),         # strips of two rows: every owned row has a neighbour's row beside it
         (20, 70, 0.30, 2, 3, 2),         # a strip of three under waves of two rows: the last wave of a strip is short
         (30, 130, 0.60, 3, 7, 0),        # three segments, the third holds the right border alone
         (41, 126, 0.41, 4, 11, 7),       # the right border is lane 63 of the last segment; the last strip is short
         (38, 1, 0.70, 6, 5, 2),          # one column
         (40, 66, 0.50, 7, 40, 1000),     # strips of 40 rows: two ranks, each one wave per segment
         (24, 200, 1.00, 8, 4, 0)]        # all wet but the NODATA cells: one pond through every strip


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "group_rims_emu")


@pytest.mark.parametrize("case", NOISE, ids=lambda c: "x".join(map(str, c[:2])) + f"-strips-of-{c[4]}")
def test_noise_in_strips_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, "noise", *case)
    assert "rim mismatches 0" in out and " N 0 " not in out, out
    if case[2] < 0.5:                             # many small ponds: some lie beside a strip without entering it
        assert " foreign 0 " not in out, out


@pytest.mark.parametrize("strip,rpw", [(4, 0), (4, 2), (2, 0), (3, 7), (8, 0), (40, 0)])
def test_hand_made_ponds_on_the_boundaries(emu, strip, rpw):
    """a foreign pond whose lowest rim cell lies across the boundary (and mirrored upward), a dry cell that touches one pond from
    both sides of a boundary, ties of the rim level across strips with both zeros, walls only, two arms joined in the next strip,
    ponds on the raster's first and last row"""
    out = emu_build.run(emu, "cases", strip, rpw)
    assert "rim mismatches 0" in out and " N 10 " in out and "without a rim 1 " in out, out
    if strip == 4:
        assert " foreign 3 " in out, out          # the two foreign ponds of the pattern, and the walled cell's ring from above


def test_the_merge_alone_on_hand_written_rank_tables(emu):
    """a tie, signed zeros on either side, no rim anywhere, a foreign row, an empty slot, counts that overflow (a message)"""
    assert "merge checks ok" in emu_build.run(emu, "merge")
