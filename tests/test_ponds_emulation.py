"""The pond kernels' own source (wdpm_amd/csrc/wdpm_ponds.hip) on the CPU: tests/ponds_emu_main.cpp runs every kernel as 256 host
threads per block under the address and undefined-behaviour sanitizers and holds labels and table against a flood fill.  What the
GPU tests cannot say - that no lane reads or writes outside a buffer - is said here, where a stray index harms nobody."""
import pytest

import emu_build

# file rows, columns, density, seed, rows per wave of the table kernel (0: as the library chooses)
CASES = [(20, 70, 0.40, 1, 0),        # two segments, the second nearly empty
         (12, 200, 0.41, 2, 0),       # four segments = one block per row, threshold 0
         (16, 130, 0.60, 3, 3),       # sums carried down three rows
         (3, 700, 0.50, 5, 2),        # wide and flat
         (40, 1, 0.70, 6, 5),         # one column
         (20, 190, 1.00, 8, 7)]       # all wet but the NODATA cells: one table row takes everything
# (more than 1024 segments - a second block of the scan - cost 20 s here as a whole label call.  The three scan kernels alone,
# on made-up counts, run past their tile edges and past 262 144 segments - the second trip of ponds_scan_sums_kernel and its
# carry - in tests/test_pond_scan_emulation.py; tests/test_pond_tall_rasters.py takes whole label calls there on the GPU.)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "ponds_emu")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:2])))
def test_kernels_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, *case)
    assert "label mismatches 0  table mismatches 0" in out, out
