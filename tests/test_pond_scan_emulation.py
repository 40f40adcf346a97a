"""The three scan kernels of wdpm_amd/csrc/wdpm_ponds.hip alone on the CPU: tests/scan_emu_main.cpp fills the per-segment counts
with random numbers, runs reduce, sums and down as 256 host threads per block under the address and undefined-behaviour sanitizers
and holds the result against a sequential prefix sum.  ponds_scan_sums_kernel walks the block sums in trips of 256 with a carry
between trips: a second trip wants more than 256 scan blocks of 1024 segments, which no whole label call of the host emulations
reaches (tests/test_ponds_emulation.py) - the counts alone do."""
import pytest

import emu_build

TILE = 1024            # segments per scan block (kScanTile)
TRIP = 256 * TILE      # segments per trip of ponds_scan_sums_kernel

# segments, seed, "zero" for all-zero counts
CASES = [(1, 1, ""),
         (TILE - 1, 2, ""), (TILE, 3, ""), (TILE + 1, 4, ""),      # the edges of one scan block
         (TRIP, 5, ""),                                            # exactly 256 blocks: one full trip
         (TRIP + 1, 6, ""),                                        # one entry in the second trip: its number is the carry
         (300007, 7, ""),                                          # a ragged second trip, a ragged last block
         (TRIP + 1, 8, "zero")]                                    # nothing to count anywhere


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "scan_emu")


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[2]}")
def test_scan_kernels_on_the_host_under_sanitizers(emu, case):
    nseg, seed, zero = case
    out = emu_build.run(emu, nseg, seed, *([zero] if zero else []))
    assert f"{nseg} segments, {-(-nseg // TILE)} scan blocks, {-(-nseg // TRIP)} trips" in out, out
    assert "scan mismatches 0 (first at -1)  status mismatches 0" in out, out
    if zero:
        assert "ponds 0 (reference 0) unions 0 (0) seam 0 (0)" in out, out
