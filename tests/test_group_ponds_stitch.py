"""The pond inventory over row blocks on the CPU: tests/group_ponds_emu_main.cpp, built with the address and undefined-behaviour
sanitizers as tests/test_ponds_emulation.py builds its program, run as a child process.

* the product's stitch header (wdpm_amd/csrc/wdpm_ponds_stitch.h) alone: strips of a raster labelled by a plain flood fill, joined
  by the stitch, held against the flood fill of the whole raster - label raster and merged table;
* the kernels' own source per strip: the existing kernels, the seam kernel, the stitch, the mapping table kernel."""
import re

import pytest

import emu_build

# file rows, columns, strips, density, seed, rows per wave of the table kernel (0: as the library chooses)
KERNEL_CASES = [(24, 70, 3, 0.41, 1, 0),
                (30, 130, 4, 0.60, 3, 3),
                (40, 1, 5, 0.70, 6, 0),
                (20, 190, 2, 1.00, 8, 0)]      # all wet but the NODATA cells


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "group_ponds_emu")


def test_stitch_against_a_flood_fill_of_the_whole_raster(emu):
    """300 x 500 in 2, 3 and 8 strips: noise at three densities, arms and combs joined only in the last (or first) strip with
    isolated cells after them, the transposed serpentine"""
    out = emu_build.run(emu, "stitch")
    lines = out.strip().splitlines()
    assert lines[-1] == "stitch: total mismatches 0" and len(lines) == 1 + 9 + 12
    assert all("label mismatches 0  table mismatches 0" in ln and "DISAGREE" not in ln for ln in lines[:-1]), out
    merged = {ln.split(":")[0] + " " + re.search(r"in (\d+) strips", ln).group(1): int(re.search(r"merged (\d+)", ln).group(1))
              for ln in lines[:-1]}
    assert merged["comb 8"] == 7 * 125 and merged["arms 3"] == 4 and merged["serpentine transposed 2"] == 250


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_kernels_per_strip_on_the_host_under_sanitizers(emu, case):
    out = emu_build.run(emu, "kernels", *case)
    assert "label mismatches 0  table mismatches 0" in out and "DISAGREE" not in out, out
    assert f"in {case[2]} strips" in out
