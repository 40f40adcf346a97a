"""The pond outlets over row blocks with one rank per GPU (include/wdpm_group_pond_outlets.h): the boundary patterns and the noise of
tests/test_group_pond_outlets.py on rowblock.spread_over_devices(torch.cuda.device_count()) - distinct devices that take their passes
side by side, each on its own stream.  Skips itself below two GPUs."""
import pytest

import group_pond_outlets_cases as oc
from group_pond_outlets_cases import OutletCase
from group_ponds_cases import slabs_of
from wdpm_amd.rowblock import spread_over_devices


def ndev():
    """GPUs on this box; counting them does not initialise any.  A torch that cannot be imported or asked is an error, no skip."""
    import torch
    return int(torch.cuda.device_count())


NDEV = ndev()
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NDEV < 2, reason=f"{NDEV} GPU: needs two or more")]
SHAPES = [(67, 193), (131, 385)]


def devices():
    return spread_over_devices(NDEV)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_boundary_patterns(hip, R, Cc):
    with OutletCase(hip, R, Cc, devices()) as case:
        slabs = slabs_of(hip, R, case.n)
        oc.run_lines_across(case, slabs)
        oc.run_ties_across(case, slabs)
        if case.n >= 3:
            oc.run_long_basin(case, slabs)
        oc.run_remote(case, slabs)
        oc.run_columns(case, slabs)
        oc.run_not_quiet(case, slabs)
        oc.run_seam_levels(case, slabs)


def test_noise(hip):
    with OutletCase(hip, 131, 385, devices()) as case:
        oc.run_noise(case)
