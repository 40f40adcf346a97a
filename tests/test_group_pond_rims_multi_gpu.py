"""The pond rims over row blocks with one rank per GPU (include/wdpm_group_pond_rims.h): the boundary patterns and the noise of
tests/test_group_pond_rims.py on rowblock.spread_over_devices(torch.cuda.device_count()) - distinct devices that take their rims
side by side, each on its own stream.  Skips itself below two GPUs."""
import pytest

import group_pond_rims_cases as rc
from group_pond_rims_cases import RimCase
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
    with RimCase(hip, R, Cc, devices()) as case:
        slabs = slabs_of(hip, R, case.n)
        rc.run_foreign(case, slabs)
        rc.run_counted_once_and_four_ponds(case, slabs)
        rc.run_ties(case, slabs)
        rc.run_shared_slots(case)
        rc.run_serpentine(case, slabs)


def test_noise(hip):
    with RimCase(hip, 131, 385, devices()) as case:
        rc.run_noise(case)
    with RimCase(hip, 257, 515, devices()[:5], every=None) as case:
        rc.run_noise(case)
