"""The pond inventory over row blocks with one rank per GPU (include/wdpm_group_ponds.h): the lines, the joined-far-away patterns
and the noise of tests/test_group_ponds.py on rowblock.spread_over_devices(torch.cuda.device_count()) - distinct devices that
label side by side, each on its own stream.  Skips itself below two GPUs."""
import pytest

import group_ponds_cases as gc
from group_ponds_cases import GroupCase, slabs_of
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
def test_lines_across_every_boundary(hip, R, Cc):
    with GroupCase(hip, R, Cc, devices()) as case:
        gc.run_lines(case, slabs_of(hip, R, case.n))


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_joined_only_far_below_or_above(hip, R, Cc):
    with GroupCase(hip, R, Cc, devices()) as case:
        gc.run_joined_far_away(case)


def test_noise(hip):
    with GroupCase(hip, 131, 385, devices()) as case:
        gc.run_noise(case)
    with GroupCase(hip, 257, 515, devices()[:5], every=None) as case:
        gc.run_noise(case)
