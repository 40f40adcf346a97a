"""The pond stage curves over row blocks with one rank per GPU (include/wdpm_group_pond_curves.h): the boundary scenes and the denser
inputs of tests/test_group_pond_curves.py on rowblock.spread_over_devices(torch.cuda.device_count()) - distinct devices that take
their passes side by side, each on its own stream.  Skips itself below two GPUs."""
import pytest

import group_pond_curves_cases as cc
from group_pond_curves_cases import CurveCase
from group_ponds_cases import slabs_of
from wdpm_amd.rowblock import spread_over_devices


def ndev():
    """GPUs on this box; counting them does not initialise any.  A torch that cannot be imported or asked is an error, no skip."""
    import torch
    return int(torch.cuda.device_count())


NDEV = ndev()
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NDEV < 2, reason=f"{NDEV} GPU: needs two or more")]


def devices():
    return spread_over_devices(NDEV)


@pytest.mark.parametrize("R,Cc", [(67, 193), (131, 385)])
def test_boundary_scenes(hip, R, Cc):
    with CurveCase(hip, R, Cc, devices()) as case:
        slabs = slabs_of(hip, R, case.n)
        cc.run_remote_bed(case, slabs)
        cc.run_edges(case, slabs)
        cc.run_stripes(case)
        cc.run_degenerate(case, slabs)


def test_noise_and_smooth_bowls(hip):
    with CurveCase(hip, 131, 385, devices()) as case:
        cc.run_noise(case)
        cc.run_smooth_bowls(case)
