"""The counters behind the benchmark's headline: bench.py divides the milliseconds of wdpm_timing_get / wdpm_timing_get_steady by
their launch counts, so what each call of the block loop adds to the two counts is part of the measurement.  The rules
(wdpm_block.hip: wdpm_iterate, wdpm_iterate_overlapped), per call of n iterations:
  fused kernels   launches += n whether or not iterations went out two per launch; steady launches += n - 2 for n >= 3 (the call's
                  first and last launch may be the flush-on-load and max-diff variants), else 0
  pass kernel     launches += 9 n (nine colour passes an iteration), steady launches stay
  overlapped      the first n - 1 iterations as a fused call of their own, then three windows: launches += (n - 1) + 3
Timed launches are queued one by one: the HIP graph counter stands still.  The expected counts are worked out here from these rules,
never read from the library."""
import numpy as np
import pytest

import wdpm_amd
from helpers import find_drain, pad, random_case

pytestmark = pytest.mark.gpu

THRES = 0.005 / 1000


def fused_rule(n):
    return n, (n - 2 if n >= 3 else 0)


def pass_rule(n):
    return 9 * n, 0


# name -> module, rows, columns, context keywords, rule, extra calls
CONTEXTS = {
    "small-add": ("add", 120, 300, {}, fused_rule),                                  # default dispatch: the small-raster kernels
    "march-add": ("add", 301, 520, dict(chunk_rows=24), fused_rule),                 # marching kernel: tile flags, pairs
    "drain": ("drain", 151, 350, {}, fused_rule),
    "pass-add": ("add", 95, 178, dict(kernel=wdpm_amd.KERNEL_PASS), pass_rule),
}


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_launch_counts_of_every_call(hip, name):
    module, R, C, extra, rule = CONTEXTS[name]
    dem, water, miss = random_case(R * 37 + C, R, C)
    bd, bw = pad(dem, water, miss)
    kw = dict(module=module, nrows=R, ncols=C, missingvalue=miss, **extra)
    if module == "drain":
        dr, dc = find_drain(bd)
        kw.update(drainrow=dr, draincol=dc)
    with hip.context(**kw) as g:
        g.upload(bd, bw)
        graphs = g.get_option(wdpm_amd.capi.OPT_GRAPH_LAUNCHES)
        g.timing_reset()
        want = [0, 0]

        def check(what, launches, steady):
            want[0] += launches
            want[1] += steady
            got = (g.timing()[0], g.timing_steady()[0])
            print(f"{name} {what}: launches {got[0]} (expected {want[0]}), steady {got[1]} (expected {want[1]})")
            assert got == tuple(want), (name, what)

        check("reset", 0, 0)
        for n in (1, 2, 3, 4, 5, 7):
            assert np.isfinite(g.run_block(n, THRES))
            check(f"run_block({n})", *rule(n))
        g.iterate(3)
        check("iterate(3)", *rule(3))
        if name == "march-add":
            # 30 rows at either end of 303 padded rows leave an interior of far more than 24: the three-window launch is used
            g.iterate_overlapped(4, 30, 30)
            check("iterate_overlapped(4, 30, 30)", fused_rule(3)[0] + 3, fused_rule(3)[1])
        if name == "small-add":
            for i in range(300):                  # past the 256 pending event pairs at which they are folded
                g.iterate(1)
            check("300 x iterate(1)", 300 * rule(1)[0], 300 * rule(1)[1])
        ms, steady_ms = g.timing()[1], g.timing_steady()[1]
        print(f"{name}: {ms} ms in all, {steady_ms} ms steady")
        if want[1]:
            assert 0 < steady_ms <= ms
        else:
            assert steady_ms == 0 and ms > 0
        assert g.get_option(wdpm_amd.capi.OPT_GRAPH_LAUNCHES) == graphs
