"""One pond handle over waters of very different pond counts: buffers that grow, stay and are used again (the holders of
wdpm_amd/csrc/wdpm_ponds_priv.h).  The unit tests give every handle one water, so a later call never outgrows the tables of the
first; here five waters follow each other on one DEM - a few ponds, many, none, more than ever before, a few again.

Whole raster: label_curves (which runs all five units) and every table against the host models the unit tests use.  Row blocks:
label_outlets on 2 and 3 ranks, the four merged tables against a whole-raster handle on the same water, byte for byte, and against
the models through tests/group_pond_outlets_cases.py; then a call that fails (a 600 m pit) between two calls on the largest
water.  Every comparison is equality; no guard byte may change.  46 x 70 file cells: two segments, padded column 63 | 64 the lanes
63 | 0."""
import math

import numpy as np
import pytest

import group_pond_rims_cases as rc
from group_pond_outlets_cases import OutletCase
from group_ponds_cases import MISS, WET, slabs_of
from helpers import pad
from pond_outlets_model import TooDeep, outlets
from pond_catchments_model import catchments
from pond_rims_model import assert_same_rims, device_dem, rims
from ponds_model import inventory
from test_pond_catchments import hold_against_model as hold_catchments, taken
from test_pond_curves import hold_against_model as hold_curves
from test_pond_outlets import hold_against_model as hold_outlets

pytestmark = pytest.mark.gpu
R, CC = 46, 70


def scene():
    """the DEM and the five waters in file layout, and their pond counts by the model"""
    dem = rc.ramp_dem(R, CC)
    few = np.zeros((R, CC))
    few[5:9, 10:20] = 0.3                       # within a segment
    few[20:24, 58:68] = 0.3                     # across padded columns 63 | 64
    few[40:46, 0:4] = 0.3                       # in the raster's corner
    many = np.where(np.random.default_rng(12).random((R, CC)) < 0.10, 0.3, 0.0)
    more = np.zeros((R, CC))
    more[::2, ::2] = 0.3                        # a pond on every second cell of every second row: no raster of this shape holds more
    again = np.zeros((R, CC))
    again[12:15, 30:40] = 0.3
    again[30:33, 61:66] = 0.3
    waters = [few, many, np.zeros((R, CC)), more, again]
    bd = pad(dem, few, MISS)[0]
    counts = [len(inventory(bd > MISS, pad(dem, w, MISS)[1], WET)[1]) for w in waters]
    return dem, waters, counts


def assert_counts_grow(counts):
    few, many, none, more, again = counts
    assert few >= 2 and many >= 10 * few and none == 0 and more > many and 2 <= again < many, counts


@pytest.mark.parametrize("env", [{}, {"WDPM_PONDS_ROWS_PER_WAVE": "1"}, {"WDPM_PONDS_TIMING": "1"}], ids=["default", "rpw1", "timing"])
def test_five_waters_on_one_whole_raster_handle(hip, monkeypatch, env):
    from wdpm_amd.ponds import CATCH_PHASES, CURVE_PHASES, OUTLET_PHASES, PHASES, RIM_PHASES, Ponds
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dem, waters, counts = scene()
    assert_counts_grow(counts)
    largest = 0
    with hip.context(module="add", nrows=R, ncols=CC, missingvalue=MISS) as ctx:
        with Ponds(ctx) as p:
            for water, count in zip(waters, counts):
                bd, bw = pad(dem, water, MISS)
                ctx.upload(bd, bw)
                n = p.label_curves(WET)
                assert n == count
                ref_labels, ddem = hold_catchments(bd, MISS, bw, WET, taken(p), n)     # labels, pond table, basins, catchments
                assert_same_rims(p.rims(), rims(ref_labels, ddem, bw, n))
                hold_outlets(bd, MISS, bw, WET, p, n)
                hold_curves(bd, MISS, bw, WET, p, n)
                if "WDPM_PONDS_ROWS_PER_WAVE" in env:
                    assert p.stats()["rows_per_wave"] == 1
                if "WDPM_PONDS_TIMING" in env and n > largest:                          # a call that made every table grow
                    for ms, names in ((p.phase_ms(), PHASES), (p.rims_phase_ms(), RIM_PHASES), (p.catchment_phase_ms(), CATCH_PHASES),
                                      (p.outlet_phase_ms(), OUTLET_PHASES), (p.curve_phase_ms(), CURVE_PHASES)):
                        assert tuple(ms) == names and all(math.isfinite(v) and v >= 0 for v in ms.values()), ms
                largest = max(largest, n)
            assert p.guard_bad() == 0


def four_tables(p):
    return p.table(), p.rims(), p.catchments(), p.outlets()


def check_against_whole(case, dem, water):
    """label_outlets on the group: against the models and a twin group (OutletCase.check), and the four merged tables against the
    whole-raster handle, which OutletCase.check has just had label the same water"""
    table, _, _, _ = case.check(water, dem)
    assert case.whole.stats()["ponds"] == len(table)
    for mine, theirs in zip(four_tables(case.ponds), four_tables(case.whole)):
        assert mine.tobytes() == theirs.tobytes()
    assert case.ponds.guard_bad() == 0 and case.whole.guard_bad() == 0
    return len(table)


@pytest.mark.parametrize("n", [2, 3])
def test_five_waters_on_one_row_block_handle_and_a_failed_call_between_two_growths(hip, n):
    import wdpm_amd
    dem, waters, counts = scene()
    assert_counts_grow(counts)
    with OutletCase(hip, R, CC, [0] * n) as case:
        for water, count in zip(waters, counts):
            assert check_against_whole(case, dem, water) == count
        # the scene of test_group_pond_outlets.test_a_600_m_pit_on_one_rank_fails_the_whole_call: a pit of one cell 600 m down in the
        # last rank's rows, a pond in it
        w, nodata = rc.noise(R, CC, 0.41, 5)
        deep = rc.ramp_dem(R, CC, nodata=nodata)
        r = slabs_of(hip, R, n)[n - 1].own_lo + 2
        deep[r - 1, 21] = -500.0
        w[r - 1, 21] = 0.5
        bd, bw = pad(deep, w, MISS)
        labels, ponds = inventory(bd > MISS, bw, WET)
        with pytest.raises(TooDeep):
            outlets(labels, device_dem(bd, MISS), bw, ponds, basin=catchments(labels, device_dem(bd, MISS), bw, ponds)[0])
        case.upload(w, deep)
        with pytest.raises(wdpm_amd.WdpmError, match="512 m"):
            case.ponds.label_outlets(WET)
        assert case.ponds.guard_bad() == 0
        assert check_against_whole(case, dem, waters[3]) == counts[3]
