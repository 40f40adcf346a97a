"""The host model of the pond stage curves (tests/pond_curves_model.py) against answers written by hand and against a plain double
loop over cells and stages in Python floats - which round every operation once and fuse nothing - so that the yardstick of
tests/test_pond_curves.py is itself held; and its stage heights against the library's wdpm_curves_stage_level, the one place the
product keeps the rule."""
import math

import numpy as np
import pytest

from helpers import pad, rough_dem
from pond_catchments_model import catchments
from pond_curves_model import STAGES, TooDeep, assert_invariants, curves, stage_levels
from pond_outlets_model import outlets
from pond_rims_model import depth_key, device_dem
from ponds_model import inventory

MISS = -99999.0
WET = 0.001
Q = 2 ** 24


def model(dem, water, md=WET):
    """(curve table, stats, outlet table, basin raster, device dem) of file rasters"""
    bd, bw = pad(np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(water, dtype=np.float64)), MISS)
    labels, ponds = inventory(bd > MISS, bw, md)
    ddem = device_dem(bd, MISS)
    basin, _, _ = catchments(labels, ddem, bw, ponds)
    out, _ = outlets(labels, ddem, bw, ponds, basin=basin)
    table, stats = curves(basin, ddem, out)
    assert_invariants(table, out)
    return table, stats, out, basin, ddem


def key(v):
    return int(depth_key(np.float64(v)).reshape(-1)[0])


def loop_curves(basin, dem, out):
    """the definitions as they are written: every cell, every stage, Python floats and integers"""
    n = len(out)
    bed = [None] * n
    for k, e in zip(basin.ravel().tolist(), dem.ravel().tolist()):
        if k > 0 and (bed[k - 1] is None or key(e) < key(bed[k - 1])):
            bed[k - 1] = e
    cells = [[0] * STAGES for _ in range(n)]
    q = [[0] * STAGES for _ in range(n)]
    for k, e in zip(basin.ravel().tolist(), dem.ravel().tolist()):
        if k <= 0 or not math.isfinite(float(out["pour_level"][k - 1])):
            continue
        z, p = bed[k - 1], float(out["pour_level"][k - 1])
        for s in range(1, STAGES + 1):
            span = p - z
            part = span * (s / 16.0)
            h = p if s == STAGES else z + part
            if key(e) < key(h):
                depth = h - e
                assert depth < 512.0
                cells[k - 1][s - 1] += 1
                t = depth * 2.0 ** 24
                fl = math.floor(t)
                q[k - 1][s - 1] += fl + (1 if t - fl > 0.5 or (t - fl == 0.5 and fl % 2) else 0)     # half to even
    return bed, cells, q


def hold_against_loop(dem, water, md=WET):
    table, stats, out, basin, ddem = model(dem, water, md)
    bed, cells, q = loop_curves(basin, ddem, out)
    assert [key(b) for b in bed] == [key(b) for b in table["bed_level"].tolist()]
    assert table["cells"].tolist() == cells and table["q"].tolist() == q
    assert stats["stage_cells"] == sum(c[STAGES - 1] for c in cells)
    return table, stats


def pyramid(R=39, Cc=39, cy=19, cx=19, water=0.5):
    """a stepped bowl: ground at the Chebyshev distance d from (cy, cx) up to d = 16, the land beyond it half a metre lower and
    falling away: Z = 0, P = 16 and h_s = s exactly"""
    y, x = np.mgrid[0:R, 0:Cc]
    d = np.maximum(abs(y - cy), abs(x - cx)).astype(np.float64)
    dem = np.where(d <= 16, d, 15.5 - (d - 17))
    w = np.zeros((R, Cc))
    w[cy, cx] = water
    return dem, w


def pyramid_row():
    cells = [(2 * s - 1) ** 2 for s in range(1, STAGES + 1)]
    q = [sum((s - d) * (8 * d if d else 1) for d in range(s)) * Q for s in range(1, STAGES + 1)]
    return cells, q


def test_a_stepped_pyramid_computed_by_hand():
    """integer ground and integer stages: a cell at exactly h_s is not counted at s and is counted at s + 1"""
    table, stats, out, _, _ = model(*pyramid())
    assert len(table) == 1 and out["pour_level"][0] == 16.0
    cells, q = pyramid_row()
    assert table["bed_level"][0] == 0.0 and table["top_level"][0] == 16.0
    assert table["cells"][0].tolist() == cells and table["q"][0].tolist() == q
    assert cells[0] == 1 and cells[1] == 9 and cells[15] == 961 and q[0] == Q and q[1] == (2 + 8) * Q
    assert stats == dict(ponds=1, no_curve=0, flat=0, stage_cells=961)
    assert out["fill_cells"][0] == 961 and out["fill_q"][0] == q[15] - Q // 2          # the water on the bed is storage used
    assert stage_levels(0.0, 16.0)[:, 0].tolist() == [float(s) for s in range(17)]


def half_to_even_row():
    return [1.0, 2.0 - 3 * 2.0 ** -25, 2.0 - 2.0 ** -25, 2.0, 1.5], [0.5, 0, 0, 0, 0]


def test_half_to_even():
    """terms of 3 * 2^-25 and 2^-25 are 1.5 and 0.5 quanta: 2 and 0"""
    table, stats, out, basin, _ = model(*half_to_even_row())
    assert basin[1, 1:-1].tolist() == [1, 1, 1, 0, 0] and out["pour_level"][0] == 2.0
    assert table["bed_level"][0] == 1.0 and table["cells"][0][15] == 3 and table["q"][0][15] == Q + 2 + 0
    assert table["cells"][0][:15].tolist() == [1] * 15                               # h_15 = 1.9375 lies below both
    assert table["q"][0][:15].tolist() == [s * Q // 16 for s in range(1, 16)]


def test_no_outlet_flat_and_one_ulp():
    y, x = np.mgrid[0:9, 0:9]
    d2 = (y - 4) ** 2 + (x - 4) ** 2
    table, stats, out, basin, _ = model(50.0 + d2 / 64.0, np.where(d2 <= 1, 0.01, 0.0))       # one basin over everything
    assert np.isposinf(table["top_level"][0]) and table["bed_level"][0] == 50.0 and not table["cells"].any() and not table["q"].any()
    assert stats == dict(ponds=1, no_curve=1, flat=0, stage_cells=0)
    # P == Z: a film too thin to lift the level of its cell, which is the bed and stands beside lower land that ends in a pit
    table, stats, out, _, _ = model([1024.0, 1000.0], [2.0 ** -60, 0.0], md=0.0)
    assert table["top_level"][0] == table["bed_level"][0] == 1024.0 and not table["cells"].any() and not table["q"].any()
    assert stats == dict(ponds=1, no_curve=0, flat=1, stage_cells=0)
    # P one ulp above Z: every stage height is Z or P, and only the last counts the bed for sure
    up = np.nextafter(5.0, 6.0)
    table, stats, out, _, _ = model([5.0, up, 4.0, 4.5], [2.0 ** -60, 0, 0, 0], md=0.0)
    assert out["pour_level"][0] == up and table["bed_level"][0] == 5.0
    h = stage_levels(5.0, up)[:, 0]
    assert set(h.tolist()) == {5.0, up} and h[8] == 5.0 and h[9] == up and table["cells"][0][15] == 1 and not table["q"].any()
    assert table["cells"][0].tolist() == [int(v > 5.0) for v in h[1:]]


def test_signed_zero_bed():
    """a -0.0 bed among +0.0 cells: -0.0 lies below +0.0, and a term of +0.0 - -0.0 is nothing"""
    table, stats, out, _, _ = model([0.0, -0.0, 0.0, 1.0, 0.5, 0.75], [0.25, 0.25, 0.25, 0, 0, 0])
    assert np.signbit(table["bed_level"][0]) and table["bed_level"][0] == 0.0 and out["pour_level"][0] == 1.0
    assert table["cells"][0][15] == 3 and table["q"][0][15] == 3 * Q


def test_too_deep():
    bd, bw = pad(np.array([[0.0, 600.0, 1.0]]), np.array([[500.0, 0.0, 0.0]]), MISS)
    labels, ponds = inventory(bd > MISS, bw, WET)
    ddem = device_dem(bd, MISS)
    basin, _, _ = catchments(labels, ddem, bw, ponds)
    out, _ = outlets(labels, ddem, bw, ponds, basin=basin)           # 100 m below the outlet: the outlets have nothing to say
    assert out["pour_level"][0] == 600.0 and out["fill_q"][0] == 100 * Q
    with pytest.raises(TooDeep):
        curves(basin, ddem, out)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_a_plain_double_loop(seed):
    rng = np.random.default_rng(seed)
    R, Cc = 23, 37
    dem = rough_dem(R, Cc, seed, step=0.125 if seed == 2 else 0.0)
    water = np.where(dem < np.quantile(dem, 0.15), 0.3, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    table, stats = hold_against_loop(dem, water)
    assert len(table) >= 2 and stats["stage_cells"] > 0 and (np.diff(table["cells"], axis=1) > 0).any()
    hold_against_loop(*pyramid())
    hold_against_loop(*half_to_even_row())


def test_stage_levels_are_the_library_s(hip):
    """the model's own heights against wdpm_curves_stage_level, bit for bit, over random pairs and the awkward ones"""
    from wdpm_amd import ponds
    rng = np.random.default_rng(0)
    bed = np.concatenate([rng.normal(500, 300, 300), [0.0, -0.0, 5.0, -1.0, 1e-300, -1e300, 999.9999]])
    top = np.concatenate([bed[:300] + rng.random(300) * 10.0 ** rng.integers(-12, 3, 300), [16.0, 0.0, np.nextafter(5.0, 6.0), 2.0 ** -60, 1e300, 1e300, 1000.0]])
    want = stage_levels(bed, top)
    for i, (z, p) in enumerate(zip(bed.tolist(), top.tolist())):
        got = ponds.stage_levels(z, p, hip)
        assert got.shape == (17,) and got.view(np.uint64).tolist() == want[:, i].view(np.uint64).tolist(), (z, p)
        assert (np.diff(got) >= 0).all() and (got <= p).all()
    assert np.isposinf(ponds.stage_levels(1.0, np.inf, hip)[1:]).all()
