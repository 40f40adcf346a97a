"""The binary-grid search of wdpm_dem_codes.hip::encode_dem as a numpy model (tests/binary_dem_model.py) held against exact rational
arithmetic: the lowest-set-bit scan, the accept / refuse rule and the decode.  No GPU needed; tests/test_binary_dem.py holds the
device against this model."""
from fractions import Fraction

import numpy as np
import pytest

from binary_dem_model import EDGE_EXPECT, MISS, codes, edge_cases, f32, largest_group_span, lowest_bit_exponent, model_grid
from helpers import pad, random_case


def test_lowest_set_bit_exponent_against_exact_arithmetic():
    rng = np.random.default_rng(1)
    tiny = np.array([5e-324, 1.5e-323, 2.2250738585072014e-308, 2.225073858507201e-308, 1e-310, -3e-320])   # subnormals and the first normal
    v = np.concatenate([tiny, [1.0, -1.0, 3.0, 0.75, 2.0 ** 60, -(2.0 ** -40) * 5, 1e300, 1.7976931348623157e308],
                        f32(500 + rng.normal(0, 3, 200)), rng.normal(0, 1, 200), rng.integers(1, 2 ** 53, 100).astype(np.float64)])
    for x, t in zip(v.tolist(), lowest_bit_exponent(v).tolist()):
        m = Fraction(x) / Fraction(2) ** t
        assert m.denominator == 1 and m.numerator % 2 == 1, (x, t)
    assert lowest_bit_exponent(np.array([5e-324]))[0] == -1074 and lowest_bit_exponent(np.array([1.7976931348623157e308]))[0] == 971


@pytest.mark.parametrize("level,noise", [(500.0, 3.0), (-120.0, 3.0), (3000.0, 40.0), (12.5, 0.4), (0.0, 2.0), (1900.0, 300.0)])
def test_accepted_float32_rasters_decode_to_their_own_bits(level, noise):
    rng = np.random.default_rng(int(abs(level)) + 7)
    for _ in range(4):
        dem = f32(level + rng.normal(0, noise, (23, 61)))
        grid, s, info = model_grid(dem)
        lo = -int(lowest_bit_exponent(dem[dem != 0]).min())
        if grid == 0:                                        # values near zero make the common grid too fine for 31 bits of relief
            assert info["s"] == lo and (info.get("relief", 0) >= 2147483647.0 or abs(info["k0"]) >= 4e15 or not 1 <= lo <= 52), info
            continue
        assert (grid, s) == (2, lo) and 1 <= s <= 52
        k0, q = codes(dem, grid, s)
        assert float(k0).is_integer() and abs(k0) < 4e15 and int(np.abs(q).max()) < 2 ** 31 - 1
        for x, k in zip(dem.ravel().tolist(), q.ravel().tolist()):
            assert Fraction(k + int(k0), 2 ** s) == Fraction(x)       # the decode n * 2^-s is exact: no rounding anywhere
        # ... and the two floating-point operations of the decoder give exactly that: (double)q + k0 and the scaling are exact
        back = (q.astype(np.float64) + k0) * 2.0 ** -s
        assert np.array_equal(back.view(np.uint64), dem.view(np.uint64))


def test_float32_rasters_at_the_level_of_the_tests_are_accepted():
    rng = np.random.default_rng(3)
    assert model_grid(f32(500 + rng.normal(0, 3, (40, 230))))[:2] == (2, 15)
    assert model_grid(f32(500 + rng.normal(0, 3, (40, 230))), binary=False)[:2] == (0, 0)      # WDPM_DEM_BINARY=0: the decimal grids alone


def test_refusals_that_existing_tests_rely_on_stay_refusals():
    # tests/test_hip_parity.py::test_dem_codes_are_refused_for_non_decimal_elevations
    dem, _, miss = random_case(77, 60, 400)
    valid = dem > miss
    grid, e, info = model_grid(dem[valid] * (1.0 + 2.0 ** -30))
    assert (grid, e) == (0, 0) and info["s"] == 44 and 4e15 <= abs(info["k0"]) and 8.6e15 < abs(info["k0"]) < 8.9e15 and "relief" not in info
    d = dem[valid] * (1.0 + 2.0 ** -30)
    assert 1.7e14 < (d.max() - d.min()) * 2.0 ** 44 < 1.9e14                                   # and the relief would not fit either
    # the four-decimal DEM itself: decimal as before; its binary side is no grid a raster fits on
    assert model_grid(dem[valid])[:2] == (10, 4)
    assert -int(lowest_bit_exponent(dem[valid]).min()) == 44 and abs(np.rint(dem[valid].min() * 2.0 ** 44)) >= 4e15
    # tests/test_hip_parity.py::test_dem_code_edge_cases, the cases that expect 0 (same generator, same order of draws)
    rng = np.random.default_rng(5)
    R, C = 40, 230
    base = rng.normal(0, 3, (R, C))
    for name in ("six_digits_high", "needs_offset", "relief_too_large", "negative", "neg_zero", "mixed_digits", "integers", "huge"):
        dem, want = {
            "six_digits_high": lambda: (np.round(1500.0 + base, 6), 1),
            "needs_offset": lambda: (np.round(3000.0 + base, 6), 1),
            "relief_too_large": lambda: (np.where(rng.random((R, C)) < 0.5, 1e-6, 5000.000001), 0),
            "negative": lambda: (np.round(-12.0 + base, 3), 1),
            "neg_zero": lambda: (np.where(rng.random((R, C)) < 0.01, -0.0, np.round(3.0 + base, 2)), 0),
            "mixed_digits": lambda: (np.where(rng.random((R, C)) < 0.5, np.round(400 + base, 1), np.round(400 + base, 5)), 1),
            "integers": lambda: (np.round(700.0 + base, 0), 1),
            "huge": lambda: (np.where(rng.random((R, C)) < 0.02, 1e300, np.round(10 + base, 2)), 0),
        }[name]()
        grid = model_grid(dem)[0]
        assert (grid != 0) == bool(want) and grid in (0, 10), (name, grid)


def test_edge_case_table_is_what_the_gpu_tests_expect():
    for name, dem in edge_cases().items():
        grid, exp, info = model_grid(dem[dem > MISS])
        want_grid, want_exp = EDGE_EXPECT[name]
        assert grid == want_grid and (want_exp is None or exp == want_exp), (name, grid, exp, info)
    for name, s in (("f32_with_1e-3", 33), ("f32_mix_half_70000", 25)):       # refused for their relief, on the grid the scan finds
        dem = edge_cases()[name]
        info = model_grid(dem[dem > MISS])[2]
        assert info["s"] == s and info["relief"] >= 2 ** 31, (name, info)


def test_group_spans_decide_the_16_bit_offsets():
    """the two rasters of the 16-bit test: gentle terrain fits 65 534 quanta per 48 columns at 2^-15 m, 3 m of noise does not"""
    import coverage_worker as cw
    dem, _ = cw.make_case(60, 400, 60 * 7 + 400)
    gentle = np.where(dem > MISS, f32(dem), dem)
    bd, _ = pad(gentle, np.zeros_like(gentle), MISS)
    assert model_grid(gentle[gentle > MISS])[:2] == (2, 15)
    assert largest_group_span(bd, 2, 15) <= 65534
    rng = np.random.default_rng(11)
    rough = f32(500 + rng.normal(0, 3, (60, 400)))
    bd, _ = pad(rough, np.zeros_like(rough), MISS)
    assert model_grid(rough)[:2] == (2, 15)
    assert largest_group_span(bd, 2, 15) > 65534
