"""A numpy model of what wdpm_dem_codes.hip::encode_dem decides for an uploaded DEM, and the rasters the binary-grid tests share.

The library expresses a DEM as 32-bit codes q with dem == (q + k0) / D bit for bit: first D = 10^e, e = 0..6; then, when all
seven fail, once D = 2^s, 2^-s being the weight of the lowest bit set in any valid non-zero elevation (dem_min_kernel), if
1 <= s <= 52 and |k0| < 4e15.  Every attempt is verified cell by cell (dem_encode_kernel): the code must fit 32 bits and decode
to the cell's own bits.  The decode fma(n, rD, n * rDlo) is RN(n / D) (tests/test_decode_forms.py) - here the correctly rounded
float division - and n * 2^-s exactly on a binary grid.

model_grid(values) -> (grid, exponent, info): (10, e), (2, s) or (0, 0), with the figures behind a refusal in info."""
import numpy as np

MISS = -99999.0
P10 = [1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6]


def lowest_bit_exponent(v):
    """t(v) per element: v is an odd multiple of 2^t.  v finite and non-zero; subnormals have exponent field 0, which stands for 1
    without the implicit bit"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) & np.uint64(0x7fffffffffffffff)
    ex = (b >> np.uint64(52)).astype(np.int64)
    sig = (b & np.uint64(0x000fffffffffffff)) | np.where(ex > 0, np.uint64(1) << np.uint64(52), np.uint64(0))
    low = sig & (~sig + np.uint64(1))                         # the lowest set bit, a power of two below 2^53: exact as a double
    tz = np.log2(low.astype(np.float64)).astype(np.int64)
    return np.maximum(ex, 1) - 1075 + tz


def _verified(v, k0, D, decode):
    """dem_encode_kernel: every code fits 32 bits and decodes to the cell's own bits; (ok, largest |code|)"""
    with np.errstate(over="ignore", invalid="ignore"):
        kk = np.rint(v * D) - k0
        fits = np.abs(kk) < 2147483647.0
        code = np.where(fits, kk, 0.0)
        same = decode(code + k0).view(np.uint64) == v.view(np.uint64)
    return bool((fits & same).all()), float(np.abs(kk).max())


def model_grid(values, binary=True):
    """values: the valid elevations (any shape).  binary=False: WDPM_DEM_BINARY=0"""
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    info = {}
    if v.size == 0:
        return 0, 0, info
    vmin = float(v.min())
    with np.errstate(over="ignore", invalid="ignore"):
        for e, D in enumerate(P10):
            k0 = float(np.rint(vmin * D))
            if not abs(k0) < 4.0e15:
                break
            ok, _ = _verified(v, k0, D, lambda n, D=D: n / D)
            if ok:
                return 10, e, info
        nz = v[v != 0.0]                                      # +0.0 and -0.0 alike: zeros lie on every grid
        if not binary or nz.size == 0:
            return 0, 0, info
        s = -int(lowest_bit_exponent(nz).min())
        info["s"] = s
        if not 1 <= s <= 52:
            return 0, 0, info
        D = float(2.0 ** s)
        k0 = float(np.rint(vmin * D))
        info["k0"] = k0
        if not abs(k0) < 4.0e15:
            return 0, 0, info
        ok, relief = _verified(v, k0, D, lambda n: n * (1.0 / D))
        info["relief"] = relief
    return (2, s, info) if ok else (0, 0, info)


def codes(values, grid, exp):
    """(k0, integer codes) of an accepted DEM"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    D = float(grid) ** exp
    k0 = float(np.rint(float(v.min()) * D))
    return k0, (np.rint(v * D) - k0).astype(np.int64)


def largest_group_span(bigdem, grid, exp, group=48):
    """the largest span of codes over the valid cells of one group of 48 padded columns of a row (dem16_encode_kernel accepts <= 65534)"""
    valid = bigdem > MISS
    _, q = codes(np.where(valid, bigdem, bigdem[valid].min()), grid, exp)
    span = 0
    for c0 in range(0, bigdem.shape[1], group):
        qs, ok = q[:, c0:c0 + group], valid[:, c0:c0 + group]
        hi = np.where(ok, qs, np.iinfo(np.int64).min).max(axis=1)
        lo = np.where(ok, qs, np.iinfo(np.int64).max).min(axis=1)
        rows = ok.any(axis=1)
        if rows.any():
            span = max(span, int((hi - lo)[rows].max()))
    return span


def f32(a):
    """elevations as a Float32 raster holds them, widened back to fp64 (exact)"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def f32_keep_nodata(dem):
    return np.where(dem > MISS, f32(dem), dem)


def edge_cases(R=40, C=230):
    """name -> DEM (4 % NODATA) of the edge-case table; one generator, drawn from in this order"""
    rng = np.random.default_rng(5)
    base = rng.normal(0, 3, (R, C))
    pick = lambda frac: rng.random((R, C)) < frac            # noqa: E731
    out = {
        "f32_500": f32(500 + base),
        "f32_mix_250_515": f32(np.where(pick(0.5), 250 + base, 515 + base)),
        "f32_negative": f32(-120 + base),
        "f32_with_zeros": np.where(pick(0.05), 0.0, f32(300 + base)),
        "f32_with_neg_zeros": np.where(pick(0.05), -0.0, f32(300 + base)),
        "f32_with_1e-3": np.where(pick(0.05), float(np.float32(1e-3)), f32(300 + base)),
        "f32_mix_half_70000": f32(np.where(pick(0.5), 0.5 + 0.01 * base, 70000 + base)),
        "multiples_of_1_128": np.round((500 + base) * 128) / 128,
        "multiples_of_1_4": np.round((700 + base) * 4) / 4,
        "f16_500": np.asarray(500 + base, dtype=np.float16).astype(np.float64),
    }
    for name in out:
        dem = out[name].copy()
        dem[pick(0.04)] = MISS
        out[name] = dem
    return out


# what the model gives for them: (grid, exponent); None: whatever binary exponent the model finds
EDGE_EXPECT = {
    "f32_500": (2, 15), "f32_mix_250_515": (2, 16), "f32_negative": (2, None), "f32_with_zeros": (2, 15),
    "f32_with_neg_zeros": (0, 0), "f32_with_1e-3": (0, 0), "f32_mix_half_70000": (0, 0), "multiples_of_1_128": (2, 7),
    "multiples_of_1_4": (10, 2), "f16_500": (10, 2),
}
