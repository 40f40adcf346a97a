"""TEST INFRASTRUCTURE: the ground and water of tests/test_pond_spills.py, as file rasters (dem, water).  Heights are multiples of
1/8 m, so every level, pass and headroom is exact.  NODATA is MISS.  What each scene must give is asserted on the model by the test
that uses it, before the device is asked."""
import numpy as np

MISS = -99999.0


def staircase(steps=95, rows=5, full=lambda i: i % 3 != 0):
    """`steps` bowls down a staircase, three columns each and `rows` rows deep: a ridge at R = 2000 - i, a floor 5/8 m below it
    under 1/8 m of water - or 3/8 m where full(i): then it stands exactly at its pass - and a slope 1/4 m below the ridge that
    already drains to the next bowl.  Bowl i's lowest pass is that slope: pond i + 1 -> pond i + 2, a chain; the last bowl can only
    spill back."""
    i = np.arange(steps)
    ridge = 2000.0 - i
    dem = np.stack([ridge, ridge - 0.625, ridge - 0.25], axis=1).ravel()
    water = np.stack([0 * ridge, np.where([full(k) for k in i], 0.375, 0.125), 0 * ridge], axis=1).ravel()
    return np.tile(dem, (rows, 1)), np.tile(water, (rows, 1))


def column(steps=6667, width=3):
    """the staircase turned by a quarter: three columns wide, one pond every three rows down `steps` steps of 1 m"""
    dem, water = staircase(steps, rows=width, full=lambda i: i % 5 != 0)
    return np.ascontiguousarray((dem + 10000.0).T), np.ascontiguousarray(water.T)


def hub(cols=385):
    """A lake along the middle row (floor 5 m, 1 m of water), a dry rim at 11 m either side of it, and beyond each rim a row of pits
    (floor 10 m) between walls of 12 m, every second pit filled to the rim: every pit spills over the rim into the lake.  The lake
    leaves over a sill of 8 m at its right end into a dry pit: land."""
    dem = np.empty((5, cols))
    water = np.zeros((5, cols))
    c = np.arange(cols)
    pit = c % 2 == 0
    for r in (0, 4):
        dem[r] = np.where(pit, 10.0, 12.0)
        water[r] = np.where(pit, np.where(c % 4 == 0, 1.0, 0.125), 0.0)
    dem[1] = dem[3] = 11.0
    dem[2], water[2] = 5.0, 1.0
    dem[2, -3], water[2, -3] = 8.0, 0.0            # the sill
    dem[2, -2:], water[2, -2:] = 1.0, 0.0          # the dry pit behind it
    return dem, water


def pair():
    """two bowls and one saddle between walls: each spills into the other"""
    return np.array([[20.0, 10.0, 12.0, 9.0, 20.0]]), np.array([[0, 0.5, 0, 0.5, 0]])


def ring_of_three():
    """Three bowls (floors at 10 m under 1/2 m of water: one cell top right, one cell in the middle, three cells along the bottom)
    among NODATA, joined by cells at 11.5 m and 12 m so that every pond pours at the same level.  The tie rule - the lowest
    cell index first, then the neighbour order - sends every bowl's overflow on to the next one: 1 -> 2 -> 3 -> 1.  Found by a
    random search over small rasters of these four values; the test asserts the ring on the model."""
    M = MISS
    dem = np.array([[12.0, M, M, 10.0],
                    [M, 10.0, M, 11.5],
                    [11.5, 12.0, 11.5, 11.5],
                    [M, 10.0, 10.0, 10.0]])
    return dem, np.where(dem == 10.0, 0.5, 0.0)


def ends():
    """pond 1 spills over a sill into a dry pit - land, basin 0; behind a NODATA cell pond 2 lies alone in its bowl: no outlet"""
    return np.array([[10.0, 12.0, 5.0, MISS, 11.0, 10.0, 11.0]]), np.array([[0.5, 0, 0, 0, 0, 0.5, 0]])


def brim(below_quanta):
    """one bowl of 2 m under a sill at 12 m with land behind it, filled to the sill less `below_quanta` quanta of 2^-24 m"""
    return np.array([[13.0, 10.0, 12.0, 5.0]]), np.array([[0, 2.0 - below_quanta * 2.0 ** -24, 0, 0]])


def bowls(R, Cc, seed, step=0.125, amp=1.0):
    """Hollows half a dozen cells across on a tilted plane, ground in steps of `step` (ties between passes), under a tilted water
    table half a step off those heights - every pond stands below its pass - and 1 m of rain on 3 % of the wet cells, which lifts
    those ponds' highest surface above it: about half the ponds spill, some into each other."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:R, 0:Cc]
    dem = 500.0 + amp * np.sin(x / 3.0) * np.cos(y / 2.5) + 0.01 * x + 0.3 * rng.random((R, Cc))
    dem = np.round(dem / step) * step
    water = np.clip(500.0 - amp * 0.5 + step / 2 + 0.01 * x - dem, 0, None)
    return dem, water + np.where((water > 0) & (rng.random((R, Cc)) < 0.03), 1.0, 0.0)
