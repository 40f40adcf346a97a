"""TEST INFRASTRUCTURE: the ground and water of tests/test_pond_spills.py and tests/pond_spill_cases.py, as file rasters (dem,
water).  Heights are multiples of 1/8 m, so every level, pass and headroom is exact.  NODATA is MISS.  What each scene must give is
asserted on the model by the test that uses it, before the device is asked."""
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


def comb(up, full, cuts_u=(), cuts_d=(), cascade=True):
    """Seven rows that give a chosen graph.  Row 3 is a row of pits: pit i has its floor of 10 m in column 2 i + 1, between walls of
    12 m.  Rows 2 and 4 are rim rows of 12 m with one cell of 11 m per pit, above it where up[i] and below it otherwise: pit i
    spills over that cell.  Rows 1 and 5 are lake rows, floor 1 m under 1 m of water; rows 0 and 6 are walls of 13 m.  full[i] fills
    pit i to its rim - headroom 0, it spills - otherwise it holds 1/8 m.  A lake row is cut into several lakes in the wall column
    left of every pit listed in cuts_u (row 1) and cuts_d (row 5): the pits from that one on feed the next lake.

    cascade: the cut is a dry sill 1/2 m above the lake on its left, every lake lies 1 m below the one before it, and the last one
    leaves over a sill at the right end into a dry pit - land: pits -> lake -> next lake -> ... -> land, a hub of hubs.
    Otherwise the cut is a NODATA column through the lake's three rows and there is no way out at the right end: every lake's
    lowest pass is the rim of its first pit, a ring of two of which one member is a hub.

    Labels run in row-major order: the upper lakes, the pits by column, the lower lakes - with U upper lakes pit i is pond
    U + 1 + i, lane (U + i) % 64 of wave (U + i) // 64 of the table."""
    up, full = np.asarray(up, dtype=bool), np.asarray(full, dtype=bool)
    n = len(up)
    assert len(full) == n and max(len(cuts_u), len(cuts_d)) <= 6
    cols = 2 * n + 3
    dem = np.full((7, cols), 12.0)
    water = np.zeros((7, cols))
    dem[0] = dem[6] = 13.0
    pits = 2 * np.arange(n) + 1
    dem[3, pits] = 10.0
    water[3, pits] = np.where(full, 1.0, 0.125)
    dem[2, pits[up]] = 11.0
    dem[4, pits[~up]] = 11.0
    for lake, rim_rows, cuts in ((1, (0, 1, 2), cuts_u), (5, (4, 5, 6), cuts_d)):
        edges = [0] + [2 * i for i in sorted(cuts)] + [2 * n]
        for k in range(len(edges) - 1):
            surface = 9.0 - k if cascade else 6.0
            span = slice(edges[k] + (k > 0), edges[k + 1])     # the cut's own column is the sill, or NODATA
            dem[lake, span], water[lake, span] = surface - 1.0, 1.0
            if cascade:
                dem[lake, edges[k + 1]], water[lake, edges[k + 1]] = surface + 0.5, 0.0        # the sill at its right end
            elif k:
                dem[rim_rows, edges[k]] = MISS
                water[rim_rows, edges[k]] = 0.0
        if cascade:
            dem[lake, 2 * n + 1:] = 1.0                        # the dry pit behind the last sill
            water[lake, 2 * n + 1:] = 0.0
        else:
            dem[lake, 2 * n:] = 12.0
            water[lake, 2 * n:] = 0.0
    return dem, water


def pits_by_lane(n_upper, waves, more=""):
    """(up, full) for comb() from one string of 64 letters per wave of the table, lane by lane: u / d for a pit that spills up or
    down, U / D for one filled to its rim.  The first n_upper letters belong to the upper lakes and are skipped; `more` goes on into a
    last, partial wave."""
    letters = "".join(waves)
    assert all(len(w) == 64 for w in waves) and set(letters + more) <= set("udUD")
    letters = (letters + more)[n_upper:]
    return np.array([c in "uU" for c in letters]), np.array([c in "UD" for c in letters])


def spread(lanes, letter, other="d", others_full=lambda lane: lane % 3 == 0):
    """one wave for pits_by_lane: `letter` in the lanes listed; elsewhere `other`, as a capital where others_full(lane)"""
    return "".join(letter if k in lanes else other.upper() if others_full(k) else other for k in range(64))


# the lanes that share the minority target: both halves of the wave, lanes 0 and 63 among them
SHARERS = {7: (0, 5, 17, 31, 32, 46, 63), 8: (0, 5, 17, 31, 32, 40, 46, 63), 9: (0, 5, 17, 22, 31, 32, 40, 46, 63)}
FILLER = "dD" * 32


def vote_boundary():
    """Two upper lakes, cut inside wave 0, and one lower lake.  Waves 1, 2 and 3: exactly 7, 8 and 9 full pits in SHARERS' lanes
    spill up into lake 2, the other 57, 56 and 55 down into the lower lake - lane 0 holds the small group, so its vote comes first.
    Waves 4 and 5: the groups of 7 and 8 moved on by one lane (lanes 1..), so that lane 0 holds the big group and the small one is
    put to the vote second."""
    first = [spread(SHARERS[k], "U") for k in (7, 8, 9)]
    second = [spread([(lane + 1) % 64 for lane in SHARERS[k] if lane != 63] + [62], "U") for k in (7, 8)]
    up, full = pits_by_lane(2, [FILLER] + first + second)
    return comb(up, full, cuts_u=(10,))


def live_is_not_forest():
    """as vote_boundary's first waves, with 12 lanes that spill up into lake 2 in waves 1 and 2: 7 of them full in wave 1, 8 in
    wave 2 - the forest's vote succeeds in both, the live forest's only in the second.  Waves 3 and 4: the same with the 12 lanes
    moved on by one (63 to 62), so that lane 0 holds the other target."""
    twelve = SHARERS[9] + (11, 52, 58)
    def wave(n_full, shift):
        lanes = [lane + shift if lane + shift < 64 else 62 for lane in twelve]
        return "".join(("U" if lanes.index(k) < n_full else "u") if k in lanes else "D" if k % 3 == 0 else "d" for k in range(64))
    up, full = pits_by_lane(2, [FILLER, wave(7, 0), wave(8, 0), wave(7, 1), wave(8, 1)])
    return comb(up, full, cuts_u=(10,))


def four_hubs():
    """two upper and two lower lakes, all four cut at the pit in lane 32 of wave 1: the even lanes of that wave spill up, the odd
    ones down - four targets of 16 lanes each for three votes.  Wave 2 the same with the lanes' roles exchanged and every third
    pit not full."""
    wave1 = "UD" * 32
    wave2 = "".join(("d" if k % 2 == 0 else "u").upper() if k % 3 else ("d" if k % 2 == 0 else "u") for k in range(64))
    up, full = pits_by_lane(2, [FILLER, wave1, wave2, FILLER])
    return comb(up, full, cuts_u=(64 + 32 - 2,), cuts_d=(64 + 32 - 2,))


def failed_votes():
    """Three upper lakes and one lower.  Wave 1: lanes 0..13 spill up into lake 1 and down in turn, 7 each, lanes 14..63 up into
    lake 2 - two votes fail (three: the first target is asked again), nobody goes together.  Wave 2 is the mirror: lanes 0..49 up
    into lake 2, then 7 and 7 into lake 3 and down.  All full, so the live forest votes the same way."""
    wave1 = "UD" * 7 + "U" * 50
    wave2 = "U" * 50 + "UD" * 7
    up, full = pits_by_lane(3, ["D" * 64, wave1, wave2], more="dDd")
    return comb(up, full, cuts_u=(64 + 14 - 3, 128 + 50 - 3))


def lane_0_on_land():
    """one upper lake, pond 1, in lane 0 of wave 0: it leaves onto land and has no target, eight pits of its own wave spill into it"""
    up, full = pits_by_lane(1, [spread(SHARERS[9], "U")], more="dDuU")
    return comb(up, full)


def ring_through_a_hub():
    """cascade=False with one lake either side: each lake's lowest pass is the rim of its first pit, a ring of two.  The upper lake
    is pond 1 and the head; its first pit, in lane 5, carries the mark and is one of eight lanes of wave 0 that share the lake.
    Below, the first pit (lane 1) is the head and the lake, the last label, carries the mark."""
    up, full = pits_by_lane(1, [spread(SHARERS[9], "u", others_full=lambda lane: lane % 2 == 0), FILLER], more="dDuUd")
    return comb(up, full, cascade=False)


def cascade():
    """three upper lakes in a chain, fed by 70 pits each, and one lower lake fed by 25: after one doubling the pits of lakes 1 and
    2 hold lakes 2 and 3 as their targets, 64 lanes to a wave"""
    n = 235
    i = np.arange(n)
    up = i < 210
    return comb(up, i % 3 != 1, cuts_u=(70, 140))


def hub_last(ponds):
    """one upper lake, ponds - 2 pits of which all but nine spill down, and the lower lake as the last label"""
    n = ponds - 2
    i = np.arange(n)
    return comb(np.isin(i, (0, 7, 60, 61, 62, 63, 64, 130, n - 1)), i % 2 == 0)


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
