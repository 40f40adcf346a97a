"""Patterns and the one check of the pond inventory over row blocks (include/wdpm_group_ponds.h), shared by
tests/test_group_ponds.py (N ranks on one GPU) and tests/test_group_ponds_multi_gpu.py (one rank per GPU).

Every check is equality of the whole label raster and the whole table against tests/ponds_model.inventory on the water the group
itself downloads.  Patterns are placed with rowblock.partition, which names every own_lo and own_hi (padded rows; file row =
padded row - 1)."""
import numpy as np

from helpers import pad
from ponds_model import assert_same, inventory

MISS = -99999.0
WET = 0.001


def flat_dem(R, Cc, nodata=None):
    dem = np.full((R, Cc), 100.0)
    if nodata is not None:
        dem[nodata] = MISS
    return dem


def slabs_of(hip, R, n, every=1):
    from wdpm_amd.rowblock import partition
    return partition(hip, R, n, every)


class GroupCase:
    """One group and one handle for several waters of one shape: upload, label at each threshold, hold against the model."""

    def __init__(self, hip, R, Cc, devices, every=1):
        from wdpm_amd.ponds import GroupPonds
        from wdpm_amd.rowblock import Group
        self.R, self.Cc, self.n = R, Cc, len(devices)
        kw = {} if every is None else dict(exchange_every=every)
        self.grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.ponds = GroupPonds(self.grp)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ponds.close()
        self.grp.close()

    def check(self, water, nodata=None, thresholds=(WET,)):
        """returns the group stats of the first threshold"""
        assert water.shape == (self.R, self.Cc)
        bd, bw = pad(flat_dem(self.R, self.Cc, nodata), water, MISS)
        self.grp.upload(bd, bw)
        first = None
        for md in thresholds:
            first = first or check_handle(self.grp, self.ponds, bd > MISS, md)
        return first


def check_handle(grp, p, dem_valid, md):
    n = p.label(md)
    labels, table, stats = p.labels(), p.table(), p.stats()
    ref_labels, ref_table = inventory(dem_valid, grp.download_water(), md)
    assert n == len(ref_table) == stats["ponds"], (n, len(ref_table), stats)
    assert_same(labels, table, ref_labels, ref_table)
    ranks = [p.rank_stats(i) for i in range(grp.size)]
    assert stats["ranks"] == grp.size and stats["local_ponds"] == sum(r["ponds"] for r in ranks), (stats, ranks)
    assert stats["ponds"] == stats["local_ponds"] - stats["merged"] and stats["merged"] >= 0 and stats["stitch_ms"] >= 0, stats
    assert all(r["passes"] == 0 for r in ranks)
    assert p.guard_bad() == 0
    return stats


# ---- case 1: lines across every boundary -----------------------------------------------------------------------------------
def lines(R, Cc, slabs):
    """a full column, full rows either side of the first boundary, the corner-to-corner staircase; depths vary along them"""
    rng = np.random.default_rng(R + len(slabs))
    w = np.zeros((R, Cc))
    w[:, Cc // 3] = 1
    w[slabs[0].own_hi - 1, :] = 1
    w[slabs[1].own_lo - 1, :] = 1
    cols = [i * (Cc - 1) // max(R - 1, 1) for i in range(R)] + [Cc - 1]
    for i in range(R):
        w[i, cols[i]:cols[i + 1] + 1] = 1
    return w * (0.01 + rng.random((R, Cc)))


def anti_diagonal(R, Cc):
    w = np.zeros((R, Cc))
    for i in range(min(R, Cc)):
        w[i, Cc - 1 - i] = 0.5 + i
    return w


def seam_corner(R, Cc, slabs, direction):
    """two cells that touch only diagonally, across the first row-block boundary AND the seam between padded columns 63 and 64"""
    w = np.zeros((R, Cc))
    hi = slabs[0].own_hi                      # padded row; padded (r, c) is file (r - 1, c - 1)
    a, b = (63, 64) if direction == 0 else (64, 63)
    w[hi - 1, a - 1] = 0.25
    w[hi, b - 1] = 0.75
    return w


# ---- case 2: joined only far below (or far above) ----------------------------------------------------------------------------
def isolated_right(w, c0):
    R, Cc = w.shape
    for c in range(c0, Cc, 2):
        w[::2, c] = 0.125 + c * 2.0 ** -12
    return w


def arms(R, Cc):
    """two arms down the whole raster, joined by a bar in the last file row; isolated cells to their right in every rank"""
    w = np.zeros((R, Cc))
    a, b = 1, max(Cc // 2, 3)
    w[:, a] = 0.5 + np.arange(R) * 1e-3
    w[:, b] = 0.25 + np.arange(R) * 1e-3
    w[R - 1, a:b + 1] = 0.3
    return isolated_right(w, b + 3)


def comb(R, Cc):
    """teeth in every other column of the left half, joined only by the last file row; returns the water and the teeth count"""
    w = np.zeros((R, Cc))
    half = max(Cc // 2, 1)
    w[:, 0:half:2] = 1
    w[R - 1, 0:half] = 1
    w *= 0.002 + np.arange(R * Cc).reshape(R, Cc) * 1e-6
    return isolated_right(w, half + 3), len(range(0, half, 2))


# ---- case 3: in and out of a rank ------------------------------------------------------------------------------------------
def serpentine_transposed(R, Cc):
    w = np.zeros((R, Cc))
    w[:, ::2] = 1
    w[-1, 1::4] = 1
    w[0, 3::4] = 1
    return w * (0.002 + np.arange(R * Cc).reshape(R, Cc) * 1e-5)


# ---- case 4: nothing to join -----------------------------------------------------------------------------------------------
def lattice(R, Cc):
    w = np.zeros((R, Cc))
    w[::2, ::2] = 0.5 + np.arange(((R + 1) // 2) * ((Cc + 1) // 2)).reshape((R + 1) // 2, (Cc + 1) // 2) * 2.0 ** -10
    return w


# ---- case 5: noise ---------------------------------------------------------------------------------------------------------
def noise(R, Cc, density, seed):
    """as tests/test_ponds.py::test_noise: 5 % NODATA with water on it, depths from subnormal to several metres, a few NaN"""
    rng = np.random.default_rng(seed)
    depth = rng.random((R, Cc)) * 0.02
    kind = rng.random((R, Cc))
    depth[kind < 0.10] = 3.0 + 5.0 * rng.random(int((kind < 0.10).sum()))
    depth[kind > 0.95] = 5e-324 * rng.integers(1, 1 << 40, int((kind > 0.95).sum()))
    w = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    w[rng.random((R, Cc)) < 0.002] = np.nan
    return w, rng.random((R, Cc)) < 0.05


# ---- the cases the multi-GPU file repeats ----------------------------------------------------------------------------------
def run_lines(case, slabs):
    R, Cc = case.R, case.Cc
    s = case.check(lines(R, Cc, slabs))
    assert s["stitch_unions"] > 0 and s["merged"] > 0, s
    s = case.check(anti_diagonal(R, Cc))
    assert s["ponds"] == 1 and (s["stitch_unions"] > 0 or Cc < R), s
    if Cc >= 64:
        for direction in (0, 1):
            s = case.check(seam_corner(R, Cc, slabs, direction))
            assert s["ponds"] == 1 and s["local_ponds"] == 2 and s["stitch_unions"] == 1 and s["merged"] == 1, s


def run_joined_far_away(case):
    R, Cc, n = case.R, case.Cc, case.n
    for flip in (False, True):                 # the bar in the last rank, then in rank 0
        w = arms(R, Cc)
        s = case.check(w[::-1].copy() if flip else w)
        assert s["merged"] == 2 * (n - 1) and s["stitch_unions"] == 2 * (n - 1), s
        w, teeth = comb(R, Cc)
        s = case.check(w[::-1].copy() if flip else w)
        assert s["merged"] == (n - 1) * teeth, (s, teeth)
        lab = case.ponds.labels()
        assert lab[R if flip else 1, 1] == 1   # the comb is pond 1 either way: its first cell is the raster's first wet cell


def run_noise(case, densities=(0.30, 0.41, 0.60), thresholds=(WET,)):
    for d in densities:
        w, nodata = noise(case.R, case.Cc, d, int(d * 100) + case.R + case.n)
        s = case.check(w, nodata, thresholds)
        assert s["ponds"] > 10 and s["stitch_unions"] > 0, s
