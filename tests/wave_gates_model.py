"""What tests/test_wave_gates.py is built from: the rasters and trigger positions of its cases, the elevation a missed NODATA gate
would decode (garbage_dem), and a plain numpy model of one iteration whose neighbour step is pluggable - exact, or always clamped.

The two gates (wdpm_march.hip::any_nodata16, wdpm_iteration.h::any_above_3m with wdpm_march.hip::deep_next and wdpm_small.hip's deep_sh)
are wave-uniform: one lane's one register out of the nine a step loads decides for all 64 lanes.  A case therefore puts exactly ONE
trigger cell - a NODATA cell, or a depth of 100 m - into a raster that holds no other, at a chosen row and at a chosen lane and
column slot of the marching strip that touches neither border (strip 1 of a 402-column padded raster: padded columns 171 .. 362).

Nothing here runs the code under test: the model and the oracle say whether the mistake a case guards against WOULD show."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from fused_model import NB, STRIP_IN, strip_geometry  # noqa: E402
from test_iter2_retired_strips import K, consumer_stores, groups, strip_origin  # noqa: E402

MISS = -99999.0
GROUP = 48                                      # wdpm_kernels.h::kDemGroup
GRID_EXP = 4                                    # the rasters live on the 1e-4 grid
K_WELL = 5_000_000                              # 500.0000 m: the dry well of every 48-column group of every row
K_PLATEAU = 5_060_000                           # 506.0000 m ...
K_RELIEF = 5534                                 # ... to 506.5534 m at most
R_MAIN, C_MAIN = 40, 400                        # padded 42 x 402: three strips, strip 1 loads padded columns 171 .. 362
STRIP = 1
GATE_LANES = (0, 1, 2, 3, 7, 31, 32, 56, 61, 62, 63)
SEAM_LANES = (0, 31, 63)
SEAM_ROWS = range(2, 14)
R_SEAM = 16
DEEP = 100.0                                    # the clamp trigger: a flow of 12.5 m where the clamped step gives 1 m
# replays of the sweep: the first depth the gate calls deep, NaN, a negative depth - and 400 m, for the third history bit of deep_next:
# a trigger in a triple's last row pours in pass oi = 2 and the row BELOW it pours on in pass oi = 3, two steps after the trigger was
# loaded; of 100 m that row receives 6.4, 5.6 and 4.9 m, less than the 8 m from which a flow exceeds 1 m - of 400 m four times as much
DEEPER = 400.0
REPLAYS = {"deeper": DEEPER, "just-above-3m": float(np.nextafter(3.0000019073486333, 4)), "nan": float("nan"), "negative": -0.25}


def seam_width():
    """the smallest unpadded width at which the strip that opens the second two-iteration group (wdpm_dispatch.h: kGroupOut; strip
    j = 0 of group 1) loads no border column: its 192 columns end one short of the padded raster's last"""
    ncp = strip_origin(1, 0) + K["StripIn"] + 1
    assert groups(ncp) == 2 and groups(ncp - 1) == 2
    return ncp - 2


C_SEAM = seam_width()                            # 854: group 1's first strip loads padded columns 663 .. 854 of 856


def strip_columns(c0, lanes):
    """the padded columns of the given lanes of the strip that starts at c0: all three slots of each"""
    return [c0 + 3 * lane + j for lane in lanes for j in range(3)]


def main_positions():
    """(padded row, padded column) of the 40 x 400 sweep: every row from 2 to R - 1, the three columns of each gate lane of strip 1"""
    c0 = strip_geometry(C_MAIN + 2)[STRIP][0]
    return [(r, c) for r in range(2, R_MAIN) for c in strip_columns(c0, GATE_LANES)]


def seam_positions():
    return [(r, c) for r in SEAM_ROWS for c in strip_columns(strip_origin(1, 0), SEAM_LANES)]


def stored_columns(ncp, c0):
    """[lo, hi]: the padded columns that the single marching loop's strip starting at c0 stores (fused_model.strip_geometry)"""
    for s0, lo, hi in strip_geometry(ncp):
        if s0 == c0:
            return lo, hi
    raise ValueError(c0)


def gated_store(raster):
    """[lo, hi]: the padded columns stored by the strip whose gate the raster's sweep aims at - "main": strip 1 of the 402-column
    raster (single loop and first two-iteration group alike); "seam": the strip that opens the second two-iteration group"""
    if raster == "main":
        return stored_columns(C_MAIN + 2, strip_geometry(C_MAIN + 2)[STRIP][0])
    return consumer_stores(C_SEAM + 2, 1, 0)


# ---------------------------------------------------------------------------------------------------------------- rasters

def well_columns(C, trigger_columns):
    """one padded column per 48-column group: inside the raster, at least three columns away from every trigger column"""
    t = np.array(sorted(set(trigger_columns)))
    wells = []
    for g in range((C + 2 + GROUP - 1) // GROUP):
        cand = [c for c in range(max(GROUP * g, 1), min(GROUP * g + GROUP, C + 1)) if np.abs(t - c).min() >= 3]
        wells.append(cand[len(cand) // 2])
    return wells


def ground(R, C, seed, wells=()):
    """padded DEM: a plateau of odd codes (no coarser decimal grid, as test_dem16_bases.make_dem) between 506.0000 and 506.5534 m,
    a NODATA border, and in every row one cell of exactly 500.0000 m in each of the padded columns `wells`"""
    rng = np.random.default_rng(seed)
    k = K_PLATEAU + (rng.integers(0, K_RELIEF, (R, C)) | 1)
    bd = np.full((R + 2, C + 2), MISS)
    bd[1:-1, 1:-1] = k / 10.0 ** GRID_EXP
    for c in wells:
        bd[1:-1, c] = K_WELL / 10.0 ** GRID_EXP
    return bd


def nodata_raster(R, C, positions, seed=11):
    """(padded DEM without any trigger, padded water): 0.8 m on the plateau, the wells dry"""
    bd = ground(R, C, seed, well_columns(C, [c for _, c in positions]))
    bw = np.where(bd > 501.0, 0.8, 0.0)
    return bd, bw


def with_nodata(bd, bw, pos):
    """the case: one interior NODATA cell, dry as the reference leaves it"""
    d, w = bd.copy(), bw.copy()
    d[pos] = MISS
    w[pos] = 0.0
    return d, w


def clamp_raster(R, C, seed=12):
    """(padded DEM, padded water): the same ground without wells, every valid cell under 0.02 - 0.1 m of water"""
    bd = ground(R, C, seed)
    rng = np.random.default_rng(seed + 1)
    bw = np.zeros_like(bd)
    bw[1:-1, 1:-1] = np.round(0.02 + 0.08 * rng.random((R, C)), 6)
    return bd, bw


def with_depth(bw, pos, depth):
    w = bw.copy()
    w[pos] = depth
    return w


def group_bases(bd, miss, grid_exp):
    """What wdpm_kernels.hip::dem16_encode_kernel stores as a group's base, as the integer (gb + k0) on the 10^-e grid: the LOWEST
    32-bit code among the valid cells of padded columns 48 g .. 48 g + 47 of the row (the last group ends with the row); the
    32-bit code of a cell is rint(dem * 10^e) - k0 with k0 = rint(the DEM's lowest valid elevation * 10^e)
    (wdpm_dem_codes.hip::encode_dem), so gb + k0 is rint(10^e times the group's lowest valid elevation) whatever k0 is.  A group
    without a valid cell has base 0, that is k0 itself."""
    rows, ncp = bd.shape
    q = np.rint(bd * 10.0 ** grid_exp).astype(np.int64)
    valid = bd > miss
    k0 = q[valid].min()
    ng = (ncp + GROUP - 1) // GROUP
    out = np.empty((rows, ng), np.int64)
    for g in range(ng):
        sl = slice(GROUP * g, min(GROUP * g + GROUP, ncp))
        v = valid[:, sl]
        out[:, g] = np.where(v.any(axis=1), np.where(v, q[:, sl], np.iinfo(np.int64).max).min(axis=1), k0)
    return out


def garbage_dem(bd, miss, grid, pos=None):
    """The padded DEM as the marching loops would see it if the NODATA select were left out where it is needed: the NODATA cell at
    `pos` (every interior NODATA cell if None) holds (base + 65535) / 10^grid, the finite elevation wdpm_stencil.h::dem16_decode_nan<true>
    computes from the NODATA offset 0xFFFF and the base of the cell's group - see group_bases for the encoder's rule."""
    bases = group_bases(bd, miss, grid)
    out = bd.copy()
    if pos is None:
        rr, cc = np.nonzero(bd[1:-1, 1:-1] <= miss)
        cells = list(zip(rr + 1, cc + 1))
    else:
        assert bd[pos] <= miss
        cells = [pos]
    for r, c in cells:
        out[r, c] = (bases[r, c // GROUP] + 65535) / 10.0 ** grid
    return out


# ---------------------------------------------------------------------------------------------------------------- the model

def iterate(bw, bd, miss, step, n=1, outlet=None, totaldrain=0.0):
    """n iterations of the reference's sweep (WDPMCL.c:1076-1122) in numpy: nine colour passes (oi outer, oj inner), in each the
    disjoint 3 x 3 blocks around the centres oi, oi + 3, ... x oj, oj + 3, ... all at once, the eight neighbours in the reference's
    order (fused_model.NB).  `step(dc, wc, dn, wn, gate, nvalid) -> (wc, wn)` is one neighbour step: test_stencil_forms.nz_step (exact),
    test_clamped_step.clamped_step (always clamped), a dict {oi: step} with one of them per row alignment, or their drain forms together with `outlet` = (row, column), padded: the drain
    module's sweep, which skips the outlet as a centre, empties centre and outlet where the outlet is the neighbour (runoffd) and
    clears the outlet's 3 x 3 after the nine passes (drain()).  bw may carry leading batch axes; bd is one padded DEM or a batch like bw.
    Returns the water, or (water, totaldrain) with an outlet; totaldrain then has the batch's shape."""
    w = np.array(bw, dtype=np.float64)
    R, C = bd.shape[-2] - 2, bd.shape[-1] - 2
    valid = bd > miss
    td = np.zeros(w.shape[:-2]) + totaldrain
    at = None if outlet is None else (Ellipsis, outlet[0], outlet[1])
    for _ in range(n):
        for oi in (1, 2, 3):
            for oj in (1, 2, 3):
                cs = (Ellipsis, slice(oi, R + 1, 3), slice(oj, C + 1, 3))
                dc, wc = bd[cs], w[cs].copy()
                gate = (wc > 0.0) & valid[cs]
                if outlet is not None and (outlet[0] - oi) % 3 == 0 and (outlet[1] - oj) % 3 == 0:
                    gate[..., (outlet[0] - oi) // 3, (outlet[1] - oj) // 3] = False
                step_now = step[oi] if isinstance(step, dict) else step
                for di, dj in NB:
                    ns = (Ellipsis, slice(oi + di, R + 1 + di, 3), slice(oj + dj, C + 1 + dj, 3))
                    b = None
                    if outlet is not None:
                        r, c = outlet[0] - di, outlet[1] - dj                 # the centre whose neighbour (di, dj) is the outlet
                        if (r - oi) % 3 == 0 and (c - oj) % 3 == 0 and 1 <= r <= R and 1 <= c <= C:
                            b = (Ellipsis, (r - oi) // 3, (c - oj) // 3)
                            before = w[at].copy(), wc[b].copy()
                    wc, wn = step_now(dc, wc, bd[ns], w[ns], gate, valid[ns])
                    w[ns] = wn
                    if b is not None:                                         # runoffd's outlet branch: no flow, both cells emptied
                        hit = gate[b]
                        td = np.where(hit, (td + before[0]) + before[1], td)
                        w[at] = np.where(hit, 0.0, w[at])
                        wc[b] = np.where(hit, 0.0, wc[b])
                w[cs] = wc
        if outlet is not None:
            s = np.zeros(w.shape[:-2])
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    k = (Ellipsis, outlet[0] + i, outlet[1] + j)
                    s = np.where(valid[k] & (w[k] > 0), s + w[k], s)
                    w[k] = 0.0
            td = td + s
    return w if outlet is None else (w, td)


# ---------------------------------------------------------------------------------------------------------------- what a case plays

THRES = 1e-5
NODATA_STEPS = ("iter1", "iter2", "iter5", "block6")
CLAMP_STEPS = ("iter1", "iter2", "iter4")


def digest(water, *scalars):
    """32 bytes that stand for a raster and the scalars that came with it (max diff, totaldrain), bit for bit"""
    h = hashlib.sha256(np.ascontiguousarray(water, dtype=np.float64).tobytes())
    h.update(np.array(scalars, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def play_nodata(ctx, bw):
    """[(raster, scalars)] after 1, 2 and 5 iterations and after one block of 6 with its max diff, each from the uploaded water"""
    out = []
    for n in (1, 2, 5):
        ctx.upload_water(bw)
        ctx.iterate(n)
        out.append((ctx.download_water(), ()))
    ctx.upload_water(bw)
    md = ctx.run_block(6, THRES)
    out.append((ctx.download_water(), (md,)))
    return out


def play_clamp(ctx, bw, drain):
    """[(raster, scalars)] after 1, 2 and 4 iterations, each from the uploaded water; drain: totaldrain from 0.0 comes with it"""
    out = []
    for n in (1, 2, 4):
        ctx.upload_water(bw)
        if drain:
            ctx.totaldrain = 0.0
        ctx.iterate(n)
        w = ctx.download_water()
        out.append((w, (ctx.totaldrain,) if drain else ()))
    return out


# ---------------------------------------------------------------------------------------------------------------- the funnel

def funnel(bd, bw, pos, p):
    """(padded DEM, padded water) with a funnel around the cell `pos`: a 7 x 7 patch on the 1e-4 grid.  The LOW cell at pos lies
    p["low"] m under the plateau's 506 m and holds p["w_low"] m; beside it, at offset p["hole"], a dry HOLE p["hole_depth"] m further down;
    its other seven neighbours (ring 1: ground 506 + p["g1"], depth p["w1"]) are fed by ring 2 (506 + p["g2"], p["w2"]); ring 3 is a dry
    rim 3.5 m above ring 2's ground, so that ring 2 gives inwards only.  No depth exceeds 3.0 m."""
    d, w = bd.copy(), bw.copy()
    r, c = pos
    q = lambda v: np.rint(v * 1e4) / 1e4
    for i in range(-3, 4):
        for j in range(-3, 4):
            ring = max(abs(i), abs(j))
            if ring == 0:
                g, h = 506.0 - p["low"], p["w_low"]
            elif (i, j) == tuple(p["hole"]):
                g, h = 506.0 - p["low"] - p["hole_depth"], 0.0
            elif ring == 1:
                g, h = 506.0 + p["g1"], p["w1"]
            elif ring == 2:
                g, h = 506.0 + p["g2"], p["w2"]
            else:
                g, h = 506.0 + p["g2"] + 3.5, 0.0
            d[r + i, c + j], w[r + i, c + j] = q(g), h
    assert w.max() <= 3.0
    return d, w


def above_gate(w):
    """the cells any_above_3m calls deep: the high word compared as an integer with 3.0's (negative and NaN count)"""
    return (np.ascontiguousarray(w).view(np.uint64) >> np.uint64(32)) > np.uint64(0x40080000)


FUNNEL_HOLES = [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]


def funnel_candidate(rng):
    """one draw of the search: rings that give inwards only (ring 2's ground above ring 1's highest surface, the low cell's surface under
    ring 1's ground even at 10 m), the hole on any side, depths up to 3.0 m"""
    g1 = float(np.round(rng.uniform(-6, -2), 2))
    return dict(low=float(np.round(rng.uniform(20, 30), 2)), hole_depth=float(np.round(rng.uniform(15, 40), 2)),
                hole=list(FUNNEL_HOLES[rng.integers(0, 8)]), g1=g1, g2=float(np.round(g1 + rng.uniform(4.5, 6), 2)),
                w_low=3.0 if rng.random() < 0.7 else float(np.round(rng.uniform(2.5, 3.0), 2)),
                w1=float(np.round(rng.uniform(1.5, 3.0), 2)), w2=3.0 if rng.random() < 0.5 else float(np.round(rng.uniform(2.4, 3.0), 2)))


def funnel_search(phase, candidates, seed, exact, clamped):
    """Part 4's search, seeded: funnels whose low cell sits at padded (row, column) = phase mod 3 of a flat 15 x 15 raster.  A hit: after
    one exact iteration exactly ONE valid cell is deep for the gate, and "iteration 1 exact, iteration 2 always clamped" differs from
    two exact iterations in a valid cell.  Returns (hits, the deepest the one deep cell stood after iteration 1 among the candidates
    that passed the first condition)."""
    rng = np.random.default_rng(seed)
    bd = np.full((17, 17), MISS)
    bd[1:-1, 1:-1] = 506.3
    bw = np.where(bd > MISS, 0.05, 0.0)
    pos = (6 + phase[0], 6 + phase[1])
    hits, deepest = [], 0.0
    for _ in range(candidates):
        p = funnel_candidate(rng)
        d, w = funnel(bd, bw, pos, p)
        w1 = iterate(w, d, MISS, exact)
        deep = above_gate(w1) & (d > MISS)
        if deep.sum() != 1:
            continue
        deepest = max(deepest, float(w1[deep][0]))
        a, b = iterate(w1, d, MISS, exact), iterate(w1, d, MISS, clamped)
        if ((a.view(np.uint64) != b.view(np.uint64)) & (d > MISS)).any():
            hits.append(p)
    return hits, deepest
