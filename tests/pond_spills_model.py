"""Host model of the pond spills (include/wdpm_pond_spills.h) in plain Python - the yardstick of tests/test_pond_spills.py.

Everything is a sequential walk along to_basin with a set or a dictionary of the ponds already seen: a ring is found where a walk
meets its own path again, a chain's answers are taken pond by pond from its end backwards, and the sums go down every chain one pond
after another, the ponds with the most hops first.  Nothing here doubles a pointer, nothing runs in rounds, nothing is pushed
concurrently; the sums are Python integers.  tests/test_pond_spills_model.py holds it against hand-written answers and against
brute_force() below, which walks the whole chain of every pond.

    table, stats = spills(pond_table, rim_table, catch_table, outlet_table, headroom_tol=0.0)
    table, stats = spills_of_water(bd, miss, water, min_depth, headroom_tol)     # through the numpy models of the older units

The four tables are those of the same call (tests/ponds_model.py, pond_rims_model.py, pond_catchments_model.py, pond_outlets_model.py).
"""
import numpy as np

SPILL_DTYPE = np.dtype([("next", "<i4"), ("sink", "<i4"), ("end", "<i4"), ("hops", "<i4"), ("rest", "<i4"), ("rest_hops", "<i4"),
                        ("spilling", "<i4"), ("reserved", "<i4"), ("path_fill_q", "<u8"), ("up_ponds", "<i8"), ("up_cells", "<i8"),
                        ("up_fill_q", "<u8"), ("live_ponds", "<i8"), ("live_cells", "<i8")])
STATS = ("ponds", "rings", "ring_ponds", "spilling", "ends_land", "ends_none", "ends_ring", "max_hops", "rounds")


def rounds_of(n):
    """launches of doubling kernels for n ponds: three passes of ceil(log2 n) + 1"""
    return 3 * ((n - 1).bit_length() + 1) if n > 0 else 0


def spilling_flags(rim_table, outlet_table, headroom_tol):
    with np.errstate(invalid="ignore"):
        headroom = np.asarray(outlet_table["pour_level"], dtype=np.float64) - np.asarray(rim_table["surface_max"], dtype=np.float64)
    return ((outlet_table["to_basin"] >= 0) & (headroom <= np.float64(headroom_tol))).tolist()


def rings_of(to):
    """the rings of the graph k -> to[k - 1] (labels from 1), each as the list of its ponds in walking order"""
    n = len(to)
    done = [False] * (n + 1)
    rings = []
    for start in range(1, n + 1):
        where = {}                                            # pond -> its place on this walk
        path = []
        k = start
        while k > 0 and not done[k] and k not in where:
            where[k] = len(path)
            path.append(k)
            k = to[k - 1]
        if k > 0 and not done[k]:                             # the walk met its own path: a ring from there on
            rings.append(path[where[k]:])
        for p in path:
            done[p] = True
    return rings


def graph(to, spilling, values, fill_q):
    """the rows and the counts from lists: to_basin, the flags, cells + catch_cells and fill_q of ponds 1..n"""
    n = len(to)
    nxt = list(to)
    rings = rings_of(to)
    for ring in rings:
        assert len(ring) >= 2
        nxt[min(ring) - 1] = -2
    # chains: from the end backwards.  A walk stops at a pond whose answers are known, then fills in its path last pond first.
    sink, hops, path_q = [0] * n, [0] * n, [0] * n
    rest, rest_hops = [0] * n, [0] * n
    known = [False] * n
    for start in range(1, n + 1):
        path = []
        k = start
        seen = set()
        while not known[k - 1] and nxt[k - 1] > 0:
            assert k not in seen, "the heads are cut: no walk comes back"
            seen.add(k)
            path.append(k)
            k = nxt[k - 1]
        if not known[k - 1]:                                  # the chain's last pond
            sink[k - 1], hops[k - 1], path_q[k - 1], rest[k - 1], rest_hops[k - 1] = k, 0, fill_q[k - 1], k, 0
            known[k - 1] = True
        for p in reversed(path):
            j = nxt[p - 1]
            sink[p - 1], hops[p - 1], path_q[p - 1] = sink[j - 1], hops[j - 1] + 1, fill_q[p - 1] + path_q[j - 1]
            if spilling[p - 1]:
                rest[p - 1], rest_hops[p - 1] = rest[j - 1], rest_hops[j - 1] + 1
            else:
                rest[p - 1], rest_hops[p - 1] = p, 0
            known[p - 1] = True
    # sums: every pond hands what it has gathered to the next one, the ponds furthest from their sinks first, so that a pond has
    # everything from above before its turn
    up = [[1, values[k], fill_q[k]] for k in range(n)]
    live = [[1, values[k]] for k in range(n)]
    for k in sorted(range(1, n + 1), key=lambda k: -hops[k - 1]):
        j = nxt[k - 1]
        if j > 0:
            for i in range(3):
                up[j - 1][i] += up[k - 1][i]
            if spilling[k - 1]:
                for i in range(2):
                    live[j - 1][i] += live[k - 1][i]
    table = np.zeros(n, dtype=SPILL_DTYPE)
    for k in range(n):
        assert up[k][2] < 2 ** 64 and path_q[k] < 2 ** 64
        table[k] = (nxt[k], sink[k], nxt[sink[k] - 1], hops[k], rest[k], rest_hops[k], int(spilling[k]), 0, path_q[k], up[k][0],
                    up[k][1], up[k][2], live[k][0], live[k][1])
    ends = [nxt[k] for k in range(n) if nxt[k] <= 0]
    stats = {"ponds": n, "rings": len(rings), "ring_ponds": sum(len(r) for r in rings), "spilling": sum(map(int, spilling)),
             "ends_land": ends.count(0), "ends_none": ends.count(-1), "ends_ring": ends.count(-2), "max_hops": max(hops, default=0),
             "rounds": rounds_of(n)}
    return table, stats


def spills(pond_table, rim_table, catch_table, outlet_table, headroom_tol=0.0):
    n = len(outlet_table)
    assert len(pond_table) == len(rim_table) == len(catch_table) == n
    values = (np.asarray(pond_table["cells"], dtype=np.int64) + np.asarray(catch_table["catch_cells"], dtype=np.int64)).tolist()
    return graph(outlet_table["to_basin"].tolist(), spilling_flags(rim_table, outlet_table, headroom_tol), values,
                 [int(q) for q in outlet_table["fill_q"].tolist()])


def spills_of_water(bd, miss, water, min_depth, headroom_tol=0.0):
    """the spill table of a padded DEM and its water, through the numpy models of inventory, rims, catchments and outlets; returns
    (table, stats, tables) with tables = dict(ponds=, rims=, catchments=, outlets=)"""
    from pond_catchments_model import catchments
    from pond_outlets_model import outlets
    from pond_rims_model import device_dem, rims
    from ponds_model import inventory
    labels, ponds = inventory(bd > miss, water, min_depth)
    dem = device_dem(bd, miss)
    rim = rims(labels, dem, water, len(ponds))
    basin, catch, _ = catchments(labels, dem, water, ponds)
    out, _ = outlets(labels, dem, water, ponds, basin=basin)
    table, stats = spills(ponds, rim, catch, out, headroom_tol)
    return table, stats, dict(ponds=ponds, rims=rim, catchments=catch, outlets=out)


def brute_force(to, spilling, values, fill_q):
    """the definitions as they are written, the whole chain of every pond walked on its own: quadratic, for small graphs"""
    n = len(to)
    on_ring = set()
    heads = set()
    for k in range(1, n + 1):
        seen, j = [], to[k - 1]
        while j > 0 and j != k and j not in seen:
            seen.append(j)
            j = to[j - 1]
        if j == k:
            on_ring.add(k)
            if k < min(seen):
                heads.add(k)
    nxt = [-2 if k in heads else to[k - 1] for k in range(1, n + 1)]
    table = np.zeros(n, dtype=SPILL_DTYPE)
    chains = []
    for k in range(1, n + 1):
        chain = [k]
        while nxt[chain[-1] - 1] > 0:
            chain.append(nxt[chain[-1] - 1])
            assert len(chain) <= n
        chains.append(chain)
    for k, chain in enumerate(chains, 1):
        row = table[k - 1]
        row["next"], row["sink"], row["end"], row["hops"] = nxt[k - 1], chain[-1], nxt[chain[-1] - 1], len(chain) - 1
        row["path_fill_q"] = sum(fill_q[p - 1] for p in chain)
        dry = [i for i, p in enumerate(chain) if not spilling[p - 1]]
        row["rest_hops"] = dry[0] if dry else len(chain) - 1
        row["rest"] = chain[row["rest_hops"]]
        row["spilling"] = int(spilling[k - 1])
        above = [c for c in chains if k in c]
        row["up_ponds"], row["up_cells"] = len(above), sum(values[c[0] - 1] for c in above)
        row["up_fill_q"] = sum(fill_q[c[0] - 1] for c in above)
        now = [c for c in above if all(spilling[p - 1] for p in c[:c.index(k)])]
        row["live_ponds"], row["live_cells"] = len(now), sum(values[c[0] - 1] for c in now)
    ends = [v for v in nxt if v <= 0]
    stats = {"ponds": n, "rings": len(heads), "ring_ponds": len(on_ring), "spilling": sum(map(int, spilling)), "ends_land": ends.count(0),
             "ends_none": ends.count(-1), "ends_ring": ends.count(-2), "max_hops": max((len(c) - 1 for c in chains), default=0),
             "rounds": rounds_of(n)}
    return table, stats


def assert_invariants(table, values, fill_q, pour_level=None):
    """what holds of every spill table: `values` is cells + catch_cells and `fill_q` the outlet table's column, per pond"""
    n = len(table)
    values = np.asarray(values, dtype=np.int64)
    fq = [int(q) for q in np.asarray(fill_q).tolist()]
    nxt, sink = table["next"], table["sink"]
    sinks = nxt <= 0
    assert int(table["up_ponds"][sinks].sum()) == n                                  # every pond's chain ends at exactly one sink
    assert int(table["up_cells"][sinks].sum()) == int(values.sum())
    assert (table["live_ponds"] <= table["up_ponds"]).all() and (table["live_cells"] <= table["up_cells"]).all()
    assert (table["live_ponds"] >= 1).all() and (table["live_cells"] >= values).all()
    assert ((table["hops"] == 0) == (sink == np.arange(1, n + 1))).all() and ((table["hops"] == 0) == sinks).all()
    assert (table["reserved"] == 0).all() and np.isin(table["end"], (0, -1, -2)).all() and (nxt >= -2).all() and (nxt <= n).all()
    assert ((table["rest"] == np.arange(1, n + 1)) | (table["spilling"] != 0)).all() and (table["rest_hops"] <= table["hops"]).all()
    on = nxt > 0
    j = nxt[on] - 1
    pq = [int(v) for v in table["path_fill_q"].tolist()]
    for k, jj in zip(np.flatnonzero(on).tolist(), j.tolist()):
        assert pq[k] == fq[k] + pq[jj], (k + 1, jj + 1)
    for k in np.flatnonzero(~on).tolist():
        assert pq[k] == fq[k]
    assert (sink[on] == sink[j]).all() and (table["hops"][on] == table["hops"][j] + 1).all() and (table["end"][on] == table["end"][j]).all()
    fed = np.ones(n, dtype=np.int64)
    np.add.at(fed, j, table["up_ponds"][on])
    assert (fed == table["up_ponds"]).all()                                          # 1 + the sum over the direct feeders
    fed = values.copy()
    np.add.at(fed, j, table["up_cells"][on])
    assert (fed == table["up_cells"]).all()
    if pour_level is not None:                                                       # pour levels never rise along a chain
        pour = np.asarray(pour_level, dtype=np.float64)
        assert (pour[j] <= pour[on]).all()
        heads = np.flatnonzero(nxt == -2)
        assert np.isfinite(pour[heads]).all()


def wave_targets(nxt, spilling, steps=1, wave=64):
    """What the lanes of every wave of `wave` labels hold as a target once every edge reaches `steps` ponds on (1: the table's own
    next; 2: the links after one doubling round): per wave a pair of histograms {target: lanes}, over the forest - the edges with
    next > 0 - and over the live forest, where a pond keeps its edge only if it is spilling, and a longer edge only if every pond
    it passes is.  A walk pond by pond; what a test claims about a scene's waves is read from here."""
    nxt = [int(v) for v in nxt]
    spilling = [bool(v) for v in spilling]
    waves = []
    for first in range(0, len(nxt), wave):
        forest, live = {}, {}
        for k in range(first, min(first + wave, len(nxt))):
            for hist, alive in ((forest, False), (live, True)):
                j = k + 1
                for _ in range(steps):
                    j = nxt[j - 1] if j > 0 and nxt[j - 1] > 0 and (spilling[j - 1] or not alive) else 0
                if j > 0:
                    hist[j] = hist.get(j, 0) + 1
        waves.append((forest, live))
    return waves


def rounds_run_of(to, spilling):
    """How many doubling rounds of each pass - rings, chains, sums - find something to do on the graph k -> to[k - 1] (the outlet
    table's to_basin, rings not yet cut): plain numpy pointer doubling with the kernels' rule that a round runs while the one
    before it has changed a minimum (rings) or left a link that is not an end (chains, sums), at most ceil(log2 n) + 1 of them.
    The results of a pass lie in buffer (that number & 1).  Never used to compute an expected table."""
    to = np.asarray(to, dtype=np.int64)
    n = len(to)
    if n == 0:
        return (0, 0, 0)
    rounds = rounds_of(n) // 3
    idx = np.arange(n)
    p = np.where(to > 0, to, 0)
    m = np.where(to > 0, to, np.iinfo(np.int64).max)
    ring, work = 0, bool((to > 0).any())
    while ring < rounds and work:
        on = p > 0
        m2 = np.where(on, m[p - 1], m)
        work = bool((m2 < m).any())
        m = np.minimum(m, m2)
        p = np.where(on, p[p - 1], 0)
        ring += 1
    nxt = np.where(m == idx + 1, -2, to)
    link = np.where(nxt > 0, nxt, 0)
    live = np.where(np.asarray(spilling, dtype=bool), link, 0)
    chain = 0
    while chain < rounds and (link > 0).any():
        assert (link[live > 0] > 0).all()                      # a live link has a forest link beside it
        link = np.where(link > 0, link[link - 1], 0)
        live = np.where(live > 0, live[live - 1], 0)
        chain += 1
    assert not (link > 0).any() and not (live > 0).any()       # the heads are cut: every chain has ended
    return (ring, chain, chain)                                # the sums pass doubles the forest's links again


def assert_same_spills(table, stats, ref_table, ref_stats):
    """the whole table and the counts, for equality"""
    assert table.dtype == SPILL_DTYPE and len(table) == len(ref_table), (table.dtype, len(table), len(ref_table))
    for name in SPILL_DTYPE.names:
        same = table[name] == ref_table[name]
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: " \
                           f"{table[name][~same][0]!r} vs {ref_table[name][~same][0]!r}"
    assert {k: stats[k] for k in STATS} == ref_stats, (stats, ref_stats)
