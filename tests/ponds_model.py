"""Host model of the pond inventory (include/wdpm_ponds.h) in plain numpy / Python - the yardstick of tests/test_ponds.py.

An independent algorithm: whole-row runs, a two-pointer sweep over the interval lists of neighbouring rows and a union-find with
path halving on run numbers; numbering and table by sorting and numpy reductions.  Nothing here knows about segments, waves or
masks.

    labels, table = inventory(dem_valid, w, min_depth)

dem_valid, w: padded rasters (rows x ncols+2); dem_valid is True where the device DEM is finite (not NODATA, not border).
"""
import numpy as np

POND_DTYPE = np.dtype([("first_row", "<i4"), ("first_col", "<i4"), ("cells", "<i8"), ("volume_q", "<u8"), ("max_depth", "<f8"),
                       ("row_min", "<i4"), ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4")])


def pond_cells(dem_valid, w, min_depth):
    """dem < +inf && w > min_depth, strict; never on the border (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        wet = np.asarray(dem_valid, dtype=bool) & (np.asarray(w) > min_depth)
    wet[0, :] = wet[-1, :] = False
    wet[:, 0] = wet[:, -1] = False
    return wet


def _runs(wet):
    """row, start and end (exclusive) of the set stretches of every row, in row-major order"""
    d = np.diff(wet.astype(np.int8), axis=1, prepend=0, append=0)
    row, s = np.nonzero(d == 1)
    _, e = np.nonzero(d == -1)          # the k-th end belongs to the k-th start: both come in row-major order
    return row, s, e


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def inventory(dem_valid, w, min_depth):
    w = np.asarray(w, dtype=np.float64)
    wet = pond_cells(dem_valid, w, min_depth)
    rows, ncp = wet.shape
    run_row, run_s, run_e = _runs(wet)
    parent = list(range(len(run_row)))
    first_of = np.searchsorted(run_row, np.arange(rows + 1)).tolist()      # run numbers [first_of[r], first_of[r + 1]) lie in row r
    has = np.diff(first_of) > 0
    s_of, e_of = run_s.tolist(), run_e.tolist()
    for r in (np.flatnonzero(has[1:] & has[:-1]) + 1).tolist():            # rows with runs under a row with runs
        # 8-connectivity: run [a, b) touches a run [c, d) of the row above when c < b + 1 and a < d + 1
        i, lo, j, hi = first_of[r - 1], first_of[r], first_of[r], first_of[r + 1]
        while i < lo and j < hi:
            if s_of[i] <= e_of[j] and s_of[j] <= e_of[i]:
                ra, rb = _find(parent, i), _find(parent, j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e_of[i] < e_of[j]:
                i += 1
            else:
                j += 1
    nruns = len(run_row)
    labels = np.zeros((rows, ncp), dtype=np.int32)
    if nruns == 0:
        return labels, np.zeros(0, dtype=POND_DTYPE)
    # runs are numbered in row-major order and links point to smaller numbers: a root is its pond's first run
    root = np.array([_find(parent, k) for k in range(nruns)], dtype=np.int64)
    is_root = root == np.arange(nruns)
    number = np.cumsum(is_root)         # 1-based pond number at each root
    run_label = number[root].astype(np.int32)
    labels[wet] = np.repeat(run_label, run_e - run_s)        # pond cells and runs are both in row-major order
    n = int(is_root.sum())
    table = np.zeros(n, dtype=POND_DTYPE)
    rr, cc = np.nonzero(labels)
    lab = labels[rr, cc].astype(np.int64) - 1
    first = np.flatnonzero(is_root)
    table["first_row"] = run_row[first]
    table["first_col"] = run_s[first]
    table["cells"] = np.bincount(lab, minlength=n)
    q = np.rint(w[rr, cc] * 16777216.0)          # exact product, round half to even
    vol = np.zeros(n, dtype=np.uint64)
    np.add.at(vol, lab, q.astype(np.uint64))
    table["volume_q"] = vol
    md = np.full(n, -np.inf)
    np.maximum.at(md, lab, w[rr, cc])
    table["max_depth"] = md
    for name, src, op, init in (("row_min", rr, np.minimum, np.iinfo(np.int32).max), ("row_max", rr, np.maximum, -1),
                                ("col_min", cc, np.minimum, np.iinfo(np.int32).max), ("col_max", cc, np.maximum, -1)):
        v = np.full(n, init, dtype=np.int64)
        op.at(v, lab, src)
        table[name] = v
    return labels, table


def assert_same(labels, table, ref_labels, ref_table):
    """whole label raster and whole table, for equality"""
    assert labels.dtype == np.int32 and labels.shape == ref_labels.shape
    bad = np.argwhere(labels != ref_labels)
    assert bad.size == 0, f"{len(bad)} cells labelled differently, first at {bad[0].tolist()}: {labels[tuple(bad[0])]} vs {ref_labels[tuple(bad[0])]}"
    assert len(table) == len(ref_table), f"{len(table)} ponds, the model has {len(ref_table)}"
    for name in POND_DTYPE.names:
        a, b = table[name], ref_table[name]
        same = a.view(np.uint64) == b.view(np.uint64) if name == "max_depth" else a == b
        assert same.all(), f"{name}: {int((~same).sum())} ponds differ, first pond {int(np.flatnonzero(~same)[0]) + 1}: {a[~same][0]} vs {b[~same][0]}"
