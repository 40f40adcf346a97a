"""Row-block decomposition (wdpm_amd/rowblock.py) on CPU ranks: world size 2 and 3 over gloo with the
oracle back-end must reproduce the single-slab result bit for bit, for several exchange intervals;
and the halo-depth rule itself is checked to be tight."""
import json
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ORACLE_SO, ROOT
from helpers import bits_equal, find_drain, n_bit_diff, pad, random_case
from wdpm_amd.rowblock import Group, RowBlockSolver, halo_depth, partition


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(world, case, libpath=ORACLE_SO, env=None):
    port = free_port()
    with tempfile.TemporaryDirectory() as td:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rowblock_worker.py"), str(r),
                                   str(world), str(port), libpath, json.dumps(case), td], env=env)
                 for r in range(world)]
        rcs = [p.wait(timeout=600) for p in procs]
        assert rcs == [0] * world, rcs
        return [dict(np.load(os.path.join(td, f"rank{r}.npz"))) for r in range(world)]


def single(oracle, case):
    dem, water, miss = random_case(case["seed"], case["R"], case["C"])
    if case.get("ponds"):
        water[:, :] = 0.0
        for r0, r1, c0, c1, d in case["ponds"]:
            water[r0:r1, c0:c1] = d
        water[dem <= miss] = 0.0
    bd, bw = pad(dem, water, miss)
    kw = {}
    if case["module"] == "drain":
        dr, dc = find_drain(bd)
        kw = dict(drainrow=dr, draincol=dc)
    s = RowBlockSolver(oracle, case["module"], case["R"], case["C"], miss, **kw)
    s.upload_global(bd, bw)
    if kw:
        s.set_totaldrain(max(bw[dr, dc], 0.0))
    mds, stats = [], []
    for n in case["blocks"]:
        mds.append(s.run_block(n, case["thres"]))
        if kw:
            stats.append(list(s.drain_stats()) + [s.totaldrain()])
    w = s.ctx.download_water()
    s.close()
    case["_stats"] = stats
    return w, mds


def test_partition_properties(oracle):
    for nrows, n, k in [(16384, 8, 4), (16384, 8, 1), (16384, 2, 10), (482, 3, 2), (8192, 4, 16), (100, 2, 1)]:
        slabs = partition(oracle, nrows, n, k)
        up, down = halo_depth(k)
        assert slabs[0].own_lo == 0 and slabs[-1].own_hi == nrows + 1
        for a, b in zip(slabs, slabs[1:]):
            assert b.own_lo == a.own_hi + 1
            assert b.own_lo % 3 == 2
        for s in slabs:
            assert s.row0 % 3 == 0
            assert s.row0 + s.rows <= nrows + 2
            if s.rank > 0:
                assert s.up == up
            if s.rank < n - 1:
                assert s.down == min(down, nrows + 1 - s.own_hi)
    with pytest.raises(ValueError):
        partition(oracle, 60, 4, 8)


def test_partition_keeps_the_outlet_inside_its_owner(oracle):
    """drain: totaldrain is summed from rows dr-1 .. dr+1, which must be OWNED rows of the rank that
    reports it (a halo row is stale by the k-th iteration after a refresh): every boundary stays
    at least three rows away from the outlet's row, and stays = 2 (mod 3)"""
    for nrows, n, k in [(150, 2, 1), (150, 2, 3), (400, 3, 2), (8192, 8, 4)]:
        plain = partition(oracle, nrows, n, k)
        for b in [s.own_lo for s in plain[1:]]:
            for dr in range(max(1, b - 5), min(nrows, b + 5) + 1):
                slabs = partition(oracle, nrows, n, k, "drain", dr)
                owner = [s for s in slabs if s.own_lo <= dr <= s.own_hi]
                assert len(owner) == 1
                o = owner[0]
                assert (o.rank == 0 or dr - o.own_lo >= 3) and (o.rank == n - 1 or o.own_hi - dr >= 3), (nrows, n, k, dr, o)
                for a, c in zip(slabs, slabs[1:]):
                    assert c.own_lo == a.own_hi + 1 and c.own_lo % 3 == 2 and c.row0 % 3 == 0


@pytest.mark.parametrize("world,k", [(2, 1), (2, 4), (3, 2)])
def test_multirank_equals_single_slab(oracle, world, k):
    case = dict(seed=11, R=150 if world == 2 else 200, C=61, module="add", k=k, thres=0.005 / 1000, blocks=[13, 8])
    want, mds = single(oracle, case)
    got = run_ranks(world, case)
    for g in got:
        lo, hi = int(g["lo"]), int(g["hi"])
        assert bits_equal(g["own"], want[lo:hi + 1]), f"rows {lo}..{hi}: {n_bit_diff(g['own'], want[lo:hi + 1])} cells differ"
        assert list(g["mds"]) == mds


@pytest.mark.parametrize("module", ["add", "drain"])
def test_eight_rank_processes_over_gloo(oracle, module):
    """N = 8 as rank PROCESSES (so far eight slabs had only run as threads of one process, and as rank processes two to
    four): the driver's partition into eight row blocks, its chain of refreshes at the default interval k = 8 with the deep
    halos that go with it (23 rows above, 46 below), the eight-way all-gather of the block scalars and, for drain, the
    rank-chained volume sum - one process per rank over gloo, here on the CPU where eight processes are allowed (the GPU
    pool's process guard stops at six on a card; four rank processes run there at 16384^2, tests/test_mock_rccl.py)."""
    case = dict(seed=23, R=960, C=45, module=module, k=8, thres=0.005 / 1000, blocks=[19, 9])
    want, mds = single(oracle, case)
    stats = case.pop("_stats")
    got = run_ranks(8, case)
    assert [int(g["lo"]) for g in got] == sorted(int(g["lo"]) for g in got) and int(got[-1]["hi"]) == case["R"] + 1
    for g in got:
        lo, hi = int(g["lo"]), int(g["hi"])
        assert bits_equal(g["own"], want[lo:hi + 1]), f"rows {lo}..{hi}: {n_bit_diff(g['own'], want[lo:hi + 1])} cells differ"
        assert list(g["mds"]) == mds
        if module == "drain":
            assert g["stats"].tolist() == stats


@pytest.mark.parametrize("world,k,R", [(2, 2, 150), (3, 1, 210)])
def test_multirank_drain_equals_single_slab(oracle, world, k, R):
    """drain module across ranks: water, max diff, totaldrain, |d totaldrain| and the chained
    row-major volume sum all equal the single-slab values bit for bit"""
    case = dict(seed=17, R=R, C=61, module="drain", k=k, thres=0.005 / 1000, blocks=[9, 6])
    want, mds = single(oracle, case)
    stats = case.pop("_stats")
    got = run_ranks(world, case)
    for g in got:
        lo, hi = int(g["lo"]), int(g["hi"])
        assert bits_equal(g["own"], want[lo:hi + 1])
        assert list(g["mds"]) == mds
        assert g["stats"].tolist() == stats
    assert stats[0][2] > 0      # something was drained, so the test is not vacuous


NB = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def taint(rows, cols, k, bad):
    """Cell-level worst-case dependency simulation of k iterations in the reference's pass order:
    bad[r,c] True = the cell may differ from the full-raster computation.  Within a block the centre
    depends on everything; neighbour i on itself, the centre and the neighbours visited before it."""
    t = bad.copy()
    for _ in range(k):
        for oi in (1, 2, 3):
            for oj in (1, 2, 3):
                R, C = np.meshgrid(np.arange(oi, rows - 1, 3), np.arange(oj, cols - 1, 3), indexing="ij")
                acc = t[R, C].copy()
                for di, dj in NB:
                    tn = t[R + di, C + dj]
                    t[R + di, C + dj] = tn | acc
                    acc = acc | tn
                t[R, C] = acc
    return t


def test_a_refused_transport_surfaces_on_every_rank(oracle):
    """the caller's host transport failing (every rank sees the refusal at the first exchange) comes back
    through the C driver as the caller's own exception - no hang, no silent continuation on stale halos"""
    case = dict(seed=23, R=150, C=70, module="add", k=2, thres=0.005 / 1000, blocks=[7], failing_transport=True)
    parts = run_ranks(2, case)
    assert all(int(p["refused"]) == 1 for p in parts)


def group_run(lib, case, devices, dr=None, dc=None):
    """the ranks of ONE process (wdpm_group_*: one host thread per slab) on `devices`"""
    dem, water, miss = random_case(case["seed"], case["R"], case["C"], **case.get("gen", {}))
    bd, bw = pad(dem, water, miss)
    kw = {}
    if case["module"] == "drain":
        if dr is None:
            dr, dc = find_drain(bd)
        kw = dict(drainrow=dr, draincol=dc)
    with Group(lib, case["module"], case["R"], case["C"], miss, devices, exchange_every=case["k"], **kw) as g:
        g.upload(bd, bw)
        if kw:
            g.set_totaldrain(max(bw[dr, dc], 0.0))
        mds, stats = [], []
        for n in case["blocks"]:
            mds.append(g.run_block(n, case["thres"]))
            if kw:
                stats.append(list(g.drain_stats()) + [g.totaldrain()])
        return g.download_water(), mds, stats, g.size


@pytest.mark.parametrize("n,k", [(2, 1), (3, 2), (4, 1)])
def test_thread_per_rank_group_equals_single_context(oracle, n, k):
    """wdpm_group: the same C ranks driven by one host thread each inside one process"""
    case = dict(seed=31, R=260, C=50, module="add", k=k, thres=0.005 / 1000, blocks=[11, 6])
    want, mds, _, _ = group_run(oracle, case, [0])
    got, mds_n, _, size = group_run(oracle, case, [0] * n)
    assert size == n and bits_equal(got, want) and mds_n == mds


@pytest.mark.parametrize("where", ["own_lo", "own_lo+1", "own_hi-1", "own_hi", "own_lo-1"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_drain_outlet_next_to_a_slab_boundary(oracle, where, k):
    """with the outlet on the first owned row of a slab, row dr-1 was a halo row and totaldrain
    went wrong by the k-th iteration after a refresh.  The outlet is forced onto the rows around the
    boundary an outlet-blind partition would choose; water, totaldrain, |d totaldrain| and the volume sum
    must all equal the single-context values"""
    R, C = 150, 40
    case = dict(seed=41, R=R, C=C, module="drain", k=k, thres=0.005 / 1000, blocks=[3 * k + 1, 2 * k],
                gen=dict(missing_frac=0.0, dry_frac=0.1))
    plain = partition(oracle, R, 2, k)
    b = plain[1].own_lo
    dr = {"own_lo": b, "own_lo+1": b + 1, "own_hi-1": b - 2, "own_hi": b - 1, "own_lo-1": b - 1}[where]
    dc = 17
    want, mds, stats, _ = group_run(oracle, case, [0], dr, dc)
    got, mds2, stats2, size = group_run(oracle, case, [0, 0], dr, dc)
    assert size == 2
    assert bits_equal(got, want) and mds2 == mds
    assert stats2 == stats, (stats2, stats)
    assert stats[0][2] > 0


def test_halo_depth_equals_worst_case_dependency_reach():
    """3k-1 rows above / 6k-2 below (slab boundaries = 2 mod 3, first slab row = 0 mod 3), and the
    fused kernel's per-iteration trapezoid: 8 columns left / 12 right, 2 rows up / 4 down"""
    n = 420
    for k in (1, 2, 3, 5, 8):
        up, down = halo_depth(k)
        bad = np.zeros((n, n), bool)
        S, E = 99, 302                       # first / last row held: S % 3 == 0, E % 3 == 2
        bad[:S] = True
        bad[E + 1:] = True
        t = taint(n, n, k, bad)[:, 100:-100]
        clean = np.nonzero(~t.any(axis=1))[0]
        assert clean.min() == S + up and clean.max() == E - down, (k, clean.min() - S, E - clean.max())
    # columns, one iteration, strip starting at a multiple of 3 (wdpm_dispatch.h: kHaloL / kHaloR)
    bad = np.zeros((n, n), bool)
    c0, c1 = 99, 99 + 191
    bad[:, :c0] = True
    bad[:, c1 + 1:] = True
    t = taint(n, n, 1, bad)[100:-100]
    clean = np.nonzero(~t.any(axis=0))[0]
    from fused_model import HALO_L, HALO_R
    assert clean.min() - c0 == 8 == HALO_L and c1 - clean.max() == 12 <= HALO_R   # 13: strip pitch must be 0 mod 3
    # rows of one marching chunk: loads [A, B] with A % 3 == 0, B % 3 == 2 -> exact [A+2, B-4]
    bad = np.zeros((n, n), bool)
    A, B = 99, 302
    bad[:A] = True
    bad[B + 1:] = True
    t = taint(n, n, 1, bad)[:, 100:-100]
    clean = np.nonzero(~t.any(axis=1))[0]
    assert clean.min() == A + 2 and clean.max() == B - 4


@pytest.mark.parametrize("k", [1, 2, 4])
def test_halo_depth_is_sufficient(oracle, k):
    """k iterations on a slab with halos (3k-1 up, 6k-2 down) leave the owned rows exact; the halo
    of k-1 iterations above does not (the downward worst case needs data that moves water along
    every dependency, so a random raster usually gets away with less below)"""
    R, C = 150, 40
    dem, water, miss = random_case(5, R, C, missing_frac=0.0, dry_frac=0.0)
    bd, bw = pad(dem, water, miss)
    with oracle.context(module="add", nrows=R, ncols=C, missingvalue=miss) as full:
        full.upload(bd, bw)
        full.iterate(k)
        want = full.download_water()
    up, down = halo_depth(k)
    lo, hi = 59, 94                       # owned rows, lo % 3 == 2, hi % 3 == 1

    def owned_after(u, d):
        r0, r1 = lo - u, hi + d
        assert r0 % 3 == 0
        with oracle.context(module="add", nrows=R, ncols=C, missingvalue=miss, slab_row0=r0,
                            slab_rows=r1 - r0 + 1) as c:
            c.upload(bd[r0:r1 + 1], bw[r0:r1 + 1])
            c.iterate(k)
            return c.download_rows(lo - r0, hi - lo + 1)
    assert bits_equal(owned_after(up, down), want[lo:hi + 1])
    if up >= 3:
        assert not bits_equal(owned_after(up - 3, down), want[lo:hi + 1])
    assert not bits_equal(owned_after(up, 0), want[lo:hi + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("world,k", [(2, 1), (3, 3)])
def test_multirank_hip_slabs_over_gloo(oracle, hip, world, k):
    """the same decomposition with the HIP back-end: ranks are processes sharing the box's one GPU,
    halos staged through host memory over gloo (the RCCL transport needs one GPU per rank)."""
    case = dict(seed=12, R=260, C=400, module="add", k=k, thres=0.005 / 1000, blocks=[14, 9],
                ctx_kw=dict(device=0))
    want, mds = single(oracle, case)
    got = run_ranks(world, case, libpath=hip.path)
    for g in got:
        lo, hi = int(g["lo"]), int(g["hi"])
        assert bits_equal(g["own"], want[lo:hi + 1]), f"rows {lo}..{hi}: {n_bit_diff(g['own'], want[lo:hi + 1])} cells differ"
        assert list(g["mds"]) == mds


@pytest.mark.gpu
def test_multirank_hip_drain_over_gloo(oracle, hip):
    case = dict(seed=18, R=240, C=380, module="drain", k=2, thres=0.005 / 1000, blocks=[9, 6], ctx_kw=dict(device=0))
    want, mds = single(oracle, dict(case, ctx_kw={}))
    ref = dict(case, ctx_kw={})
    single(oracle, ref)
    stats = ref["_stats"]
    got = run_ranks(2, case, libpath=hip.path)
    for g in got:
        lo, hi = int(g["lo"]), int(g["hi"])
        assert bits_equal(g["own"], want[lo:hi + 1])
        assert list(g["mds"]) == mds
        assert g["stats"].tolist() == stats


@pytest.mark.gpu
@pytest.mark.parametrize("module,n,k", [("add", 3, 3), ("add", 4, 1), ("drain", 2, 2), ("drain", 3, 1)])
def test_hip_group_threads_equal_single_context(oracle, hip, module, n, k):
    """wdpm_group on the HIP back-end: n slabs of one GPU, one host thread each, peer-copy halos chained by
    stream events, the overlapped last iteration before every refresh - against the oracle on one slab"""
    case = dict(seed=33, R=300, C=420, module=module, k=k, thres=0.005 / 1000, blocks=[13, 8])
    want, mds, stats, _ = group_run(oracle, case, [0])
    got, mds_n, stats_n, size = group_run(hip, case, [0] * n)
    assert size == n and bits_equal(got, want), n_bit_diff(got, want)
    assert mds_n == mds and stats_n == stats


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["own_lo", "own_hi"])
def test_hip_drain_outlet_next_to_a_slab_boundary(oracle, hip, where):
    R, C, k = 240, 300, 2
    case = dict(seed=43, R=R, C=C, module="drain", k=k, thres=0.005 / 1000, blocks=[7, 4],
                gen=dict(missing_frac=0.0, dry_frac=0.1))
    b = partition(oracle, R, 2, k)[1].own_lo
    dr, dc = (b if where == "own_lo" else b - 1), 100
    want, mds, stats, _ = group_run(oracle, case, [0], dr, dc)
    got, mds2, stats2, _ = group_run(hip, case, [0, 0], dr, dc)
    assert bits_equal(got, want) and mds2 == mds and stats2 == stats


def test_driver_error_paths_report_instead_of_crashing(oracle):
    """bad arguments to the multi-rank entry points come back as errors with a message (wdpm_last_error)"""
    import ctypes as C
    from wdpm_amd.capi import Params, SlabStruct, WdpmError
    dll = oracle.dll
    p = Params(module=0, nrows=60, ncols=30, drainrow=0, draincol=0, slab_row0=0, slab_rows=0, device=0, kernel=0,
               chunk_rows=0, missingvalue=-99999.0)
    h = C.c_void_p()
    # more ranks than the raster has room for, a rank outside the world, RCCL without an id, host halos without a transport
    assert dll.wdpm_rank_create(C.byref(h), C.byref(p), 0, 40, 1, 0, None, None) != 0 and b"too short" in dll.wdpm_last_error()
    assert dll.wdpm_rank_create(C.byref(h), C.byref(p), 5, 2, 1, 0, None, None) != 0
    assert dll.wdpm_rank_create(C.byref(h), C.byref(p), 0, 2, 1, 1, None, None) != 0 and b"RCCL" in dll.wdpm_last_error()
    assert dll.wdpm_rank_create(C.byref(h), C.byref(p), 0, 2, 1, 3, None, None) != 0 and b"transport" in dll.wdpm_last_error()
    assert dll.wdpm_partition(60, 4, 8, 0, -1, (SlabStruct * 4)()) != 0
    # a group shrinks instead: first the exchange interval (60 rows serve k = 1 on 4 ranks), then the rank count
    with Group(oracle, "add", 60, 30, -99999.0, [0, 0, 0, 0], exchange_every=8) as g:
        assert g.size == 4
    with Group(oracle, "add", 20, 30, -99999.0, [0] * 8, exchange_every=2) as g:
        assert 1 <= g.size < 8
    with Group(oracle, "add", 60, 30, -99999.0, [0, 0], exchange_every=1) as g:
        with pytest.raises(WdpmError):
            oracle.check(dll.wdpm_group_set_drain(g._h, 5, 5))      # not a drain group
        with pytest.raises(WdpmError):
            oracle.check(dll.wdpm_group_upload_unpadded(g._h, None, None, None))


def _random_group_jobs(lib, ref_lib, seeds):
    """random rasters (3 .. 160 rows), 2 .. 7 slabs on one device, exchange every 1 .. 6 iterations, any module, the drain
    outlet anywhere, blocks of 1 .. 9 iterations with and without a flush threshold: the group's max change, rasters,
    totaldrain and drain statistics against ONE context of `ref_lib` (the oracle)"""
    import random
    for seed in seeds:
        rng = random.Random(seed)
        R, C = rng.randint(3, 160), rng.randint(1, 60)
        n, k = rng.randint(2, 7), rng.randint(1, 6)
        module = rng.choice(["add", "drain", "subtract"])
        dem, water, miss = random_case(seed, R, C, missing_frac=rng.choice([0, 0.05, 0.3]))
        bd, bw = pad(dem, water, miss)
        kw = {}
        if module == "drain":
            dr, dc = find_drain(bd)
            valid = np.argwhere(bd > miss)
            if rng.random() < 0.5 and len(valid):
                dr, dc = map(int, valid[rng.randrange(len(valid))])
            kw = dict(drainrow=dr, draincol=dc)
        iters = [rng.randint(1, 9) for _ in range(3)]
        thres = rng.choice([0.0, 1e-5])
        with ref_lib.context(module=module, nrows=R, ncols=C, missingvalue=miss, **kw) as c:
            c.upload(bd, bw)
            if module == "drain":
                c.totaldrain = max(float(bw[dr, dc]), 0.0)
            want = ([c.run_block(i, thres) for i in iters], c.totaldrain, c.drain_stats() if module == "drain" else None)
            w1 = c.download_water()
        with Group(lib, module, R, C, miss, [0] * n, exchange_every=k, **kw) as g:
            g.upload(bd, bw)
            if module == "drain":
                g.set_totaldrain(max(float(bw[dr, dc]), 0.0))
            got = ([g.run_block(i, thres) for i in iters], g.totaldrain() if module == "drain" else want[1],
                   g.drain_stats() if module == "drain" else None)
            assert got == want, (seed, R, C, n, k, module, kw, g.size)
            assert n_bit_diff(g.download_water(), w1) == 0, (seed, R, C, n, k, module, kw, g.size)


def test_random_group_jobs_equal_one_context(oracle):
    _random_group_jobs(oracle, oracle, range(0, 150))


@pytest.mark.gpu
def test_hip_random_group_jobs_equal_the_oracle(oracle, hip):
    lo, hi = (int(v) for v in os.environ.get("WDPM_FUZZ_SEEDS", "2000:2080").split(":"))       # a longer hunt: WDPM_FUZZ_SEEDS=lo:hi
    _random_group_jobs(hip, oracle, range(lo, hi))


def test_partition_properties_on_random_inputs(oracle):
    """wdpm_partition on 3000 random (rows, ranks, exchange interval, module, outlet row): whenever it accepts, the slabs tile
    the padded rows, every boundary is = 2 (mod 3), every slab starts on a multiple of 3 and lies inside the raster, interior
    halos have the full depth, and a drain outlet is at least three owned rows away from its owner's boundaries"""
    import random
    rng = random.Random(7)
    accepted = 0
    for _ in range(3000):
        nrows = rng.choice([rng.randint(1, 60), rng.randint(60, 3000), rng.randint(3000, 70000)])
        n, k = rng.randint(1, 16), rng.randint(1, 12)
        module = rng.choice(["add", "drain"])
        dr = rng.randint(1, nrows) if module == "drain" else -1
        try:
            slabs = partition(oracle, nrows, n, k, module, dr)
        except ValueError:
            continue
        accepted += 1
        up, down = halo_depth(k)
        assert len(slabs) == n and slabs[0].own_lo == 0 and slabs[-1].own_hi == nrows + 1
        for a, b in zip(slabs, slabs[1:]):
            assert b.own_lo == a.own_hi + 1 and b.own_lo % 3 == 2, (nrows, n, k, module, dr)
        for s in slabs:
            assert s.own_lo <= s.own_hi and s.row0 % 3 == 0 and s.row0 >= 0 and s.row0 + s.rows <= nrows + 2
            assert s.row0 <= s.own_lo - (s.up if s.rank > 0 else 0) and s.row0 + s.rows - 1 >= s.own_hi + (s.down if s.rank < n - 1 else 0)
            if s.rank > 0:
                assert s.up == up
            if s.rank < n - 1:
                assert s.down == min(down, nrows + 1 - s.own_hi)
            if module == "drain" and s.own_lo <= dr <= s.own_hi and n > 1:
                assert (s.rank == 0 or dr - s.own_lo >= 3) and (s.rank == n - 1 or s.own_hi - dr >= 3), (nrows, n, k, dr, s)
    assert accepted > 1000


def _outlet_on_a_slab_edge_cases(lib):
    """(R, n, k, dr) with the outlet's row = the last (or first) row of a slab that does not own it: there the slab's kernels
    cannot apply drain() to their copy of the outlet's 3x3 (it is cut by the slab edge), so the rows must ARRIVE drained"""
    cases = []
    for R, n, k in [(14, 2, 1), (40, 2, 2), (60, 3, 2), (90, 3, 3), (33, 2, 1), (120, 4, 2)]:
        for dr in range(1, R + 1):
            try:
                slabs = partition(lib, R, n, k, "drain", dr)
            except ValueError:
                continue
            for s in slabs:
                owns = s.own_lo <= dr <= s.own_hi
                if not owns and dr in (s.row0, s.row0 + s.rows - 1):
                    cases.append((R, n, k, dr))
    return cases


def _check_outlet_on_slab_edges(lib, oracle):
    cases = _outlet_on_a_slab_edge_cases(oracle)
    assert len(cases) >= 8
    for R, n, k, dr in cases:
        C = 53
        dem, water, miss = random_case(R * 100 + dr, R, C, missing_frac=0.0)
        bd, bw = pad(dem, water, miss)
        for dc in (1, 27, C):
            kw = dict(drainrow=dr, draincol=dc)
            with oracle.context(module="drain", nrows=R, ncols=C, missingvalue=miss, **kw) as c:
                c.upload(bd, bw)
                c.totaldrain = 0.1
                want = [c.run_block(i, 1e-5) for i in (4, 9)]
                w1, td1 = c.download_water(), c.totaldrain
            with Group(lib, "drain", R, C, miss, [0] * n, exchange_every=k, **kw) as g:
                g.upload(bd, bw)
                g.set_totaldrain(0.1)
                got = [g.run_block(i, 1e-5) for i in (4, 9)]
                assert got == want and g.totaldrain() == td1, (R, n, k, dr, dc)
                assert n_bit_diff(g.download_water(), w1) == 0, (R, n, k, dr, dc)


def test_outlet_on_the_edge_row_of_a_neighbours_slab(oracle):
    _check_outlet_on_slab_edges(oracle, oracle)


@pytest.mark.gpu
def test_hip_outlet_on_the_last_row_of_the_neighbours_halo(oracle, hip):
    """found by the long fuzz hunt (seed 12601): rows sent to a neighbour did not carry the owed drain(), and a slab whose
    last row is the outlet's row never applies its own"""
    _check_outlet_on_slab_edges(hip, oracle)


def _every_height_in_slabs(lib, oracle):
    """every raster height from 20 to 75 rows on 2 and 3 slabs with a refresh every 1 and 2 iterations: each boundary position of
    the 3-row cadence, slabs of every size down to the smallest the partition accepts"""
    for R in range(20, 76):
        for n, k in ((2, 1), (3, 1), (2, 2)):
            C = 40 + R % 7
            dem, water, miss = random_case(R * 13 + n, R, C)
            bd, bw = pad(dem, water, miss)
            with oracle.context(module="add", nrows=R, ncols=C, missingvalue=miss) as c:
                c.upload(bd, bw)
                want = [c.run_block(i, 1e-5) for i in (3, 4)]
                w1 = c.download_water()
            with Group(lib, "add", R, C, miss, [0] * n, exchange_every=k) as g:
                g.upload(bd, bw)
                assert [g.run_block(i, 1e-5) for i in (3, 4)] == want, (R, n, k, g.size)
                assert n_bit_diff(g.download_water(), w1) == 0, (R, n, k, g.size)


def test_every_height_in_slabs(oracle):
    _every_height_in_slabs(oracle, oracle)


@pytest.mark.gpu
def test_hip_every_height_in_slabs(oracle, hip):
    _every_height_in_slabs(hip, oracle)
