"""The host model of the pond spills (tests/pond_spills_model.py) against answers written out by hand - a mutual pair, a ring of three
with a tail, a chain onto land beside a pond without an outlet, a hub - against a brute-force walk of every pond's whole chain on
random graphs, and against the invariants include/wdpm_pond_spills.h implies."""
import numpy as np
import pytest

from pond_spills_model import SPILL_DTYPE, assert_invariants, assert_same_spills, brute_force, graph, rings_of, rounds_of, spills


def rows(table, name):
    return table[name].tolist()


def test_layout():
    assert SPILL_DTYPE.itemsize == 80
    assert [SPILL_DTYPE.fields[n][1] for n in SPILL_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72]
    assert [rounds_of(n) for n in (0, 1, 2, 3, 4, 5, 64, 65, 65537)] == [0, 3, 6, 9, 9, 12, 21, 24, 54]


def test_a_mutual_pair():
    t, s = graph([2, 1], [True, True], [10, 20], [5, 7])
    assert rows(t, "next") == [-2, 1] and rows(t, "sink") == [1, 1] and rows(t, "end") == [-2, -2] and rows(t, "hops") == [0, 1]
    assert rows(t, "path_fill_q") == [5, 12] and rows(t, "up_ponds") == [2, 1] and rows(t, "up_cells") == [30, 20]
    assert rows(t, "up_fill_q") == [12, 7] and rows(t, "rest") == [1, 1] and rows(t, "rest_hops") == [0, 1]
    assert rows(t, "live_ponds") == [2, 1] and rows(t, "live_cells") == [30, 20] and rows(t, "spilling") == [1, 1]
    assert s == dict(ponds=2, rings=1, ring_ponds=2, spilling=2, ends_land=0, ends_none=0, ends_ring=1, max_hops=1, rounds=6)
    t, s = graph([2, 1], [True, False], [10, 20], [5, 7])          # pond 2 holds its water: nothing is connected to pond 1 now
    assert rows(t, "rest") == [1, 2] and rows(t, "rest_hops") == [0, 0] and rows(t, "live_ponds") == [1, 1]
    assert rows(t, "live_cells") == [10, 20] and rows(t, "up_ponds") == [2, 1] and s["spilling"] == 1


def test_a_ring_of_three_with_a_tail():
    """1 -> 3 -> 2 -> 1, and 4 -> 2: the head is 1, so the forest is 3 -> 2 -> 1 and 4 -> 2 -> 1"""
    t, s = graph([3, 1, 2, 2], [False, True, False, True], [1, 2, 3, 4], [10, 20, 30, 40])
    assert rings_of([3, 1, 2, 2]) == [[1, 3, 2]]
    assert rows(t, "next") == [-2, 1, 2, 2] and rows(t, "sink") == [1] * 4 and rows(t, "end") == [-2] * 4 and rows(t, "hops") == [0, 1, 2, 2]
    assert rows(t, "path_fill_q") == [10, 30, 60, 70] and rows(t, "up_ponds") == [4, 3, 1, 1] and rows(t, "up_cells") == [10, 9, 3, 4]
    assert rows(t, "up_fill_q") == [100, 90, 30, 40] and rows(t, "rest") == [1, 1, 3, 1] and rows(t, "rest_hops") == [0, 1, 0, 2]
    assert rows(t, "live_ponds") == [3, 2, 1, 1] and rows(t, "live_cells") == [7, 6, 3, 4]
    assert s == dict(ponds=4, rings=1, ring_ponds=3, spilling=2, ends_land=0, ends_none=0, ends_ring=1, max_hops=2, rounds=9)


def test_a_chain_onto_land_and_a_pond_without_an_outlet():
    """1 -> 2 -> 3 -> land; 4 has no outlet and can never spill; fill_q above 2^53 adds up exactly"""
    big = 2 ** 60 + 1
    t, s = graph([2, 3, 0, -1], [True, True, True, False], [5, 6, 7, 8], [big, 2, big, 0])
    assert rows(t, "next") == [2, 3, 0, -1] and rows(t, "sink") == [3, 3, 3, 4] and rows(t, "end") == [0, 0, 0, -1]
    assert rows(t, "hops") == [2, 1, 0, 0] and rows(t, "path_fill_q") == [2 * big + 2, big + 2, big, 0]
    assert rows(t, "up_ponds") == [1, 2, 3, 1] and rows(t, "up_cells") == [5, 11, 18, 8] and rows(t, "up_fill_q") == [big, big + 2, 2 * big + 2, 0]
    assert rows(t, "rest") == [3, 3, 3, 4] and rows(t, "rest_hops") == [2, 1, 0, 0]      # all of them spill: the water rests at the sink
    assert rows(t, "live_ponds") == [1, 2, 3, 1] and rows(t, "live_cells") == [5, 11, 18, 8]
    assert s == dict(ponds=4, rings=0, ring_ponds=0, spilling=3, ends_land=1, ends_none=1, ends_ring=0, max_hops=2, rounds=9)
    t, s = graph([2, 3, 0, -1], [True, False, True, False], [5, 6, 7, 8], [1, 2, 3, 0])
    assert rows(t, "rest") == [2, 2, 3, 4] and rows(t, "rest_hops") == [1, 0, 0, 0] and rows(t, "live_ponds") == [1, 2, 1, 1]
    assert rows(t, "live_cells") == [5, 11, 7, 8]


def test_a_hub():
    """ponds 2..200 all spill into pond 1, which spills onto land; every other feeder stands at its pour level"""
    n = 200
    spilling = [False] + [k % 2 == 0 for k in range(2, n + 1)]
    t, s = graph([0] + [1] * (n - 1), spilling, list(range(1, n + 1)), [3] * n)
    assert t["up_ponds"][0] == n and t["up_cells"][0] == n * (n + 1) // 2 and t["up_fill_q"][0] == 3 * n
    assert t["live_ponds"][0] == 1 + 100 and t["live_cells"][0] == 1 + sum(range(2, n + 1, 2))
    assert rows(t, "up_ponds")[1:] == [1] * (n - 1) and rows(t, "hops") == [0] + [1] * (n - 1) and rows(t, "path_fill_q") == [3] + [6] * (n - 1)
    assert rows(t, "rest")[1:] == [1 if k % 2 == 0 else k for k in range(2, n + 1)]
    assert s == dict(ponds=n, rings=0, ring_ponds=0, spilling=100, ends_land=1, ends_none=0, ends_ring=0, max_hops=1, rounds=27)


def test_no_pond_and_one_pond():
    t, s = graph([], [], [], [])
    assert len(t) == 0 and s == dict(ponds=0, rings=0, ring_ponds=0, spilling=0, ends_land=0, ends_none=0, ends_ring=0, max_hops=0, rounds=0)
    t, s = graph([0], [True], [9], [4])
    assert t.tolist() == [(0, 1, 0, 0, 1, 0, 1, 0, 4, 1, 9, 4, 1, 9)] and s["ends_land"] == 1 and s["rounds"] == 3


def random_graph(rng, n, p_end=0.2):
    """a functional graph without self loops: every pond spills into another one, onto land or nowhere"""
    to = []
    for k in range(1, n + 1):
        u = rng.random()
        if u < p_end or n == 1:
            to.append(0 if u < p_end / 2 else -1)
        else:
            j = int(rng.integers(1, n))
            to.append(j if j < k else j + 1)
    spilling = [(t >= 0) and bool(rng.random() < 0.6) for t in to]
    return to, spilling, rng.integers(1, 1000, n).tolist(), [int(v) for v in rng.integers(0, 2 ** 55, n)]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 40, 150])
def test_against_the_brute_force_walk_and_the_invariants(n):
    rng = np.random.default_rng(n)
    rings = 0
    for trial in range(12):
        to, spilling, values, fq = random_graph(rng, n, p_end=[0.0, 0.05, 0.3][trial % 3])
        t, s = graph(to, spilling, values, fq)
        bt, bs = brute_force(to, spilling, values, fq)
        assert_same_spills(t, s, bt, bs)
        assert_invariants(t, values, fq)
        rings += s["rings"]
        assert s["ends_ring"] == s["rings"] and s["ends_land"] + s["ends_none"] + s["ends_ring"] == int((t["next"] <= 0).sum())
    assert n < 3 or rings > 0


def test_from_the_tables_of_the_older_models():
    """spills() reads cells, surface_max, catch_cells and pour_level / to_basin / fill_q, and the tolerance is a double compared as one"""
    from pond_catchments_model import CATCH_DTYPE
    from pond_outlets_model import OUTLET_DTYPE
    from pond_rims_model import RIM_DTYPE
    from ponds_model import POND_DTYPE
    ponds, rims, catch, out = (np.zeros(3, dtype=d) for d in (POND_DTYPE, RIM_DTYPE, CATCH_DTYPE, OUTLET_DTYPE))
    ponds["cells"], catch["catch_cells"] = [1, 2, 3], [10, 20, 30]
    out["to_basin"], out["fill_q"] = [2, 0, -1], [7, 8, 0]
    out["pour_level"] = [100.0, 90.0, np.inf]
    rims["surface_max"] = [100.0, np.nextafter(90.0, 0.0), 50.0]          # at the pour level; one step of the format below it; no outlet
    t, s = spills(ponds, rims, catch, out, 0.0)
    assert rows(t, "spilling") == [1, 0, 0] and rows(t, "up_cells") == [11, 33, 33] and rows(t, "live_cells") == [11, 33, 33]
    assert rows(t, "rest") == [2, 2, 3] and rows(t, "path_fill_q") == [15, 8, 0] and s["spilling"] == 1
    t, s = spills(ponds, rims, catch, out, 0.001)
    assert rows(t, "spilling") == [1, 1, 0] and s["spilling"] == 2 and s["ends_none"] == 1
    assert_invariants(t, [11, 22, 33], out["fill_q"], out["pour_level"])
