"""The host model of the pond routing (tests/pond_routing_model.py) against answers written out by hand, against an independent
brute force - out = f(in) over all ponds until nothing changes - on random forests, and against the invariants of
include/wdpm_pond_routing.h.  No GPU, no library: plain Python."""
import numpy as np
import pytest

from pond_routing_model import ROUTE_DTYPE, assert_invariants, brute_force, level_sizes, plan_of, routing, runoff_q_of
from pond_spills_model import graph

TOP_Q = 255 * 2 ** 24


def route(to, values, fill_q, runoff_q):
    spill_table, _ = graph(to, [False] * len(to), values, fill_q)
    table, stats = routing(spill_table, values, fill_q, runoff_q)
    assert_invariants(table, stats, spill_table, values, fill_q)
    return table, stats, spill_table


def column(table, name):
    return [int(v) for v in table[name].tolist()]


def test_the_runoff_rule():
    assert runoff_q_of(0.0) == 0 and runoff_q_of(0.001) == 16777 and runoff_q_of(1.0) == 2 ** 24 and runoff_q_of(255.0) == TOP_Q
    assert runoff_q_of(2.0 ** -25) == 0 and runoff_q_of(3 * 2.0 ** -25) == 2            # halves go to the even quantum
    assert runoff_q_of(256.0 - 2.0 ** -24) == 2 ** 32 - 1 and runoff_q_of(256.0) == -1 and runoff_q_of(256.0 - 2.0 ** -26) == -1
    assert runoff_q_of(-0.0) == 0
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf"), 1e300):
        assert runoff_q_of(bad) == -1


@pytest.mark.parametrize("fill_2,out_2", [(130, 0), (129, 1)])
def test_a_chain_of_three_whose_middle_pond_fills_exactly_and_one_quantum_more(fill_2, out_2):
    """1 -> 2 -> 3 -> land, 5 quanta on 10, 20 and 30 cells: pond 1 passes 30 on, pond 2 then holds 130"""
    t, s, sp = route([2, 3, 0], [10, 20, 30], [20, fill_2, 1000], 5)
    assert sp["hops"].tolist() == [2, 1, 0] == t["level"].tolist()
    assert column(t, "own_q") == [50, 100, 150] and column(t, "in_q") == [0, 30, out_2] and column(t, "out_q") == [30, out_2, 0]
    assert column(t, "kept_q") == [20, fill_2, 150 + out_2]
    assert t["full"].tolist() == [1, 1, 0] and t["overflows"].tolist() == [1, out_2, 0]
    assert t["reach_ponds"].tolist() == [1, 2, 3 if out_2 else 1] and t["reach_cells"].tolist() == [10, 30, 60 if out_2 else 30]
    assert s == dict(ponds=3, runoff_q=5, levels=3, overflowing=1 + out_2, full=2, own_q=300, kept_q=300, out_land_q=0, out_ring_q=0)


def test_a_hub():
    """ponds 2..6 spill into pond 1, which leaves onto land: two of the five overflow, then the hub does"""
    t, s, _ = route([0, 1, 1, 1, 1, 1], [100, 1, 2, 3, 4, 5], [150, 10, 10, 10, 45, 30], 10)
    assert column(t, "out_q") == [1000 + 10 + 20 + 20 - 150, 0, 10, 20, 0, 20] and column(t, "in_q") == [50, 0, 0, 0, 0, 0]
    assert t["reach_ponds"].tolist() == [4, 1, 1, 1, 1, 1] and t["reach_cells"].tolist() == [100 + 2 + 3 + 5, 1, 2, 3, 4, 5]
    assert t["full"].tolist() == [1, 1, 1, 1, 0, 1] and t["overflows"].tolist() == [1, 0, 1, 1, 0, 1] and t["level"].tolist() == [0, 1, 1, 1, 1, 1]
    assert s["out_land_q"] == 900 and s["kept_q"] == 150 + 10 + 10 + 10 + 40 + 30 and s["own_q"] == 1150 and s["levels"] == 2


def test_a_pond_without_an_outlet_below_an_overflowing_pond():
    t, s, _ = route([2, -1], [4, 6], [10, 0], 100)
    assert column(t, "out_q") == [390, 0] and column(t, "in_q") == [0, 390] and column(t, "kept_q") == [10, 990]
    assert t["full"].tolist() == [1, 0] and t["overflows"].tolist() == [1, 0] and t["reach_ponds"].tolist() == [1, 2]
    assert s["out_land_q"] == 0 and s["out_ring_q"] == 0 and s["kept_q"] == s["own_q"] == 1000


def test_a_mutual_pair_whose_heads_overflow_leaves_at_the_ring():
    t, s, sp = route([2, 1], [5, 7], [30, 20], 10)
    assert sp["next"].tolist() == [-2, 1]
    assert column(t, "out_q") == [50 + 50 - 30, 50] and column(t, "in_q") == [50, 0]              # nothing enters pond 2 again
    assert s["out_ring_q"] == 70 and s["out_land_q"] == 0 and t["reach_ponds"].tolist() == [2, 1] and t["level"].tolist() == [0, 1]


def test_fill_q_above_2_to_the_53():
    """quantities no double holds: one quantum decides"""
    area, q = 2 ** 30, 2 ** 32 - 1
    own = area * q
    assert own > 2 ** 61
    for fill, out in ((own, 0), (own - 1, 1), (own + 1, 0)):
        t, s, _ = route([2, 0], [area, 3], [fill, 2 ** 63], q)
        assert column(t, "out_q") == [out, 0] and column(t, "kept_q") == [own - out, 3 * q + out] and t["full"].tolist() == [int(fill <= own), 0]
        assert t["own_q"].dtype == np.uint64 and int(t["own_q"][0]) == own


def random_forest(rng, n):
    to = []
    for k in range(1, n + 1):
        u = int(rng.integers(100))
        j = 0 if u < 8 else -1 if u < 14 else 1 + int(rng.integers(n))
        if j == k:
            j = k % n + 1 if n > 1 else 0
        to.append(j)
    values = [1 + int(rng.integers(5000)) for _ in range(n)]
    kind = int(rng.integers(3))                               # shallow, mixed and deep storage: few, some and most ponds overflow
    fill = [0 if t == -1 else int(rng.integers(1, 2 ** (14 + 12 * kind))) * int(rng.integers(1, v + 1)) for t, v in zip(to, values)]
    return to, values, fill


@pytest.mark.parametrize("seed", range(12))
def test_against_the_brute_force_on_random_forests(seed):
    rng = np.random.default_rng(seed)
    n = (1, 2, 3, 17, 64, 65, 100, 150, 150, 150, 149, 128)[seed]
    to, values, fill = random_forest(rng, n)
    spill_table, _ = graph(to, [False] * n, values, fill)
    for q in (0, 1, 16777, 2 ** 24, int(rng.integers(2 ** 32)), 2 ** 32 - 1):
        table, stats = routing(spill_table, values, fill, q)
        assert_invariants(table, stats, spill_table, values, fill)
        own, inq, kept, out, reach_p, reach_c = brute_force(spill_table["next"].tolist(), values, fill, q)
        for name, want in (("own_q", own), ("in_q", inq), ("kept_q", kept), ("out_q", out), ("reach_ponds", reach_p), ("reach_cells", reach_c)):
            assert column(table, name) == want, (name, q)


@pytest.mark.parametrize("seed", range(4))
def test_invariants_over_rising_runoff(seed):
    rng = np.random.default_rng(100 + seed)
    to, values, fill = random_forest(rng, 120)
    fill = [min(f, 200 * 2 ** 24 * v) for f, v in zip(fill, values)]                    # every basin is full at 255 m
    spill_table, _ = graph(to, [False] * 120, values, fill)
    before = None
    for q in (0, 1, 1000, 16777, 2 ** 20, 2 ** 24, 2 ** 28, TOP_Q):
        table, stats = routing(spill_table, values, fill, q)
        assert_invariants(table, stats, spill_table, values, fill)
        if q == 0:                                            # no runoff: zeros, and every pond alone
            for name in ("own_q", "in_q", "kept_q", "out_q", "overflows"):
                assert not table[name].any()
            assert (table["reach_ponds"] == 1).all() and (table["reach_cells"] == values).all()
            assert (table["full"] == ((spill_table["next"] != -1) & (np.asarray(fill) == 0))).all()
        if q == TOP_Q:                                        # everything with an outlet overflows: all that is upstream is connected
            assert (table["reach_ponds"] == spill_table["up_ponds"]).all() and (table["reach_cells"] == spill_table["up_cells"]).all()
        if before is not None:
            assert (table["out_q"] >= before["out_q"]).all() and (table["reach_ponds"] >= before["reach_ponds"]).all()
            assert (table["reach_cells"] >= before["reach_cells"]).all()
        before = table


def test_level_sizes_and_the_plan_in_words():
    spill_table, _ = graph([0, 1, 1, 2, 4, 5], [False] * 6, [1] * 6, [1] * 6)
    assert level_sizes(spill_table) == [1, 2, 1, 1, 1] and level_sizes(spill_table[:0]) == []
    assert plan_of([1, 2, 1, 1, 1]) == [("run", 4, 5)] and plan_of([1, 2, 1, 1, 1], narrow=1) == [("run", 4, 3), ("wide", 1), ("run", 0, 1)]
    assert plan_of([1] * 7, run_levels=3) == [("run", 6, 3), ("run", 3, 3), ("run", 0, 1)] and plan_of([]) == []
    assert plan_of([256, 257]) == [("wide", 1), ("run", 0, 1)] and ROUTE_DTYPE.itemsize == 64
