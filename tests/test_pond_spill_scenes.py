"""What every scene of tests/pond_spill_cases.py must give, asserted on the host model (tests/pond_spills_model.py) - no device here.
tests/test_pond_spill_votes.py runs the same scenes through the spill kernels; a ground that fails to put the targets into the
lanes it is named after fails here first.  Also the two helpers the claims are read with: wave_targets and rounds_run_of."""
import numpy as np
import pytest

import pond_spill_scenes as scenes
from helpers import pad
from pond_spill_cases import CASES, EDGE_STEPS, PARITY_CASES, PARITY_STEPS, rounds_run_in
from pond_spills_model import assert_invariants, graph, rounds_run_of, spills_of_water, wave_targets

MISS = scenes.MISS
_MODEL = {}


def model(name, call=0):
    """(table, stats, tables) of a case's scene under its call number `call`: computed once"""
    if (name, call) not in _MODEL:
        scene, _, calls = CASES[name]
        bd, bw = pad(*scene(), MISS)
        _MODEL[name, call] = spills_of_water(bd, MISS, bw, *calls[call])
    return _MODEL[name, call]


# ---- the helpers -----------------------------------------------------------------------------------------------------------------
def test_wave_targets_on_a_graph_written_out_by_hand():
    """1 -> 2 -> 3 -> land, 4 and 5 -> 2, 6 without an outlet; pond 2 holds its water; waves of four lanes"""
    to, spilling = [2, 3, 0, 2, 2, -1], [True, False, True, True, False, False]
    assert wave_targets(to, spilling, wave=4) == [({2: 2, 3: 1}, {2: 2}), ({2: 1}, {})]
    assert wave_targets(to, spilling, steps=2, wave=4) == [({3: 2}, {}), ({3: 1}, {})]
    assert wave_targets(to, [True] * 6, steps=2, wave=4) == [({3: 2}, {3: 2}), ({3: 1}, {3: 1})]
    assert wave_targets(to, spilling, steps=3, wave=4) == [({}, {}), ({}, {})]
    assert wave_targets([], []) == []


def test_rounds_run_of_on_graphs_written_out_by_hand():
    assert rounds_run_of([], []) == (0, 0, 0)
    assert rounds_run_of([0], [False]) == (0, 0, 0)                                   # nothing has a target: no round has work
    assert rounds_run_of([2, 1], [True, True]) == (2, 1, 1)                           # round 0 lowers pond 1's minimum, round 1 nothing
    assert rounds_run_of([2, 3, 1], [True] * 3) == (3, 2, 2)                          # a ring of three: all three rounds of N = 3
    # a chain of N ponds: the ring pass finds nothing to lower; the links reach 2^r ponds on while 2^r <= N - 1
    for n, chain in ((2, 1), (3, 2), (4, 2), (5, 3), (8, 3), (9, 4), (16, 4), (17, 5), (1000, 10)):
        assert rounds_run_of(list(range(2, n + 1)) + [0], [True] * n) == (1, chain, chain)
    rng = np.random.default_rng(4)
    for n in (7, 64, 150):                                                            # never more than the launches there are
        to = [int(j) if j != k else 0 for k, j in enumerate(rng.integers(-1, n + 1, n), 1)]
        ran = rounds_run_of(to, rng.random(n) < 0.5)
        hops = graph(to, [True] * n, [1] * n, [1] * n)[1]["max_hops"]
        assert max(ran) <= (n - 1).bit_length() + 1 and ran[1] == ran[2] == (hops.bit_length() if hops else 0)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_scene_gives_what_it_is_named_after(name):
    scene, claim, calls = CASES[name]
    dem, water = scene()
    assert dem.shape == water.shape and dem.shape[0] in (5, 7) and dem.shape[1] <= 800
    assert (np.round(dem[dem > MISS] * 8) == dem[dem > MISS] * 8).all() and (np.round(water * 8) == water * 8).all()
    for call in range(len(calls)):
        t, s, tables = model(name, call)
        claim(t, s, tables)
        assert_invariants(t, tables["ponds"]["cells"] + tables["catchments"]["catch_cells"], tables["outlets"]["fill_q"],
                          tables["outlets"]["pour_level"])


@pytest.mark.parametrize("name", ["vote_boundary", "live_is_not_forest"])
def test_the_second_tolerance_lets_the_lakes_spill(name):
    """at 0.5 m the first upper lake, 1/2 m under its sill, spills as well: the live sums of the lake below it grow by that one pond"""
    (t0, s0, _), (t1, s1, _) = model(name, 0), model(name, 1)
    assert CASES[name][2][1][1] == 0.5 and s1["spilling"] == s0["spilling"] + 3 and (t0["next"] == t1["next"]).all()
    assert t0["spilling"][0] == 0 and t1["spilling"][0] == 1 and t1["live_ponds"][1] == t0["live_ponds"][1] + 1
    assert (t0["up_ponds"] == t1["up_ponds"]).all()


@pytest.mark.parametrize("steps", EDGE_STEPS)
def test_a_staircase_has_as_many_ponds_as_steps(steps):
    t, s, tables = model(f"staircase_{steps}")
    assert s["ponds"] == steps == len(t)                       # 63, 64, 65: one wave less a lane, one wave, one lane more; 255 .. 257: blocks


def test_every_pass_ends_in_either_buffer():
    """The results of a pass lie in buffer (rounds run & 1).  Over the family, every pass ends in buffer 0 and in buffer 1.  A
    staircase's ring pass runs one round - nothing on a chain lowers a minimum - except where the last bowl is not full and spills
    back (4 and 16 steps: a pair at the foot, two rounds); the ring through a hub adds a second scene with two rounds."""
    ran = {name: rounds_run_in(name, model(name)) for name in PARITY_CASES}
    for p in range(3):
        assert {r[p] & 1 for r in ran.values()} == {0, 1}, (p, ran)
    assert [ran[f"staircase_{n}"][1] for n in PARITY_STEPS] == [1, 2, 2, 3, 3, 4, 4, 5]
    assert [ran[f"staircase_{n}"][0] for n in PARITY_STEPS] == [1, 1, 2, 1, 1, 1, 2, 1] and ran["ring_through_a_hub"][0] == 2
    assert all(r[1] == r[2] for r in ran.values())             # the sums pass doubles the same links as the chain pass
