"""TEST INFRASTRUCTURE: the scenes of tests/pond_spill_scenes.py that are built to put chosen targets into chosen lanes of the spill
kernels' waves (wdpm_amd/csrc/wdpm_pond_spills.hip: push_group's votes, the wave and block edges of N, the buffers a pass ends in),
each with the claim it must fulfil ON THE MODEL: tests/test_pond_spill_scenes.py asserts the claims without a device,
tests/test_pond_spill_votes.py asserts them again and then asks the device for the same tables.

    CASES[name] = (scene, claim, calls)       scene() -> (dem, water); claim(table, stats, tables); calls: ((min_depth, tol), ...)

The kernels run one lane per pond in label order: pond k is lane (k - 1) % 64 of wave (k - 1) // 64, four waves to a block.  A
claim reads what the lanes of a wave hold from pond_spills_model.wave_targets - a walk, pond by pond."""
import numpy as np

import pond_spill_scenes as scenes
from pond_spills_model import rounds_run_of, wave_targets

WET = 0.001
HUB_LANES = 8                                  # push_group takes the lanes of a wave together from this many sharers on
BOTH_TOLERANCES = ((WET, 0.0), (WET, 0.5))     # at 0.5 m a cascade's lakes spill as well: their sills lie 1/2 m above them
PARITY_STEPS = (2, 3, 4, 5, 8, 9, 16, 17)
EDGE_STEPS = (63, 64, 65, 255, 256, 257)


def lane_targets(t, wave):
    """next of the 64 ponds of one wave, lane by lane"""
    return t["next"][64 * wave:64 * wave + 64].tolist()


def lanes_of(t, wave, target):
    return [lane for lane, j in enumerate(lane_targets(t, wave)) if j == target]


def claim_vote_boundary(t, s, tables):
    n = s["ponds"]
    assert n == 6 * 64 + 1 and s["rings"] == 0 and t["next"][:2].tolist() == [2, 0] and t["next"][-1] == 0
    waves = wave_targets(t["next"], t["spilling"])
    for first, k in ((1, 7), (2, 8), (3, 9), (4, 7), (5, 8)):
        forest, live = waves[first]
        assert forest == {2: k, n: 64 - k} and live[2] == k and HUB_LANES <= live[n] < 64 - k
        lanes = lanes_of(t, first, 2)
        assert min(lanes) < 8 and max(lanes) > 56 and sum(lane < 32 for lane in lanes) >= 3 and sum(lane >= 32 for lane in lanes) >= 3
        if first <= 3:                                          # the small group holds lanes 0 and 63: its vote is the first
            assert lanes[0] == 0 and lanes[-1] == 63
        else:                                                   # the big group is asked first, the small one second
            assert lanes[0] == 1 and lanes[-1] == 62
    assert t["up_ponds"][1] == 2 + 39 and t["live_ponds"][1] in (1 + 39, 2 + 39)


def claim_live_is_not_forest(t, s, tables):
    n = s["ponds"]
    assert n == 5 * 64 + 1 and s["rings"] == 0
    waves = wave_targets(t["next"], t["spilling"])
    for wave, full in ((1, 7), (2, 8), (3, 7), (4, 8)):
        forest, live = waves[wave]
        assert forest == {2: 12, n: 52} and live[2] == full and HUB_LANES <= live[n] < 52
        lanes = lanes_of(t, wave, 2)
        assert (lanes[0], lanes[-1]) == ((0, 63) if wave <= 2 else (1, 62))
    assert t["up_ponds"][1] == 2 + 48 and t["live_ponds"][1] in (1 + 30, 2 + 30)


def claim_four_hubs(t, s, tables):
    n = s["ponds"]
    assert n == 4 * 64 + 2 and s["rings"] == 0 and t["next"][:2].tolist() == [2, 0] and t["next"][-2:].tolist() == [n, 0]
    waves = wave_targets(t["next"], t["spilling"])
    assert waves[1][0] == waves[1][1] == {1: 16, 2: 16, n - 1: 16, n: 16}            # four targets for three votes
    assert lane_targets(t, 1)[:2] == [1, n - 1] and lane_targets(t, 1)[32:34] == [2, n]
    assert waves[2][0] == {2: 32, n: 32} and waves[2][1] == {2: 21, n: 21}
    assert t["up_ponds"][0] == 17 and t["up_ponds"][1] == 17 + 1 + 16 + 32


def claim_failed_votes(t, s, tables):
    n = s["ponds"]
    assert n == 3 * 64 + 3 + 1 and s["rings"] == 0 and t["next"][:3].tolist() == [2, 3, 0]
    waves = wave_targets(t["next"], t["spilling"])
    assert waves[1][0] == waves[1][1] == {1: 7, n: 7, 2: 50}
    assert lane_targets(t, 1) == [1, n] * 7 + [2] * 50                               # 7 and 7 first: no vote succeeds
    assert waves[2][0] == waves[2][1] == {2: 50, 3: 7, n: 7}
    assert lane_targets(t, 2) == [2] * 50 + [3, n] * 7                               # the mirror: the big group first
    assert min(7, 7) < HUB_LANES <= 20 <= 50


def claim_lane_0_on_land(t, s, tables):
    n = s["ponds"]
    assert n == 64 + 4 + 1 and t["next"][0] == 0 and t["end"][0] == 0
    forest, live = wave_targets(t["next"], t["spilling"])[0]
    assert forest == {1: 8, n: 55} and live[1] == 8 and lanes_of(t, 0, 1)[0] == 5
    assert t["up_ponds"][0] == 1 + 8 + 2 and s["ends_land"] == 2


def claim_ring_through_a_hub(t, s, tables):
    n = s["ponds"]
    to = tables["outlets"]["to_basin"]
    assert n == 128 + 5 + 1 and s["rings"] == 2 and s["ring_ponds"] == 2 * s["rings"] and s["ends_ring"] == 2
    assert t["next"][0] == -2 and to[0] == 6 and to[5] == 1                          # the lake is the head, the pit of lane 5 is marked
    forest, _ = wave_targets(t["next"], t["spilling"])[0]
    assert forest[1] >= HUB_LANES and 5 in lanes_of(t, 0, 1) and lanes_of(t, 0, 1)[0] == 5
    feeders = np.flatnonzero(t["next"] == 1)
    assert len(feeders) >= 10 and (t["end"][feeders] == -2).all() and (t["sink"][feeders] == 1).all()
    assert to[1] == n and to[n - 1] == 2 and t["next"][1] == -2 and t["next"][n - 1] == 2      # below: the pit of lane 1 is the head
    assert forest[n] >= 40 and (t["end"][t["next"] == n] == -2).all()


def claim_cascade(t, s, tables):
    n = s["ponds"]
    assert n == 3 + 235 + 1 and s["rings"] == 0 and s["max_hops"] == 3 and t["next"][:3].tolist() == [2, 3, 0]
    fed = [int((t["next"] == lake).sum()) for lake in (1, 2, 3)]
    assert fed == [70, 71, 71]                                                         # 70 pits each, and the lake before
    assert t["up_ponds"][2] == 3 + 210 == int((t["sink"] == 3).sum()) and t["up_ponds"][:2].tolist() == [71, 142]
    assert t["up_cells"][2] == int((tables["ponds"]["cells"] + tables["catchments"]["catch_cells"])[t["sink"] == 3].sum())
    second = wave_targets(t["next"], t["spilling"], steps=2)                           # what round 1 of the sums pass sees
    assert second[0][0] == {2: 64 - 3, 3: 1} and second[1][0] == {2: 9, 3: 55}
    if t["spilling"][0]:                                                               # the lakes spill (tolerance 0.5): live hubs of hubs
        assert second[0][1][2] >= 32 and second[1][1][3] >= 32 and t["live_ponds"][2] >= 3 + 128
    else:
        assert second[0][1] == second[1][1] == {} and t["live_ponds"][2] < 64
    third = wave_targets(t["next"], t["spilling"], steps=3)
    assert third[0][0] == {3: 61}


def claim_hub_last(ponds):
    def claim(t, s, tables):
        n = s["ponds"]
        assert n == ponds and t["next"][n - 1] == 0 and int((t["next"] == n).sum()) == ponds - 2 - 9
        assert t["up_ponds"][n - 1] == ponds - 10 and t["up_ponds"][0] == 10
        last = wave_targets(t["next"], t["spilling"])[-1][0]
        assert last == ({n: 62, 1: 1} if ponds == 256 else {})                            # at 257 the hub is alone in its wave and block
    return claim


def claim_staircase(steps):
    def claim(t, s, tables):
        assert s["ponds"] == steps and (t["next"][:steps - 2] == np.arange(2, steps)).all() and s["max_hops"] >= steps - 2
        assert 0 < s["spilling"] <= steps
    return claim


def staircase_of(steps):
    return lambda: scenes.staircase(steps)


def claim_random_comb(rings):
    def claim(t, s, tables):
        assert s["ponds"] == 307 and s["rings"] == rings and s["ring_ponds"] == 2 * rings
        if rings == 0:
            assert t["next"][:4].tolist() == [2, 3, 4, 0] and s["max_hops"] == 4
    return claim


def random_comb(cascade):
    def scene():
        rng = np.random.default_rng(1)
        return scenes.comb(rng.random(300) < 0.5, rng.random(300) < 0.5, (70, 150, 230), (100, 200), cascade)
    return scene


CASES = {
    "vote_boundary": (scenes.vote_boundary, claim_vote_boundary, BOTH_TOLERANCES),
    "live_is_not_forest": (scenes.live_is_not_forest, claim_live_is_not_forest, BOTH_TOLERANCES),
    "four_hubs": (scenes.four_hubs, claim_four_hubs, ((WET, 0.0),)),
    "failed_votes": (scenes.failed_votes, claim_failed_votes, ((WET, 0.0),)),
    "lane_0_on_land": (scenes.lane_0_on_land, claim_lane_0_on_land, ((WET, 0.0),)),
    "ring_through_a_hub": (scenes.ring_through_a_hub, claim_ring_through_a_hub, ((WET, 0.0),)),
    "cascade": (scenes.cascade, claim_cascade, BOTH_TOLERANCES),
    "random_comb_cascade": (random_comb(True), claim_random_comb(0), ((WET, 0.0),)),
    "random_comb_rings": (random_comb(False), claim_random_comb(7), ((WET, 0.0),)),
    "hub_last_256": (lambda: scenes.hub_last(256), claim_hub_last(256), ((WET, 0.0),)),
    "hub_last_257": (lambda: scenes.hub_last(257), claim_hub_last(257), ((WET, 0.0),)),
}
CASES.update({f"staircase_{n}": (staircase_of(n), claim_staircase(n), ((WET, 0.0),)) for n in EDGE_STEPS + PARITY_STEPS})
# every buffer parity of the ring pass: a staircase's ring pass always ends after one round (or two, with a pair at its foot)
PARITY_CASES = tuple(f"staircase_{n}" for n in PARITY_STEPS) + ("ring_through_a_hub",)


def rounds_run_in(case, reference):
    """rounds_run_of for a case, from the model's tables: reference(bd, bw, md, tol) -> (table, stats, tables)"""
    t, s, tables = reference
    return rounds_run_of(tables["outlets"]["to_basin"], t["spilling"])
