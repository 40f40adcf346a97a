"""The spill kernels' own source (wdpm_amd/csrc/wdpm_pond_spills.hip) on the CPU: tests/spills_emu_main.cpp runs them as 256 host
threads per block under the address and undefined-behaviour sanitizers - a stand-alone program, nothing is loaded into Python - on
tables made up directly, every array of exact size, and holds the whole spill table and the counts against sequential walks."""
import re

import pytest

import emu_build

FLAGS = dict(random=0, all=1, none=2, alternating=3)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "spills_emu")


def run(emu, kind, size, seed, flags):
    out = emu_build.run(emu, kind, size, seed, FLAGS[flags])
    assert "table mismatches 0 counts agree" in out, out
    got = {k.replace(" ", "_"): int(v) for k, v in re.findall(r"(N|rings|ring ponds|spilling|max hops|rounds) (\d+)", out)}
    return got, [int(v) for v in re.search(r"ran (\d+) (\d+) (\d+)", out).groups()]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100003])
def test_random_functional_graphs(emu, n):
    got, ran = run(emu, "random", n, n, "random")
    assert got["N"] == n and got["rounds"] == (n - 1).bit_length() + 1 and all(r <= got["rounds"] for r in ran)
    if n >= 63:
        assert got["max_hops"] >= 3 and 0 < got["spilling"] < n
    if n == 100003:
        assert got["rings"] >= 1 and got["ring_ponds"] >= 2 * got["rings"]


@pytest.mark.parametrize("length", [2, 3, 64, 65, 1000])
def test_rings_with_trees_hanging_on_them(emu, length):
    """the ring, a mutual pair beside it, length / 2 + 37 ponds in trees on the ring, under shuffled labels"""
    got, ran = run(emu, "ring", length, length, "random")
    assert got["N"] == length + length // 2 + 37 + 2 and got["rings"] == 2 and got["ring_ponds"] == length + 2
    assert got["max_hops"] >= length - 1 and ran[0] <= got["rounds"]


def test_a_chain_of_65537_ponds_takes_17_rounds(emu):
    got, ran = run(emu, "chain", 65537, 1, "random")
    assert got["N"] == 65537 and got["max_hops"] == 65536 and got["rounds"] == 18 and ran[1:] == [17, 17] and got["rings"] == 0


def test_a_hub_fed_by_70000_ponds(emu):
    got, ran = run(emu, "hub", 70000, 1, "alternating")
    assert got["N"] == 70001 and got["max_hops"] == 1 and ran == [1, 1, 1] and got["spilling"] == 35000


@pytest.mark.parametrize("flags", ["all", "none", "alternating"])
@pytest.mark.parametrize("kind,size", [("random", 777), ("ring", 130), ("chain", 300)])
def test_all_none_and_every_second_pond_spilling(emu, kind, size, flags):
    got, _ = run(emu, kind, size, 9, flags)
    if flags == "none":
        assert got["spilling"] == 0
    elif flags == "all" and kind != "random":
        assert got["spilling"] == got["N"]                     # every pond of these two has an outlet
    else:
        assert got["spilling"] > 0


@pytest.mark.parametrize("flags", ["random", "all", "none", "alternating"])
def test_waves_made_lane_by_lane_for_the_votes(emu, flags):
    """A wave of hubs, then groups of 7, 8, 9 and 40; four groups of 16; 7 + 7 + 20 and its mirror; a wave whose lane 0 has no
    target; one pond in a last wave of its own.  Pond 1 and one of the eight lanes that share it are a ring of two.  The flags
    decide which lanes the live forest's votes see: every second lane halves every group - 16 become 8, 9 become 4 or 5."""
    got, ran = run(emu, "votes", 1, 1, flags)
    assert got["N"] == 64 + 5 * 64 + 1 and got["rings"] == 1 and got["ring_ponds"] == 2 and got["max_hops"] == 8
    assert got["spilling"] == {"none": 0, "alternating": 161}.get(flags, got["spilling"]) and (got["spilling"] > 300) == (flags == "all")
    assert ran[1:] == [4, 4] and 2 <= ran[0] <= got["rounds"] == 10       # links reach 1, 2, 4 and 8 ponds on: four rounds with work


def test_the_vote_waves_three_times_over_cross_the_blocks_elsewhere(emu):
    got, ran = run(emu, "votes", 3, 2, "random")
    assert got["N"] == 64 + 15 * 64 + 1 and got["rings"] == 1 and got["ring_ponds"] == 2 and ran[1:] == [4, 4]
