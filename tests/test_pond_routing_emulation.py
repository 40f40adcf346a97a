"""The routing kernels' own source (wdpm_amd/csrc/wdpm_pond_routing.hip) on the CPU: tests/routing_emu_main.cpp runs them as 256 host
threads per block, with a real block barrier between the levels of a run, under the address and undefined-behaviour sanitizers - a
stand-alone program, nothing is loaded into Python - on tables made up directly, every array of exact size, and holds the order, the
whole routing table and the totals against a sequential walk.  What the emulation cannot show is whether a word added to by another
wave is read fresh on the device: tests/test_pond_routing.py compares the runs exactly on the GPU."""
import re

import pytest

import emu_build

MM, M, TOP = 16777, 2 ** 24, 2 ** 32 - 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return emu_build.build(tmp_path_factory, "routing_emu")


def run(emu, kind, size, seed, *runoffs, narrow=256, run_levels=65536):
    out = emu_build.run(emu, kind, size, seed, narrow, run_levels, *runoffs)
    lines = [ln for ln in out.splitlines() if "table mismatches" in ln]
    assert len(lines) == len(runoffs) and "order sorted" in out, out
    got = []
    for ln, q in zip(lines, runoffs):
        assert f"runoff_q {q}:" in ln and "table mismatches 0 totals agree" in ln, out
        got.append({k.replace(" ", "_"): int(v) for k, v in re.findall(r"(N|levels|launches|wide|overflowing|full|land|ring) (\d+)", ln)})
    return got, out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 100003])
def test_random_forests(emu, n):
    got, _ = run(emu, "random", n, n, M)
    assert got[0]["N"] == n and got[0]["launches"] >= 1
    if n == 100003:
        assert got[0]["levels"] >= 5 and got[0]["wide"] >= 2 and got[0]["launches"] > got[0]["wide"]
        assert 0 < got[0]["overflowing"] <= got[0]["full"] < n and got[0]["land"] > 0 and got[0]["ring"] > 0


def test_a_chain_of_65537_ponds_is_two_runs(emu):
    got, _ = run(emu, "chain", 65537, 1, 255 * M)
    assert got[0] == dict(got[0], N=65537, levels=65537, launches=2, wide=0) and got[0]["overflowing"] > 30000


def test_a_hub_fed_by_70000_ponds(emu):
    got, _ = run(emu, "hub", 70000, 1, M)
    assert got[0] == dict(got[0], N=70001, levels=2, launches=2, wide=1) and 8 * 64 < got[0]["overflowing"] < 70000


@pytest.mark.parametrize("size,wide,launches", [(256, 0, 1), (257, 3, 3)])
def test_levels_of_exactly_256_and_257_ponds(emu, size, wide, launches):
    got, _ = run(emu, "ladder", size, 3, M, 40 * M)
    assert all(g == dict(g, N=3 * size, levels=3, wide=wide, launches=launches) for g in got)
    assert got[0]["overflowing"] < got[1]["overflowing"] and got[1]["ring"] > 0


def test_narrow_bounds_split_the_same_table_differently(emu):
    for narrow, run_levels in ((8, 65536), (256, 2), (1, 1)):
        got, _ = run(emu, "random", 777, 9, M, narrow=narrow, run_levels=run_levels)
        assert got[0]["N"] == 777 and (got[0]["wide"] > 0) == (narrow < 256)
    got, _ = run(emu, "chain", 300, 2, 200 * M, run_levels=100)
    assert got[0]["launches"] == 3


@pytest.mark.parametrize("over,expected", [(0, "in 0 30 0 out 30 0 0 full 1 1 0 reach 1 2 1"), (1, "in 0 30 1 out 30 1 0 full 1 1 0 reach 1 2 3")])
def test_the_exact_fill_and_one_quantum_more(emu, over, expected):
    _, out = run(emu, "exact", over, 1, 5)
    assert "exact: " + expected in out, out


@pytest.mark.parametrize("kind,size", [("random", 1000), ("hub", 300), ("chain", 130)])
def test_no_runoff_and_the_most_runoff(emu, kind, size):
    got, _ = run(emu, kind, size, 5, 0, TOP)
    assert got[0]["overflowing"] == 0 and got[0]["land"] == 0 and got[1]["overflowing"] > size // 2 and got[1]["land"] > 0


def test_three_reruns_in_non_monotone_order_on_one_state(emu):
    got, _ = run(emu, "random", 5000, 11, M, 100 * M, MM, 10 * M)
    over = [g["overflowing"] for g in got]
    assert over[2] < over[0] < over[3] < over[1]
