"""What the launch planner decides (wdpm_amd/csrc/wdpm_dispatch.h::plan_iteration), threshold by threshold, without a GPU.

A host-only program (tests/dispatch_plans_main.cpp, built by wdpm_amd/csrc/Makefile with the host compiler) runs the fixed sweep of
tests/dispatch_sweep.h through the planner under every switch profile and prints one row per request: the request, the kernel
family and template arguments chosen, and every geometry field of the plan.  tests/golden/dispatch_plans.json.gz holds those rows as
the commit named in its header decided them - recorded from THAT commit's host dispatch, compiled unmodified against a stub of the
HIP calls it makes, not from the planner (the header says how, and which device facts were used).  The parity suites are bit-exact
whatever the dispatch picks; this is the test in which a `<=` that becomes `<`, a chunk height off by a triple, a lost LDS pad or
a two-waves-per-SIMD decision that flips at another size shows up, as the first differing row.

The sweep takes every source-level condition of the planner both ways (g++ --coverage, gcov -b; the one exception is
wdpm_find_variant's "not in the list", which the second test forbids).

A deliberate retune changes rows on purpose: `python tests/test_dispatch_plans.py --regenerate` rewrites the fixture's rows from the
planner (the header keeps naming the commit of the original recording), and the diff of the readable table -
`zcat tests/golden/dispatch_plans.json.gz` - is what the reviewer of that retune reads."""
import gzip
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wdpm_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_plans.json.gz")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_and_run(objdir):
    """the Makefile's recipe with its outputs in objdir (the tree is not written to); returns (exit status, {profile: rows})"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "dispatch_plans", f"OBJ={objdir}"])
    run = subprocess.run([os.path.join(str(objdir), "dispatch_plans")], capture_output=True, text=True)
    profiles, cur = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("# profile "):
            cur = profiles.setdefault(line[len("# profile "):], [])
        else:
            cur.append(line)
    return run.returncode, run.stderr, profiles


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("dispatch_plans"))


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def test_every_plan_is_the_recorded_one(planned, recorded):
    _, _, profiles = planned
    assert list(profiles) == list(recorded["profiles"]), "the switch profiles of tests/dispatch_sweep.h and of the fixture differ"
    for name, rows in profiles.items():
        want = recorded["profiles"][name]
        for i, (got, exp) in enumerate(zip(rows, want)):
            assert got == exp, f"profile {name}, row {i}: the planner decides\n  {got}\nrecorded from {recorded['recorded_from'][:7]}\n  {exp}"
        assert len(rows) == len(want), f"profile {name}: {len(rows)} rows planned, {len(want)} recorded"
    assert sum(len(r) for r in profiles.values()) > 50000


def variant_lists():
    """the instantiation lists of wdpm_dispatch.h, as the text says them: {family: set of argument tuples}"""
    text = open(os.path.join(CSRC, "wdpm_dispatch.h")).read()
    out = {}
    for family, macro in (("marching", "WDPM_VARIANTS_MARCHING"), ("relay", "WDPM_VARIANTS_RELAY"), ("triangle", "WDPM_VARIANTS_TRIANGLE")):
        body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*\n)", text).group(1)
        rows = [tuple({"true": 1, "false": 0}.get(a.strip(), a.strip()) for a in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body)]
        out[family] = [tuple(int(a) for a in r) for r in rows]
    return out


def test_every_planned_instantiation_is_in_its_family_list(planned):
    status, stderr, profiles = planned
    assert status == 0, stderr[:2000]                      # the program looks every plan up in the lists as compiled
    lists = variant_lists()
    assert {k: len(v) for k, v in lists.items()} == {"marching": 26, "relay": 15, "triangle": 11}
    assert all(len(set(v)) == len(v) for v in lists.values())
    seen = {k: set() for k in lists}
    for rows in profiles.values():
        for row in rows:
            m = re.search(r"-> (\w+)<([\d,]+)>", row)
            if m:
                seen[m.group(1)].add(tuple(int(a) for a in m.group(2).split(",")))
    for family, tuples in seen.items():
        assert tuples <= set(lists[family]), (family, sorted(tuples - set(lists[family])))
        assert tuples == set(lists[family]), f"{family}: the sweep never plans {sorted(set(lists[family]) - tuples)}"


def test_slot_filling_geometry_is_what_test_balance_pairing_restates(planned):
    """tests/test_balance_pairing.py::launch_geometry restates in Python how many chunks a strip is cut into when the balance table
    fills every resident slot; here it is held against the planner for the shapes that test uses (steady launches, balance mode 1)"""
    from test_balance_pairing import launch_geometry
    _, _, profiles = planned
    shapes = [(1055, 8192), (2051, 16386), (4098, 4098), (8194, 8194), (16386, 16386), (3002, 3002)]
    filled = set()
    for rows, ncp in shapes:
        for module in (0, 2):
            key = f"m={module} {rows}x{ncp} w=0:{rows - 1} ch=0 z=0 fl=0 md=0 wp=1 db=1 lc=0 dem=2 frc=0 t=0 tc=0 b=1 bc=16384 -> "
            (row,) = [r for r in profiles["default"] if r.startswith(key)]
            f = dict(kv.split("=") for kv in row[len(key):].split()[1:])
            assert row[len(key):].startswith("marching<") and f["table"] == "1"
            H, nchunks = int(f["H"]), int(f["nchunks"])
            # (on the three shapes where equal heights of H rows fill the slots already, the two counts coincide)
            assert (int(f["nstrips"]), nchunks) == launch_geometry(rows, ncp)[:2], row
            if nchunks != (rows - 2 + H - 1) // H:             # not the equal heights of H rows: the slot-filling path
                assert f["pair"] == "1"
                filled.add((rows, ncp))
            if (rows, ncp, module) == (1055, 8192, 2):         # the drain slab of an 8-GPU run
                assert (int(f["nstrips"]), nchunks, H) == (48, 42, 27)
    assert filled == {(1055, 8192), (4098, 4098), (3002, 3002)}


def regenerate():
    import tempfile
    with gzip.open(FIXTURE, "rt") as f:
        doc = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        status, stderr, profiles = build_and_run(d)
    assert status == 0, stderr
    doc["profiles"] = profiles
    with open(FIXTURE, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=9, mtime=0, filename="") as g:
        g.write(json.dumps(doc, indent=0).encode())
    print(f"{FIXTURE}: {sum(len(r) for r in profiles.values())} rows, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["--regenerate"]:
        regenerate()
    else:
        sys.exit("usage: python tests/test_dispatch_plans.py --regenerate")
