"""Every kernel instantiation of the build, and every state of the switches the host hands the marching and relay kernels, runs in
a case that is compared bit for bit with the CPU oracle - and the launch ledger (include/wdpm.h: wdpm_launch_ledger) proves it ran.

The parity suites pass the same way whether or not the variant they were written for was chosen: which one runs is decided at run
time from sizes, water kinds, DEM checks, the launch's place in a block and the WDPM_* switches.  Here each case is a small table
row (module, shape, chunk height, DEM level, water kind, call script) that declares the ledger entries and switch states it hits;
tests/coverage_worker.py plays it on the HIP library and on the oracle in a child process per environment profile (the switches
are read once per process) and reports what the case added to the ledger.  A case fails when any observation differs from the
oracle or when a dispatch change sends it elsewhere; the union of all cases must cover the whole ledger.

The forced-variant suites (tests/test_forced_variants.py) assume that their switches still take effect: one small case under each
of their environments must show the forced family in the ledger and none of the ones it excludes.

Writes kernel_coverage.json (per entry, its launches and the cases that hit it) to $WDPM_REPORT_DIR, by default build/reports."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

F, T = False, True
MARCH, RELAY, TRI = "fused_iteration_kernel", "relay_iteration_kernel", "tri_iteration_kernel"


def fused(module, szs, dem32, flush=F, md=F, plain=F):
    return f"{MARCH}<{module}, {str(szs).lower()}, {dem32}, {str(flush).lower()}, {str(md).lower()}, {str(plain).lower()}>"


def relay(module, flush, plain, nw, dem32=F):
    return f"{RELAY}<{module}, {str(flush).lower()}, {str(plain).lower()}, {nw}, {str(dem32).lower()}>"


def tri(module, flush, k=1, plain=F, md=F):
    return f"{TRI}<{module}, {str(flush).lower()}, {k}, {str(plain).lower()}, {str(md).lower()}>"


LEVEL = {"fp64": 0, "codes32": 1, "codes16": 2}
# a block of one iteration (flush and max change in one launch), a block of four (flush, two plain, max change), then the water
# with negative depths iterated without a block (no flush, no max change, gated)
SCRIPT = [("block", 1), ("block", 4), ("negative",), ("iter", 3)]
SCRIPT_DRAIN = [("block", 1), ("block", 4), ("negative",), ("iter", 3), ("max_diff",)]

PROFILES = {
    "default": {},
    "relay-nw8": dict(WDPM_RELAY_NW="8"),
    "triangle": dict(WDPM_RELAY="0"),
    "triangle-k2": dict(WDPM_RELAY="0", WDPM_TRI_K="2"),
    "balance": dict(WDPM_BALANCE="2"),
}

# name -> spec; "hits": ledger entries the case must add to; "sw": (family, bit, state) the case must show in some launch
CASES = {}
for lv in LEVEL:
    d = LEVEL[lv]
    # the marching kernel (a chunk height of the caller's keeps every launch on it): 301 rows (R % 3 == 1), 520 columns (4 strips,
    # the last one partial), chunks of 24 rows
    CASES[f"march-add-{lv}"] = dict(profile="default", module="add", shape=(301, 520), chunk=24, level=lv, script=SCRIPT,
                                    hits=[fused(0, F, d, T, T), fused(0, F, d, T), fused(0, F, d, plain=T), fused(0, F, d, md=T),
                                          fused(0, F, d)],
                                    sw=[(MARCH, "TILE_FLAGS", 1), (MARCH, "TILE_FLAGS", 0), (MARCH, "NO_CLAMP", 0), (MARCH, "PRIO", 0),
                                        (MARCH, "BALANCE", 0)])
    CASES[f"march-drain-{lv}"] = dict(profile="default", module="drain", shape=(200, 350), chunk=12, level=lv, script=SCRIPT_DRAIN,
                                      hits=[fused(2, F, d, T), fused(2, F, d, plain=T), fused(2, F, d), "max_diff_kernel",
                                            "seqsum_a_kernel"])
CASES["march-add-codes16"]["hits"] += ["mark_nodata_kernel", "dem_min_kernel", "dem_encode_kernel", "dem16_encode_kernel", "scan_water_kernel"]
CASES.update({
    "march-add-negzero": dict(profile="default", module="add", shape=(179, 178), chunk=12, level="fp64", water="negzero",
                              script=[("block", 3), ("iter", 2)], hits=[fused(0, T, 0), "flush_snapshot_kernel", "max_diff_kernel"]),
    "march-drain-negzero": dict(profile="default", module="drain", shape=(95, 350), chunk=6, level="fp64", water="negzero",
                                script=[("block", 3)], hits=[fused(2, T, 0), "flush_snapshot_kernel", "max_diff_kernel"]),
    "march-add-unclamped": dict(profile="default", module="add", shape=(121, 350), chunk=12, level="fp64", dem="huge", water="nodata",
                                script=[("block", 4)], hits=[fused(0, F, 0, T)], sw=[(MARCH, "NO_CLAMP", 1)]),
    # two waves per SIMD (eight-wave workgroups, issue priorities): a drain launch of this size fills every slot twice (rows x strips
    # >= 12 x the resident waves: 2402 x 12 against 12 x 2048 on 256 CUs; 2000^2 falls just short)
    "march-drain-two-waves": dict(profile="default", module="drain", shape=(2400, 2000), chunk=12, level="codes32", force=False,
                                  script=[("block", 3)], hits=[fused(2, F, 1, T), fused(2, F, 1, plain=T)], sw=[(MARCH, "PRIO", 1)]),
    # the relay kernel, four-wave workgroups (small rasters)
    "relay-add": dict(profile="default", module="add", shape=(121, 178), level="codes32", force=False, script=SCRIPT,
                      hits=[relay(0, T, F, 4), relay(0, F, T, 4), relay(0, F, F, 4), tri(0, T, md=T), tri(0, F, md=T)],
                      sw=[(RELAY, "ORDINARY_STORES", 0), (RELAY, "PRIO", 0), (RELAY, "NO_CLAMP", 0)]),
    "relay-drain": dict(profile="default", module="drain", shape=(151, 350), level="codes32", force=False, script=SCRIPT_DRAIN,
                        hits=[relay(2, T, F, 4), relay(2, F, T, 4), relay(2, F, F, 4)]),
    "relay-add-unclamped": dict(profile="default", module="add", shape=(100, 178), level="fp64", dem="huge", script=[("block", 3)],
                                hits=[relay(0, T, F, 4)], sw=[(RELAY, "NO_CLAMP", 1)]),
    # more workgroups than CUs, one round: stage priorities
    "relay-add-stage-priorities": dict(profile="default", module="add", shape=(500, 520), level="codes32", force=False,
                                       script=[("block", 3)], hits=[relay(0, T, F, 4)], sw=[(RELAY, "PRIO", 1)]),
    # about 2000^2 wet, no dry-tile flags: eight-wave workgroups in six rounds, ordinary stores, the DEM as codes
    "relay-add-ordinary-stores": dict(profile="default", module="add", shape=(2000, 2000), level="codes32", force=False, tiles=0,
                                      script=[("block", 3)], hits=[relay(0, T, F, 8, T), relay(0, F, T, 8, T)],
                                      sw=[(RELAY, "ORDINARY_STORES", 1)]),
    # a long block: the steady launches are captured into a HIP graph (counted once, when captured) and replayed
    "relay-add-graph": dict(profile="default", module="add", shape=(120, 350), level="codes32", force=False, script=[("block", 40)],
                            hits=[relay(0, F, T, 4)]),
    "overlapped-add": dict(profile="default", module="add", shape=(302, 350), level="codes32", force=False,
                           script=[("overlap", 3, 30, 30), ("overlap", 1, 30, 30)], hits=[]),
    "pass-add": dict(profile="default", module="add", shape=(95, 178), kernel=1, level="fp64", script=[("block", 1), ("block", 2)],
                     hits=["pass_kernel<0>", "flush_snapshot_kernel", "max_diff_kernel"]),
    "pass-drain": dict(profile="default", module="drain", shape=(95, 178), kernel=1, level="fp64", script=[("block", 2)],
                       hits=["pass_kernel<2>", "drain_outlet_kernel", "flush_snapshot_kernel", "max_diff_kernel"]),
    "setup-and-statistics": dict(profile="default", module="add", shape=(101, 350), level="codes32", force=False, unpadded=True,
                                 script=[("block", 2)], hits=["pad_setup_kernel", "count_stats_kernel", "drain_min_kernel",
                                                              "drain_first_kernel", "unpad_kernel"]),
})
for lv in ("fp64", "codes32"):
    CASES[f"relay8-add-{lv}"] = dict(profile="relay-nw8", module="add", shape=(121, 520), level=lv, script=SCRIPT,
                                     hits=[relay(0, T, F, 8, lv != "fp64"), relay(0, F, T, 8, lv != "fp64"), relay(0, F, F, 8, lv != "fp64")])
CASES.update({
    "relay8-drain": dict(profile="relay-nw8", module="drain", shape=(151, 350), level="codes32", script=SCRIPT_DRAIN,
                         hits=[relay(2, T, F, 8), relay(2, F, T, 8), relay(2, F, F, 8)]),
    "tri-add": dict(profile="triangle", module="add", shape=(100, 350), level="codes32", force=False, script=SCRIPT,
                    hits=[tri(0, T, md=T), tri(0, T), tri(0, F, plain=T), tri(0, F, md=T), tri(0, F)]),
    "tri-drain": dict(profile="triangle", module="drain", shape=(121, 178), level="codes32", force=False, script=SCRIPT_DRAIN,
                      hits=[tri(2, T), tri(2, F, plain=T), tri(2, F)]),
    "tri-k2-add": dict(profile="triangle-k2", module="add", shape=(200, 520), level="codes32", force=False, script=SCRIPT,
                       hits=[tri(0, T, 2), tri(0, F, 2, plain=T), tri(0, F, 2)]),
    "balance-add": dict(profile="balance", module="add", shape=(301, 520), chunk=6, level="codes32", force=False,
                        script=[("block", 8)], hits=["xcd_rebalance_kernel"], sw=[(MARCH, "BALANCE", 1)]),
})

# a case the forced-variant profiles run: small, add, every place in a block
GUARD_CASE = dict(module="add", shape=(121, 350), level="codes32", force=False, script=SCRIPT)

SWITCH_BITS = {MARCH: {"NO_CLAMP": 1, "PRIO": 2, "TILE_FLAGS": 4, "BALANCE": 8},
               RELAY: {"ORDINARY_STORES": 1, "PRIO": 2, "NO_CLAMP": 4}}
# entries no case can reach, with the reason (it should stay empty)
EXEMPT = {}


def family_of(name):
    return name.split("<")[0]


def run_children(jobs, timeout=600):
    """jobs: {label: (env, [case names])} -> {label: {case: result}}; the children run one after the other"""
    out = {}
    for label, (env, names) in jobs.items():
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coverage_worker.py"), *names], cwd=ROOT,
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0, f"{label} {env}: exit status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
        out[label] = json.loads(p.stdout.strip().splitlines()[-1])
        missing = [n for n in names if n not in out[label]]
        assert not missing, f"{label}: no result for {missing}\n{p.stderr[-3000:]}"
    return out


def switch_states(sw_delta, family):
    """{bit name: set of states seen} over the launches of one family"""
    seen = {b: set() for b in SWITCH_BITS[family]}
    for name, states in sw_delta.items():
        if family_of(name) != family:
            continue
        for bits in states:
            for b, mask in SWITCH_BITS[family].items():
                seen[b].add(1 if int(bits) & mask else 0)
    return seen


@pytest.mark.gpu
def test_every_kernel_instantiation_runs_and_matches_the_oracle(hip):
    jobs = {p: (env, [n for n, c in CASES.items() if c["profile"] == p]) for p, env in PROFILES.items()}
    results = run_children(jobs)
    failures, report = [], {}
    for label, res in results.items():
        for case, r in res.items():
            spec = CASES[case]
            if not r["ok"]:
                failures.append(f"{case} [{label}]: {r['error']}")
                continue
            missing = [h for h in spec["hits"] if not r["delta"].get(h)]
            for fam, bit, state in spec.get("sw", []):
                if state not in switch_states(r["switches"], fam)[bit]:
                    missing.append(f"{fam} {bit}={state}")
            if missing:
                failures.append(f"{case} [{label}]: declared but not launched: {missing}; it launched {sorted(r['delta'])}")
            for name, n in r["delta"].items():
                e = report.setdefault(name, {"launches": 0, "cases": [], "switch_states": {}})
                e["launches"] += n
                e["cases"].append(case)
                for bits, k in r["switches"].get(name, {}).items():
                    e["switch_states"][bits] = e["switch_states"].get(bits, 0) + k
    counts, _ = hip.launch_ledger()
    all_sw = {name: e["switch_states"] for name, e in report.items()}
    uncovered = sorted(n for n in counts if n not in report and n not in EXEMPT)
    sw_uncovered = [f"{fam} {bit}={s}" for fam in SWITCH_BITS for bit, seen in switch_states(all_sw, fam).items() for s in (0, 1)
                    if s not in seen]
    report_dir = os.environ.get("WDPM_REPORT_DIR") or os.path.join(ROOT, "build", "reports")
    os.makedirs(report_dir, exist_ok=True)
    with open(os.path.join(report_dir, "kernel_coverage.json"), "w") as f:
        json.dump(dict(entries={n: report.get(n, {"launches": 0, "cases": [], "switch_states": {}}) for n in sorted(counts)},
                       uncovered=uncovered, switch_states_uncovered=sw_uncovered, exempt=EXEMPT, failures=failures), f, indent=1)
    assert not failures, "\n".join(failures)
    assert not uncovered, f"ledger entries no case launched: {uncovered}"
    assert not sw_uncovered, f"switch states no launch showed: {sw_uncovered}"
    assert all(reason for reason in EXEMPT.values())


def forced_expectations():
    """per VARIANTS entry of the forced-variant suites: (families that must launch, entries or families that must not)"""
    from test_forced_variants import VARIANTS
    exp = {}
    for name, env in VARIANTS.items():
        must, must_not = [], []
        if env.get("WDPM_RELAY") == "0" and env.get("WDPM_TRI") == "0":
            must, must_not = [MARCH], [RELAY, TRI]
        elif env.get("WDPM_RELAY") == "2":
            nw = env.get("WDPM_RELAY_NW", "0")
            must = [f"{RELAY} NW={nw}"]
            must_not = [f"{RELAY} NW={4 if nw == '8' else 8}"]
        elif env.get("WDPM_TRI") == "2":
            k = env.get("WDPM_TRI_K", "0")
            must, must_not = [f"{TRI} K={k}", ], [RELAY, f"{TRI} K={2 if k == '1' else 1}"]
        elif env.get("WDPM_PLAIN") == "0":
            must, must_not = ["gated"], ["plain"]
        exp[name] = (env, must, must_not)
    return exp


def matches(name, what):
    fam = family_of(name)
    args = [a.strip() for a in name[len(fam) + 1:-1].split(",")] if "<" in name else []
    if what in (MARCH, RELAY, TRI):
        return fam == what
    if what.startswith(f"{RELAY} NW="):
        return fam == RELAY and args[3] == what.split("=")[1]
    if what.startswith(f"{TRI} K="):
        return fam == TRI and args[2] == what.split("=")[1]
    plain = (fam == MARCH and args[5] == "true") or (fam in (RELAY, TRI) and args[2 if fam == RELAY else 3] == "true")
    if what == "plain":
        return plain
    if what == "gated":
        return fam in (MARCH, RELAY, TRI) and not plain
    raise ValueError(what)


@pytest.mark.gpu
def test_the_forced_variant_switches_still_take_effect():
    exp = forced_expectations()
    jobs = {name: (env, ["guard"]) for name, (env, _, _) in exp.items()}
    results = run_children(jobs)
    failures = []
    for name, (env, must, must_not) in exp.items():
        r = results[name]["guard"]
        if not r["ok"]:
            failures.append(f"{name} {env}: {r['error']}")
            continue
        launched = sorted(r["delta"])
        for what in must:
            if not any(matches(n, what) for n in launched):
                failures.append(f"{name} {env}: no {what} launch; launched {launched}")
        for what in must_not:
            bad = [n for n in launched if matches(n, what)]
            if bad:
                failures.append(f"{name} {env}: {what} launches {bad}")
    assert not failures, "\n".join(failures)
