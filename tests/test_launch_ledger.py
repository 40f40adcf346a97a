"""The launch ledger (include/wdpm.h: wdpm_launch_ledger) is the whole kernel inventory of the build: one entry per kernel
instantiation in the device code of wdpm_march.hip, wdpm_small.hip and wdpm_kernels.hip, named as c++filt names the symbol.
An instantiation the dispatch launches without a ledger line, or a ledger line whose arguments are not those of a kernel in the
build, fails here.  No GPU: the table is filled when the library is loaded, and reading it makes no HIP call."""
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "wdpm_amd", "csrc")
ASM = [os.path.join(CSRC, "build", f) for f in ("wdpm_march.s", "wdpm_small.s", "wdpm_kernels.s")]
SOURCES = [os.path.join(CSRC, f) for f in ("wdpm_iteration.h", "wdpm_march.hip", "wdpm_small.hip", "wdpm_kernels.hip", "wdpm_kernels.h", "wdpm_stencil.h", "wdpm_ledger.h")]


def demangled_kernel_name(sym: str) -> str:
    """"void (anonymous namespace)::relay_iteration_kernel<0, true, false, 8, true>(double const*, ...)" -> "relay_iteration_kernel<0, true, false, 8, true>" """
    s = re.sub(r"^void ", "", sym.strip())
    s = s.replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(s):                      # the parameter list: the first "(" outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def build_kernels():
    """{kernel name: [.s files holding it]} of the built device code; `make check-asm` writes the .s files (about 2 min) where they
    are missing or older than the sources."""
    newest = max(os.path.getmtime(p) for p in SOURCES)
    if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in ASM):
        subprocess.check_call(["make", "-C", CSRC, "check-asm"], env=dict(os.environ, PYTORCH_ROCM_ARCH="gfx950"))
    found = {}
    for path in ASM:
        mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), flags=re.M)
        assert mangled, f"no kernels in {path}"
        names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(names) == len(mangled)
        for n in names:
            found.setdefault(demangled_kernel_name(n), []).append(os.path.basename(path))
    return found


def fresh_ledger():
    """the ledger as a process that has loaded the library and launched nothing sees it"""
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import wdpm_amd; "
            "c, s = wdpm_amd.load_hip().launch_ledger(); print(json.dumps([c, s]))")
    p = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    counts, switches = json.loads(p.stdout.strip().splitlines()[-1])
    return counts, switches


def test_demangled_names_are_cut_at_the_parameter_list():
    assert demangled_kernel_name("void (anonymous namespace)::fused_iteration_kernel<0, false, 2, true, true, false>(double const*, "
                                 "double*, (anonymous namespace)::TileFlags)") == "fused_iteration_kernel<0, false, 2, true, true, false>"
    assert demangled_kernel_name("void pass_kernel<2>(double*, double const*, SlabGeom, int, int, double*)") == "pass_kernel<2>"
    assert demangled_kernel_name("mark_nodata_kernel(double*, unsigned long, double)") == "mark_nodata_kernel"


def test_the_ledger_names_every_kernel_of_the_build_and_nothing_else():
    built = build_kernels()
    counts, _ = fresh_ledger()
    missing = sorted(set(built) - set(counts))
    stray = sorted(set(counts) - set(built))
    assert not missing, f"kernels in the build that no launch counts (a launch without WDPM_LEDGER / WDPM_LEDGER_T?): {missing}"
    assert not stray, f"ledger entries that name no kernel of the build (template arguments not written out in full?): {stray}"
    # no kernel is in two units: the probe and the balance kernels belong to the marching unit, which alone launches them
    twice = {k: v for k, v in built.items() if len(v) != 1}
    assert not twice, f"kernels that more than one .s file holds: {twice}"
    assert built["dpp_probe_kernel"] == ["wdpm_march.s"] and built["xcd_rebalance_kernel"] == ["wdpm_march.s"]


def test_a_fresh_process_has_counted_nothing():
    counts, switches = fresh_ledger()
    assert counts and all(v == 0 for v in counts.values()), {k: v for k, v in counts.items() if v}
    assert all(not v for v in switches.values())


def test_the_oracle_has_an_empty_ledger(oracle):
    assert oracle.launch_ledger() == ({}, {})
