"""Build and run the stand-alone host emulations of the pond units (tests/*_emu_main.cpp): each compiles a unit's kernels for the CPU
over tests/hip_emu.h with the address and undefined-behaviour sanitizers on, and runs as a child process of the test - nothing is
loaded into Python, nothing is preloaded."""
import os
import subprocess

from conftest import ROOT

SANITIZER_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]


def build(tmp_path_factory, name):
    """compile tests/<name>_main.cpp into a temporary directory; the program's path"""
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([os.environ.get("CXX", "g++")] + SANITIZER_FLAGS + [os.path.join(ROOT, "tests", name + "_main.cpp"), "-o", exe])
    return exe


def run(exe, *args):
    """the program's stdout, after it has ended with status 0 and no sanitizer report"""
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ERROR" not in p.stderr, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout
