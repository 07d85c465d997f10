"""Kernel LOGIC of the issue resolution without a GPU: gyeeta_amd/csrc/gys_svcresol.hpp (k_resol_seed, k_resol_level, k_resol_settle,
k_resol_finish, k_resol_rows), compiled by g++ against the CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h) and
run by tests/cpp/kemu/test_svcresol.cc against a level-by-level search over std::map written from the definition ("Issue resolution" in
include/gysketch.h).  A stand-alone executable: it runs once plain and once built with -fsanitize=address (every array a kernel writes
is a heap array of its exact size); nothing is loaded into Python.  The -m gpu tests (tests/test_gpu_svcresol.py) remain the check of
the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
BUILDS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}
SRC, OK_LINE = os.path.join(KEMU, "test_svcresol.cc"), "kemu svcresol ok"


@pytest.fixture(scope="module")
def svcresol_runs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kemu_svcresol")
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("svcresol_%s" % name))
        procs[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-ffp-contract=off", "-I" + KEMU] + flags + [SRC, "-o", exe, "-pthread"],
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    builds = {}
    for k, (exe, p) in procs.items():
        log = p.communicate()[0]
        builds[k] = (exe, p.returncode, log)
    runs = {k: subprocess.Popen(["timeout", "-s", "KILL", "900", exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for k, (exe, rc, log) in builds.items() if rc == 0}
    results = {}
    for k, (exe, rc, log) in builds.items():
        if rc != 0:
            results[k] = (-1, "", "build failed:\n" + log[-3000:])
        else:
            so, se = runs[k].communicate()
            results[k] = (runs[k].returncode, so, se)
    return results


@pytest.mark.parametrize("build", list(BUILDS))
def test_svcresol_logic_equals_the_model(svcresol_runs, build):
    rc, so, se = svcresol_runs[build]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and OK_LINE in so, (rc, so[-2000:], se[-2000:])
