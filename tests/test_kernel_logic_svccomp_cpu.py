"""Kernel LOGIC of the service components without a GPU: gyeeta_amd/csrc/gys_svccomp.hpp (k_cc_init, k_cc_hook, k_cc_flatten, k_cc_sizes,
k_cc_roots, k_cc_rows, k_cc_labels) compiled by g++ against the CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h)
and run by tests/cpp/kemu/test_svccomp.cc against a sequential union-find over the same pair array and a std::map of the figures, written
from the definition ("Service components" in include/gysketch.h).  A workgroup's 256 threads are real threads there, so the hooks of a
launch race as they do on the device; every kernel runs at one workgroup and at several, and the termination counter word must stay 0.
A stand-alone executable: it runs once plain and once built with -fsanitize=address (every array a kernel writes is a heap array of its
exact size, one case names slots at and above the number of services).  The -m gpu tests (tests/test_gpu_svccomp.py) remain the check
of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
SRC = os.path.join(KEMU, "test_svccomp.cc")
BUILDS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}


@pytest.fixture(scope="module")
def svccomp_runs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kemu_svccomp")
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("svccomp_%s" % name))
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
def test_svccomp_logic_equals_the_model(svccomp_runs, build):
    rc, so, se = svccomp_runs[build]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu svccomp ok" in so, (rc, so[-2000:], se[-2000:])
