"""Kernel LOGIC of the service dependency graph without a GPU: gyeeta_amd/csrc/gys_svcdeps.hpp (k_dep_edges, k_dep_seed, k_dep_level,
k_dep_collect) compiled by g++ against the CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h) and run by
tests/cpp/kemu/test_svcdeps.cc against a std::map of edges and a deque BFS written from the definition ("Service dependency graph" in
include/gysketch.h); and the pure host builder of the task -> services list (gyeeta_amd/csrc/gys_svcdeps_host.hpp) run by
tests/cpp/test_svcdeps_host.cc on empty input, id 0, equal ids and a task of 70 slots.  Both are stand-alone executables: each runs once
plain and once built with -fsanitize=address (every array a kernel writes is a heap array of its exact size).  The -m gpu tests
(tests/test_gpu_svcdeps.py) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
BUILDS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}
PROGRAMS = {"kernels": (os.path.join(KEMU, "test_svcdeps.cc"), "kemu svcdeps ok"),
            "host-builder": (os.path.join(ROOT, "tests", "cpp", "test_svcdeps_host.cc"), "svcdeps host ok")}


@pytest.fixture(scope="module")
def svcdeps_runs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kemu_svcdeps")
    procs = {}
    for prog, (src, _) in PROGRAMS.items():
        for name, flags in BUILDS.items():
            exe = str(out / ("svcdeps_%s_%s" % (prog, name)))
            procs[prog, name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-ffp-contract=off", "-I" + KEMU] + flags + [src, "-o", exe, "-pthread"],
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
@pytest.mark.parametrize("prog", list(PROGRAMS))
def test_svcdeps_logic_equals_the_model(svcdeps_runs, prog, build):
    rc, so, se = svcdeps_runs[prog, build]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and PROGRAMS[prog][1] in so, (rc, so[-2000:], se[-2000:])
