"""Kernel LOGIC of the rankings on sketch results without a GPU: gyeeta_amd/csrc/gys_topk.hpp (k_topk_keys, k_topk_ties, k_topk_gather) with the
selection rounds k_svc_hist / k_svc_pick of gys_svcquery.hpp, and k_td_slab_quantiles of gys_tdrank.hpp, compiled by g++ against the CPU
stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h) and run by tests/cpp/kemu/test_topk.cc on the tables of
tests/test_gpu_topk.py and tests/test_gpu_slab_quantiles_dev.py: every answer equals a plain C++ loop of the definition ("Top-k" in
include/gysketch.h; the loop of gys_tdigest_slab_quantiles) bit for bit.  The program is a stand-alone executable: it runs once plain and
once built with -fsanitize=address (the candidate, tie and output lists are heap arrays of their exact sizes; under the sanitizer, where a thread
of the stand-in costs several times as much, without the sizes 4 095 and 4 096 -- 4 097 stays -- and the larger stride / subset / weight table).
The -m gpu tests remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
BUILDS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}


@pytest.fixture(scope="module")
def kemu_topk(tmp_path_factory):
    out = tmp_path_factory.mktemp("kemu_topk")
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("kemu_topk_" + name))
        procs[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-ffp-contract=off", "-I" + KEMU] + flags + [os.path.join(KEMU, "test_topk.cc"), "-o", exe, "-pthread"],
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    builds = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        builds[name] = (exe, p.returncode, log)
    runs = {name: subprocess.Popen(["timeout", "-s", "KILL", "900", exe, "3"] + (["brief"] if BUILDS[name] else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for name, (exe, rc, log) in builds.items() if rc == 0}
    results = {}
    for name, (exe, rc, log) in builds.items():
        if rc != 0:
            results[name] = (-1, "", "build failed:\n" + log[-3000:])
        else:
            so, se = runs[name].communicate()
            results[name] = (runs[name].returncode, so, se)
    return results


@pytest.mark.parametrize("build", list(BUILDS))
def test_topk_and_slab_quantile_kernel_logic_equals_the_definitions(kemu_topk, build):
    rc, so, se = kemu_topk[build]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu topk ok" in so, (rc, so[-2000:], se[-2000:])
