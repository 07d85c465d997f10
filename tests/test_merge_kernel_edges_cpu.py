"""The value-bin merge kernel k_digest_bins at the edges of its phases, without a GPU: tests/cpp/kemu/test_bins_edges.cc (its own main) built
by g++ against the CPU stand-in of the device model, the recipe of tests/test_kernel_logic_cpu.py.  One workgroup walks a list of 38 entries
back to back -- the list of non-empty bins written by the bin scan with 0 / 1 / 256 / 257 / 1 024 entries, 512 / 513 large values and more than
the list holds, the edge values of the bins, old clusters on both sides of 1 024, folded parts, a staged run, both hand-overs, an empty entry
between two others -- for the instances of 4, 8 and 64 values per thread, after mb_bin was compared with the bit formula for every value
below 2^20.  Every program is built twice: plain, and with -fsanitize=address,undefined (an index outside a __shared__ array or a global
buffer, a shift or conversion out of range, aborts it)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
VPTS = (4, 8, 64)
SANITIZE = {"plain": [], "asan-ubsan": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module")
def edge_results(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    out = tmp_path_factory.mktemp("kemu_edges")
    odir = os.path.join(ROOT, "oracle")
    builds = {}
    for vpt in VPTS:
        for san, flags in SANITIZE.items():
            exe = str(out / ("edges_%d_%s" % (vpt, san)))
            builds[vpt, san] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, "-DKEMU_BINS_VPT=%d" % vpt] + flags +
                                                      [os.path.join(KEMU, "test_bins_edges.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                                                       "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = {k: (exe, p.communicate()[0], p.returncode) for k, (exe, p) in builds.items()}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    runs = {k: subprocess.Popen(["timeout", "-s", "KILL", "600", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
            for k, (exe, _, rc) in logs.items() if rc == 0}
    results = {}
    for k, (exe, log, rc) in logs.items():
        if k in runs:
            so, se = runs[k].communicate()
            results[k] = (runs[k].returncode, so, se)
        else:
            results[k] = (-1, "", "build failed:\n" + log[-3000:])
    return results


@pytest.mark.parametrize("san", list(SANITIZE))
@pytest.mark.parametrize("vpt", VPTS)
def test_merge_kernel_edges_equal_oracle(edge_results, vpt, san):
    rc, so, se = edge_results[vpt, san]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "mb_bin: every value below 2^20" in so and "kemu bins edges ok" in so, (rc, so[-2000:], se[-2000:])
    assert "AddressSanitizer" not in se and "runtime error" not in se, se[-2000:]
