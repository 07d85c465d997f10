"""The value-bin merge kernel k_digest_bins at the bounds that decide what a round of 256 values has to test, and at the shapes of its
large-value list, without a GPU: tests/cpp/kemu/test_bins_rounds.cc (its own main) built by g++ against the CPU stand-in of the device model,
the recipe of tests/test_merge_kernel_edges_cpu.py.  One workgroup walks ~140 entries back to back: each of nh, max(nh, nw), ent.nbuf and m at
0, 1, 255, 256, 257, 511, 512, 513, the last round's first element, the last element and one past it while the other three sit on round
boundaries, all four in one round, with and without a staged run, with nothing folded and with a folded part; then 0 ... 1 024 large values
and one more than the list holds, one cell full of one value / of distinct values, every cell once, the cells' first and last values, old
clusters whose thresholds lie in an occupied cell, in an empty one between two occupied ones and exactly on a large value.  For the instances
of 4, 8 and 64 values per thread; every program is built twice: plain, and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
VPTS = (4, 8, 64)
SANITIZE = {"plain": [], "asan-ubsan": ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module")
def round_results(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    out = tmp_path_factory.mktemp("kemu_rounds")
    odir = os.path.join(ROOT, "oracle")
    builds = {}
    for vpt in VPTS:
        for san, flags in SANITIZE.items():
            exe = str(out / ("rounds_%d_%s" % (vpt, san)))
            builds[vpt, san] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, "-DKEMU_BINS_VPT=%d" % vpt] + flags +
                                                      [os.path.join(KEMU, "test_bins_rounds.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
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
def test_merge_kernel_rounds_equal_oracle(round_results, vpt, san):
    rc, so, se = round_results[vpt, san]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu bins rounds ok" in so, (rc, so[-2000:], se[-2000:])
    assert "AddressSanitizer" not in se and "runtime error" not in se, se[-2000:]
