"""The large-key t-digest path of gys_huge.hpp without a GPU, at the inputs that steer it (tests/cpp/kemu/test_huge_edges.cc, built by g++
against the CPU stand-in of the device model like the programs of tests/test_kernel_logic_cpu.py): the table of
tests/test_gpu_huge_edges.py -- run lengths around a chunk and a sweep of the count kernel's vector loop, runs at every residue from a
16-byte boundary, runs of equal values on either side of bin 16 383 | 16 384, tail counts around the capacities of the two merge tiers,
tail values split between buffer and run, every route in one batch, several pool rounds, a full and an overflowing global tail list --
against the oracle's sequential engine, with the path's own list lengths as the witness of the route.  The program's parts run side by
side, each once plain and once as a stand-alone program built with -fsanitize=address (the run area, the bin pool, the tail list and
the lists are heap arrays there).  Under AddressSanitizer the tail-list part runs with a list of 2^16 places (4 + 1 keys): at the
engine's 2^20 (64 + 1 keys of 16 384 tail values: 10^6 events per batch) it takes minutes there; the plain build runs it at 2^20."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
ASAN = ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]

# build -> (defines, extra compiler flags); program -> (build, part)
BUILDS = {"plain": ([], []), "asan": ([], ASAN), "asan-short-tail-list": (["KEMU_TAIL_CAP=65536u"], ASAN)}
PARTS = ["lengths", "values", "tails", "routes", "taillist"]
PROGRAMS = {p: ("plain", p) for p in PARTS}
PROGRAMS.update({p + "-address-sanitizer": ("asan-short-tail-list" if p == "taillist" else "asan", p) for p in PARTS})


@pytest.fixture(scope="module")
def edge_results(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    out = tmp_path_factory.mktemp("kemu_huge_edges")
    odir = os.path.join(ROOT, "oracle")
    builds = {}
    for name, (defs, flags) in BUILDS.items():
        exe = str(out / name)
        builds[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU] + flags + ["-D" + d for d in defs] +
                                              [os.path.join(KEMU, "test_huge_edges.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so", "-Wl,-rpath," + odir, "-pthread"],
                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = {name: (p.communicate()[0], p.returncode) for name, (_, p) in builds.items()}
    runs, results = {}, {}
    for name, (build, part) in PROGRAMS.items():
        if logs[build][1] != 0:
            results[name] = (-1, "", "build failed:\n" + logs[build][0][-3000:])
        else:
            runs[name] = subprocess.Popen(["timeout", "-s", "KILL", "1200", builds[build][0], "4100", part], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in runs.items():
        so, se = p.communicate()
        results[name] = (p.returncode, so, se)
    return results


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_huge_edges_equal_oracle(edge_results, name):
    rc, so, se = edge_results[name]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu huge edges ok" in so, (rc, so[-2000:], se[-2000:])
