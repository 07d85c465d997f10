"""k_resp_host without a GPU at the segment lengths around a slot, a group and a tile of each tile form (tests/cpp/kemu/test_resp_edges.cc,
built by g++ against the CPU stand-in of the device model like the programs of tests/test_kernel_logic_cpu.py): the packed last group
and the waves that leave the group loop early must give what the oracle's sequential engine gives on the same bytes.  The 16 384-event form is also built as a stand-alone program with -fsanitize=address: the event buffer
holds exactly the batch's events, so a load at or past byte 24 n is a heap overflow there, not on a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")

# name -> (defines, extra compiler flags)
PROGRAMS = {
    "tiles-16384": (["KEMU_TPT=16"], []),
    "tiles-6144": (["KEMU_TPT=12"], []),
    "tiles-8192": (["KEMU_TPT=8"], []),
    "tiles-16384-address-sanitizer": (["KEMU_TPT=16"], ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]),
}


@pytest.fixture(scope="module")
def edge_results(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    out = tmp_path_factory.mktemp("kemu_edges")
    odir = os.path.join(ROOT, "oracle")
    builds = {}
    for name, (defs, flags) in PROGRAMS.items():
        exe = str(out / name)
        builds[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU] + flags + ["-D" + d for d in defs] +
                                              [os.path.join(KEMU, "test_resp_edges.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so", "-Wl,-rpath," + odir, "-pthread"],
                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    runs, results = {}, {}
    for name, (exe, p) in builds.items():
        log = p.communicate()[0]
        if p.returncode != 0:
            results[name] = (-1, "", "build failed:\n" + log[-3000:])
        else:
            runs[name] = subprocess.Popen(["timeout", "-s", "KILL", "1200", exe, "5151"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in runs.items():
        so, se = p.communicate()
        results[name] = (p.returncode, so, se)
    return results


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_resp_edge_lengths_equal_oracle(edge_results, name):
    rc, so, se = edge_results[name]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu resp edges ok" in so, (rc, so[-2000:], se[-2000:])
