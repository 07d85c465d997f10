"""k_resp_host's listener lookup without a GPU on the key sets of tests/lstkeys.py (tests/cpp/kemu/test_resp_lookup.cc, built by g++ against
the CPU stand-in of the device model like the programs of tests/test_kernel_logic_cpu.py): runs that wrap around the end of a 16-, 64- and
4096-entry sub-table (the copy of entry 0 behind the last entry, the wrap of the third-and-later probe walk), long runs, misses that walk
them, keys that agree with a stored entry in one 32-bit half of the packed compare, the all-ones key -- the key bits of a free entry --
registered and not, a host in two parts, keys with candidates among the displaced entries and tables rebuilt after a delete must give
what the oracle's sequential engine gives on the same bytes.  The program is also built as a stand-alone program with -fsanitize=address: an event resolved to a local index the host
does not have indexes the per-key areas out of bounds there, not on a GPU.  Nothing is loaded into Python.
Both builds and both runs together take about 17 s (measured; the sanitizer run itself under 2 s)."""
import os
import subprocess

import pytest

from tests import lstkeys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")

# name -> extra compiler flags
PROGRAMS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}


@pytest.fixture(scope="module")
def lookup_results(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    out = tmp_path_factory.mktemp("kemu_lookup")
    odir = os.path.join(ROOT, "oracle")
    worlds = lstkeys.standin_worlds()
    lstkeys.write_standin(str(out / "worlds.txt"), worlds)
    builds = {}
    for name, flags in PROGRAMS.items():
        exe = str(out / name)
        builds[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU] + flags +
                                              [os.path.join(KEMU, "test_resp_lookup.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so", "-Wl,-rpath," + odir, "-pthread"],
                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    runs, results = {}, {}
    for name, (exe, p) in builds.items():
        log = p.communicate()[0]
        if p.returncode != 0:
            results[name] = (-1, "", "build failed:\n" + log[-3000:])
        else:
            runs[name] = subprocess.Popen(["timeout", "-s", "KILL", "1200", exe, str(out / "worlds.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in runs.items():
        so, se = p.communicate()
        results[name] = (p.returncode, so, se)
    return results, len(worlds)


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_resp_lookup_scenarios_equal_oracle(lookup_results, name):
    results, nworlds = lookup_results
    rc, so, se = results[name]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu resp lookup ok (%d worlds" % nworlds in so, (rc, so[-2000:], se[-2000:])


def test_every_scenario_is_in_a_world():
    """the launches cover every host and every step with events of every scenario (H, keys with candidates, under the MODE 1 instance; its IPv6 form is the GPU's)"""
    seen = {(id(h), id(st)) for w in lstkeys.standin_worlds() for h, st in w.hosts}
    for name in lstkeys.BUILDERS:
        for h in lstkeys.scenario(name).hosts:
            for st in h.steps:
                assert st.events is None or (id(h), id(st)) in seen, (name, h.name)
