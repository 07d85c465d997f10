"""The host mirror of the listener registry without a GPU: gyeeta_amd/csrc/gys_hostlst.hpp (pure host code: per-host sub-tables, the cut of
a many-listener host into parts, chains of bound-address listeners, the overflow fallback, the dirty / rebuild protocol) compiled by g++
with AddressSanitizer and UBSan into a stand-alone program (tests/cpp/test_hostlst.cc, over the CPU stand-in of the HIP device model,
tests/cpp/kemu, as tests/test_resp_plan_cpu.py) and checked against the plain statement of the reference's insert-or-replace / first-match
rule over named edge cases and seeded random sequences of registrations and deletions.  Nothing is loaded into Python.
The -m gpu tests (tests/test_gpu_listener_delete.py, tests/test_gpu_round3.py) remain the check of the device copy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def hostlst_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostlst") / "test_hostlst")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + KEMU,
                        os.path.join(ROOT, "tests", "cpp", "test_hostlst.cc"), "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_host_listeners_equal_plain_rules(hostlst_exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "300", hostlst_exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "host listeners ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
