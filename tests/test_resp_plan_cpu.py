"""The plan of a response batch without a GPU: gyeeta_amd/csrc/gys_resp_plan.hpp (pure host functions: which front end a batch takes, which
tile form the event kernel runs in, the virtual segments of the split / many-listener forms) compiled by g++ with AddressSanitizer and
UBSan into a stand-alone program (tests/cpp/test_resp_plan.cc, over the CPU stand-in of the HIP device model, tests/cpp/kemu, as
tests/test_groups_cpu.py) and checked against the rules' plain statements over seeded random segment lists.  Nothing is loaded into Python.
The -m gpu tests (tests/test_gpu_resp.py and the bit-exact files of the later rounds) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resp_plan") / "test_resp_plan")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + KEMU,
                        os.path.join(ROOT, "tests", "cpp", "test_resp_plan.cc"), "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_resp_plan_equals_plain_rules(plan_exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "300", plan_exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "resp plan ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
