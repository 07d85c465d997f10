"""The group-list builders of the roll-ups without a GPU: gyeeta_amd/csrc/gys_groups.hpp (pure host functions: which members a group has,
how its members are cut into chunks, which chunks belong to a group) compiled by g++ with AddressSanitizer and UBSan into a stand-alone
program (tests/cpp/test_groups.cc; RollupChunk comes from gys_rollup.hpp over the CPU stand-in of the HIP device model, tests/cpp/kemu, as in
tests/test_kernel_logic_histroll_cpu.py) and checked against the builders' plain definitions over seeded random inputs.  Nothing is loaded
into Python.  The -m gpu tests (tests/test_gpu_registry_generation.py and the bit-exact roll-up files) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def groups_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("groups") / "test_groups")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + KEMU,
                        os.path.join(ROOT, "tests", "cpp", "test_groups.cc"), "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_group_builders_equal_plain_definitions(groups_exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "300", groups_exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "kemu groups ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
