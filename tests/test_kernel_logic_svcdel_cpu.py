"""Kernel LOGIC of the listener-deletion kernels without a GPU: gyeeta_amd/csrc/gys_svcdel.hpp compiled by g++ against the CPU stand-in of
the HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_histroll_cpu.py does for the group histograms) and run by
tests/cpp/kemu/test_svcdel.cc: backward-shift erase and the insert with explicit values on a 64-entry table against std::unordered_map over
10 000 random steps (plus a probe run of colliding keys erased from its middle, head and tail, and one that wraps round the table's end),
the stale scan on 5 000 kept records against a plain loop (both flags, caps below and above the hit count), and the per-slot clear on
segments of every size class.  The -m gpu tests (tests/test_gpu_listener_delete.py) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_svcdel(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kemu_svcdel") / "kemu_svcdel")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, "-I" + os.path.join(ROOT, "include"), os.path.join(KEMU, "test_svcdel.cc"), "-o", exe,
                        "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_svcdel_kernel_logic(kemu_svcdel, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_svcdel, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu svcdel ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
