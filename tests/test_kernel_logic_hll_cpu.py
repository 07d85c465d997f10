"""Kernel LOGIC of the distinct-count kernels without a GPU: gyeeta_amd/csrc/gys_hllroll.hpp compiled by g++ against the CPU stand-in of
the HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_cpu.py does for the other kernels) and run on synthetic
register files (tests/cpp/kemu/test_hllroll.cc): p = 4, 6, 8, 10; group files equal gyo_hll_merge byte for byte (groups of 0, 1, 3 members
and of one, two and three chunks, with and without member lists), estimates within 1e-12 of gyo_hll_estimate, the all-zero file exactly 0,
and the estimate of a file the same bits through every lane position, grid size and launch shape.  The -m gpu tests
(tests/test_gpu_hll_rollup.py) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_hll(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    exe = str(tmp_path_factory.mktemp("kemu_hll") / "kemu_hll")
    odir = os.path.join(ROOT, "oracle")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, os.path.join(KEMU, "test_hllroll.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                        "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_hll_kernel_logic_equals_oracle(kemu_hll, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_hll, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu hllroll ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
