"""Kernel LOGIC of the distinct-count LEVEL kernels without a GPU: k_hll_level_roll and k_hll_level_view of gyeeta_amd/csrc/gys_hllroll.hpp
compiled by g++ against the CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_hll_cpu.py does
for the open-window kernels) and driven through 64 window closes (tests/cpp/kemu/test_hlllevels.cc): p = 4, 6, 8, 10; 1, 63, 64, 65 and 1000
services; every level file equals the ring model of the definition and the closed-form union of the member windows byte for byte, estimates
within 1e-12 of gyo_hll_estimate and exactly 0 for the all-zero file.  The -m gpu tests (tests/test_gpu_hll_levels.py) remain the check of
the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_hll_levels(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    exe = str(tmp_path_factory.mktemp("kemu_hll_levels") / "kemu_hll_levels")
    odir = os.path.join(ROOT, "oracle")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, os.path.join(KEMU, "test_hlllevels.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                        "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1])  # (about two minutes: the stand-in starts 256 host threads per workgroup and launch)
def test_hll_level_kernel_logic_equals_models(kemu_hll_levels, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "900", kemu_hll_levels, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu hlllevels ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
