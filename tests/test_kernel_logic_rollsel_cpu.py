"""Kernel LOGIC of the selection kernels of the filtered roll-ups without a GPU: gyeeta_amd/csrc/gys_rollsel.hpp compiled by g++ against the
CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_hll_cpu.py does for the distinct-count
kernels) and run on synthetic state records (tests/cpp/kemu/test_rollsel.cc): rows, member sets per row, chunk lists and totals equal a
plain loop over the oracle's criteria walk plus the grouping -- all four group_by values with and without GYS_RF_ANY_STATE, an empty result,
groups of several chunks, maxrows below the number of rows, a label domain larger than a workgroup's LDS table, several grid sizes -- and the
chunk lists fed to k_hll_union give gyo_hll_merge of the members byte for byte.  The -m gpu tests (tests/test_gpu_rollup_filtered.py)
remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_rollsel(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    exe = str(tmp_path_factory.mktemp("kemu_rollsel") / "kemu_rollsel")
    odir = os.path.join(ROOT, "oracle")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, os.path.join(KEMU, "test_rollsel.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                        "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_rollsel_kernel_logic_equals_plain_loop(kemu_rollsel, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_rollsel, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu rollsel ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
