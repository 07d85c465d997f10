"""Kernel LOGIC of the group-histogram kernel without a GPU: gyeeta_amd/csrc/gys_histroll.hpp compiled by g++ against the CPU stand-in of the
HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_rollsel_cpu.py does for the selection kernels) and run on
synthetic cumulative / window / snapshot / last-window records with their td_meta and tags (tests/cpp/kemu/test_histroll.cc): all three
level modes with and without lazily folded records, chunks of 1 .. 1024 members, a group of three chunks, an empty group, several grid sizes
-- the chunks' partial records and the rows' records equal a plain loop of the shared level-view rule followed by gyo_hist_merge byte for
byte, and the plain mode over the partials equals the direct sum.  The -m gpu tests (tests/test_gpu_hist_rollup.py) remain the check of the
real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_histroll(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    exe = str(tmp_path_factory.mktemp("kemu_histroll") / "kemu_histroll")
    odir = os.path.join(ROOT, "oracle")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, os.path.join(KEMU, "test_histroll.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                        "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_histroll_kernel_logic_equals_plain_loop(kemu_histroll, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_histroll, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu histroll ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
