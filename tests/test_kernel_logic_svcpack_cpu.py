"""Kernel LOGIC of the service-record kernels without a GPU: gyeeta_amd/csrc/gys_svcpack.hpp compiled by g++ against the CPU stand-in of the
HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_svcdel_cpu.py does for the deletion kernels) and run by
tests/cpp/kemu/test_svcpack.cc: pack, k_svc_clear, unpack over a synthetic segment list with segments of every size class, value buffers at
all four residues from a 16-byte boundary and cursors at the edges -- once plain, once as a stand-alone program built with
-fsanitize=address,undefined, which has to report nothing.  The -m gpu tests (tests/test_gpu_svcpack.py) remain the check of the real thing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, "-I" + os.path.join(ROOT, "include"), os.path.join(KEMU, "test_svcpack.cc"), "-o", exe,
                        "-pthread"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.fixture(scope="module")
def kemu_svcpack(tmp_path_factory):
    return _build(tmp_path_factory, "kemu_svcpack", [])


@pytest.fixture(scope="module")
def kemu_svcpack_san(tmp_path_factory):
    return _build(tmp_path_factory, "kemu_svcpack_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def _run(exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu svcpack ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return p


@pytest.mark.parametrize("seed", [1, 2])
def test_svcpack_kernel_logic(kemu_svcpack, seed):
    _run(kemu_svcpack, seed)


def test_svcpack_kernel_logic_sanitized(kemu_svcpack_san):
    p = _run(kemu_svcpack_san, 3)  # (a sanitizer report ends the program with a non-zero status)
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
