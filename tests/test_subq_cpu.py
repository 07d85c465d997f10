"""The submission queues and the staging ring of the host-pointer calls without a GPU: gyeeta_amd/csrc/gys_subq.hpp (the library's only
multi-threaded code: group commit from 16 caller threads, a flusher thread per queue, parked errors, first-use allocation outside the
lock, the 16-slot ring) compiled by g++ into a stand-alone program (tests/cpp/test_subq.cc) over a fake HIP runtime whose device is a
thread that the test can stall, and checked against the sentences of the header's own protocol comment -- once under ThreadSanitizer,
once under AddressSanitizer + UBSan (+ LeakSanitizer), two seeds each.  Nothing is loaded into Python.
The -m gpu tests (tests/test_gpu_round3.py, tests/test_gpu_round4.py) remain the check against the real runtime.
Measured on 8 cores: 2.7 - 2.9 s per run under ThreadSanitizer, 1.0 - 1.2 s under AddressSanitizer (960 calls from 16 threads)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
SANITIZERS = {"tsan": ["-fsanitize=thread"], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def subq_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subq_" + request.param) / "test_subq")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w"] + SANITIZERS[request.param] + ["-I" + KEMU, os.path.join(ROOT, "tests", "cpp", "test_subq.cc"),
                        "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_submission_queues_and_ring_keep_their_protocol(subq_exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "300", subq_exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "subq ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
