"""The shim's service-record members (gys_mconn_shim.hpp: save_all / load_all, save_partha_services / restore_services) from plain C++:
tests/cpp/test_shim_state.cc compiles and links with g++ against the C ABI (CPU check) and restores a handler from a file and from one
partha's blob on the GPU (gpu check)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from gyeeta_amd import build
    if build.needs_build():
        build.build()
    exe = str(tmp_path / "test_shim_state")
    lib = os.path.join(ROOT, "gyeeta_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_shim_state.cc"), "-o", exe,
                           "-L" + lib, "-lgysketch", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_shim_state_compiles_and_links_with_gxx(tmp_path):
    exe = _build(tmp_path)
    assert "link ok, abi 7" in subprocess.check_output([exe]).decode()


@pytest.mark.gpu
def test_shim_state_runs_on_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run(["timeout", "-s", "KILL", "120", exe, str(tmp_path / "state.gys")], capture_output=True, text=True)
    assert r.returncode == 0 and "shim state ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
