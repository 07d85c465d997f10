"""Kernel LOGIC of the live active-connection row table without a GPU: gyeeta_amd/csrc/gys_actpairs.hpp (k_actp_find / _keep / _add, the fused
k_actp_all, k_actp_rebuild, k_actp_list, k_actp_svc_accum) compiled by g++ against the CPU stand-in of the HIP device model
(tests/cpp/kemu/hip/hip_runtime.h) and run by tests/cpp/kemu/test_actpairs.cc against a std::map written from the definition ("Live
active-connection rows" in include/gysketch.h): call sizes around the wave and the fused form's limit, one key 300 times, keys that share a
home entry and a chain that wraps the table's end, the window rule, the rebuild (cap 128, 32 fresh keys per window over 40 windows: no drop)
and a call with more keys than entries.  The program is a stand-alone executable: it runs once plain and once built with
-fsanitize=address (the tables, the row -> entry list and the output rows are heap arrays of their exact sizes).  The -m gpu tests remain
the check of the real thing.  A second test compares the JSON field list the GPU test uses with the reference's json_db_activeconn_arr."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
BUILDS = {"plain": [], "address-sanitizer": ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]}

# the fields of one "activeconn" object, in order (gys_json_activeconn; tests/test_gpu_actconn_pairs.py imports this list)
ACTIVECONN_FIELDS = ["time", "svcid", "svcname", "cprocid", "cname", "cparid", "cmadid", "cnetout", "cnetin", "cdelms", "sdelms", "rttms", "nconns", "csvc"]


@pytest.fixture(scope="module")
def kemu_actpairs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kemu_actpairs")
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("kemu_actpairs_" + name))
        procs[name] = (exe, subprocess.Popen(["g++", "-std=c++20", "-O1", "-w", "-ffp-contract=off", "-I" + KEMU] + flags + [os.path.join(KEMU, "test_actpairs.cc"), "-o", exe, "-pthread"],
                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    builds = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        builds[name] = (exe, p.returncode, log)
    runs = {name: subprocess.Popen(["timeout", "-s", "KILL", "900", exe, "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for name, (exe, rc, log) in builds.items() if rc == 0}
    results = {}
    for name, (exe, rc, log) in builds.items():
        if rc != 0:
            results[name] = (-1, "", "build failed:\n" + log[-3000:])
        else:
            so, se = runs[name].communicate()
            results[name] = (runs[name].returncode, so, se)
    return results


@pytest.mark.parametrize("build", list(BUILDS))
def test_actpairs_kernel_logic_equals_the_map_model(kemu_actpairs, build):
    rc, so, se = kemu_actpairs[build]
    if rc == 77:
        pytest.skip(so.strip())
    assert rc == 0 and "kemu actpairs ok" in so, (rc, so[-2000:], se[-2000:])


def test_activeconn_json_fields_are_the_reference_field_map():
    """json_db_activeconn_arr (common/gy_json_field_maps.h:1479-1495), parsed from the reference header: names and order"""
    ref = os.path.join(os.environ.get("GY_REFERENCE_DIR", "/root/reference"), "common", "gy_json_field_maps.h")
    if not os.path.isfile(ref):
        pytest.skip("no reference tree here")
    src = open(ref, errors="replace").read()
    m = re.search(r"json_db_activeconn_arr\[\]\s*=\s*\{(.*?)\n\};", src, flags=re.S)
    assert m, "json_db_activeconn_arr not found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = re.findall(r'\{\s*"([a-z0-9_]+)"\s*,\s*"[a-z0-9_]+"\s*,', body)
    assert fields == ACTIVECONN_FIELDS, fields
