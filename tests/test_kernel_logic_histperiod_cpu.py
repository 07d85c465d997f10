"""Kernel LOGIC of the group-period kernel without a GPU: k_hist_period_union (gyeeta_amd/csrc/gys_histroll.hpp) compiled by g++ against the
CPU stand-in of the HIP device model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_histroll_cpu.py does for the level union)
and run on synthetic cumulative / window / boundary-snapshot / last-window / first-close records with their td_meta and tags
(tests/cpp/kemu/test_histperiod.cc): all four period modes with and without lazily folded records, 1, 2 and 10 ring buckets, whole and
partly covered ones under scales that truncate, chunks of 1 .. 1024 members, a group of three chunks, an empty group, several grid sizes --
the chunks' partial records and the rows' records equal a plain loop of period_pair_value per member followed by gyo_hist_merge byte for
byte, and k_level_period stores the same per-member records.  Plus, independent of any build: the six group entry points are declared in
include/gysketch.h and listed in capi.SIGNATURES.  The -m gpu tests (tests/test_gpu_hist_period_rollup.py) remain the check of the real
thing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")

NEW_SYMBOLS = ["gys_hist_rollup_period_dev", "gys_hist_rollup_period_filtered_dev", "gys_svc_hist_rollup_dev", "gys_svc_hist_rollup_filtered_dev",
               "gys_day_stats_rollup_dev", "gys_day_stats_rollup_filtered_dev"]


@pytest.fixture(scope="module")
def kemu_histperiod(tmp_path_factory, oracle):
    oracle.lib()  # builds oracle/liboracle.so if needed
    exe = str(tmp_path_factory.mktemp("kemu_histperiod") / "kemu_histperiod")
    odir = os.path.join(ROOT, "oracle")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-I" + KEMU, os.path.join(KEMU, "test_histperiod.cc"), "-o", exe, "-L" + odir, "-l:liboracle.so",
                        "-Wl,-rpath," + odir, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_histperiod_kernel_logic_equals_plain_loop(kemu_histperiod, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_histperiod, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu histperiod ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


def test_group_entry_points_declared_and_bound():
    from gyeeta_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gysketch.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gys_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/gysketch.h"
        assert name in capi.SIGNATURES, name + " is not in capi.SIGNATURES"
        assert capi.SIGNATURES[name][0] is not None and len(capi.SIGNATURES[name][1]) >= 4
    assert "#define GYS_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "gysketch.h")).read()  # symbols are added only
