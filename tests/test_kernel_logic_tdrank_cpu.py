"""Kernel LOGIC of the rank kernel without a GPU: gyeeta_amd/csrc/gys_tdrank.hpp compiled by g++ against the CPU stand-in of the HIP device
model (tests/cpp/kemu/hip/hip_runtime.h, as tests/test_kernel_logic_histroll_cpu.py does for the group histograms) and run on synthetic
digests (tests/cpp/kemu/test_tdrank.cc): service members with buffers of 0 .. td_pend_cap values at a buffer stride that is a multiple of 4
and one that is not, 0 / 1 / 2 / 200 clusters, gaps, equal neighbouring means, slab members with counts above 2^32, 1 .. 17 members and the
whole world, several grid sizes, thresholds at every place of the definition -- every answer equals a plain C++ loop of the definition
("Ranks" in include/gysketch.h) bit for bit.

And the definition itself, restated in Python (tests/test_gpu_td_ranks.py: the restatement the GPU tests compare the kernel with), on the
oracle's buffered digests against the EXACT SORT: |below - #{values <= x}| / total <= 0.01 (the project's rank-error tolerance, DESIGN.md
section 4) for every service, the totals, monotone in x, 0 below the minimum, the total at and above the maximum.  The definition reads the
clusters at x + 1/2; read at x itself it reaches 1.0 - 1.5e-2 on the lognormal, normal-1500-3 and edges cases here, and this test fails.
The -m gpu tests (tests/test_gpu_td_ranks.py) remain the check of the real thing."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def kemu_tdrank(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kemu_tdrank") / "kemu_tdrank")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-w", "-ffp-contract=off", "-I" + KEMU, os.path.join(KEMU, "test_tdrank.cc"), "-o", exe, "-pthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_tdrank_kernel_logic_equals_the_definition(kemu_tdrank, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "600", kemu_tdrank, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode == 77:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0 and "kemu tdrank ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


@pytest.mark.parametrize("td_cap", [896, 1920])
@pytest.mark.parametrize("dist", ["lognormal", "normal-1500-3", "uniform-600000-605000", "edges", "constant"])
def test_restatement_against_the_exact_sort_on_oracle_digests(oracle, dist, td_cap):
    from tests.test_gpu_td_ranks import H, S, RANK_TOL, below_restated, latencies, accepted_by_service, sort_thresholds
    rng = np.random.default_rng(["lognormal", "normal-1500-3", "uniform-600000-605000", "edges", "constant"].index(dist) * 7 + td_cap)
    orc = oracle.OracleEngine(H * S, td_cap=td_cap)
    info, _ = helpers.register_world(None, orc, range(H), S)
    vals = [[] for _ in range(H * S)]
    for rnd in range(7):  # (the last round is small: it stays in the buffers)
        for h in range(H):
            ev = helpers.make_resp_events(rng, h, int(rng.integers(1500, 4000)) if rnd < 6 else 200, S, lat=latencies(rng, dist))
            orc.resp_batch(ev.tobytes(), [info[h][1]], [0])
            for s, v in accepted_by_service(ev, S).items():
                vals[info[h][1] * S + s].append(v)
    sums, cnts, mm = orc.td_arrays()
    npend, pend = orc.td_pending()
    assert int(cnts.sum()) > 0 and int(npend.min()) > 0  # (merges have happened and every buffer holds values)
    worst = 0.0
    for slot in range(H * S):
        x = np.sort(np.concatenate(vals[slot]))
        thr = sort_thresholds(x)
        got = [below_restated(sums[slot], cnts[slot], mm[slot][0], mm[slot][1], pend[slot, :npend[slot]], t) for t in thr]
        exact = np.searchsorted(x, thr, side="right")
        assert int(cnts[slot].sum()) + int(npend[slot]) == len(x)
        err = np.abs(np.array(got) - exact) / len(x)
        worst = max(worst, float(err.max()))
        assert err.max() <= RANK_TOL, (dist, td_cap, slot, float(err.max()), int(thr[int(err.argmax())]))
        assert (np.diff(got) >= 0).all(), (dist, slot, "not monotone in x")
        assert got[0] == 0.0 and got[-1] == float(len(x))  # (the thresholds start below the minimum and end above the maximum)
    print("%s cap %d: worst rank error %.2e" % (dist, td_cap, worst))
