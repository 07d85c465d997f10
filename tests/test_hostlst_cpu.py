"""The host mirror of the listener registry without a GPU: gyeeta_amd/csrc/gys_hostlst.hpp (pure host code: per-host sub-tables, the cut of
a many-listener host into parts, chains of bound-address listeners, the overflow fallback, the dirty / rebuild protocol) compiled by g++
with AddressSanitizer and UBSan into a stand-alone program (tests/cpp/test_hostlst.cc, over the CPU stand-in of the HIP device model,
tests/cpp/kemu, as tests/test_resp_plan_cpu.py) and checked against the plain statement of the reference's insert-or-replace / first-match
rule over named edge cases and seeded random sequences of registrations and deletions.  Nothing is loaded into Python.
The same program's --tables mode registers the key lists of the lookup scenarios (tests/lstkeys.py) through host_lst_insert / host_lst_remove
and prints every sub-table: the Python restatement of the hash, the capacity rule and the insertion order that picks those keys is pinned
to the mirror entry for entry.
The -m gpu tests (tests/test_gpu_listener_delete.py, tests/test_gpu_round3.py) remain the check of the device copy."""
import os
import subprocess

import pytest

from tests import lstkeys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")


@pytest.fixture(scope="module")
def hostlst_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostlst") / "test_hostlst")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + KEMU,
                        os.path.join(ROOT, "tests", "cpp", "test_hostlst.cc"), "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_host_listeners_equal_plain_rules(hostlst_exe, seed):
    p = subprocess.run(["timeout", "-s", "KILL", "300", hostlst_exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "host listeners ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


def test_lookup_scenario_tables_equal_the_mirror(hostlst_exe, tmp_path):
    """every scenario of tests/lstkeys.py (each checks its own witnesses when it is built): after every registry call of every host the
    mirror's sub-tables and local -> slot lists are the predicted ones, entry for entry"""
    names = list(lstkeys.BUILDERS)
    hosts = lstkeys.write_registry_ops(str(tmp_path / "ops.txt"), names)
    p = subprocess.run(["timeout", "-s", "KILL", "300", hostlst_exe, "--tables", str(tmp_path / "ops.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "host listener tables ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    got = lstkeys.parse_registry_dump(p.stdout)
    assert len(got) == len(hosts) >= 13 and any(st.cands for h in hosts for st in h.steps)
    for h, dumps in zip(hosts, got):
        assert len(dumps) == len(h.steps)
        for i, (st, (parts, cands)) in enumerate(zip(h.steps, dumps)):
            assert len(parts) == len(st.tables), (h.name, i)
            assert cands == st.cands, "%s step %d: candidate records differ" % (h.name, i)
            for p_no, ((tbl, slots), (want_tbl, want_slots)) in enumerate(zip(parts, st.tables)):
                assert slots == want_slots, "%s step %d part %d: local -> slot list differs" % (h.name, i, p_no)
                assert len(tbl) == len(want_tbl), "%s step %d part %d: %d entries, predicted %d" % (h.name, i, p_no, len(tbl), len(want_tbl))
                bad = [(j, hex(a), hex(b)) for j, (a, b) in enumerate(zip(tbl, want_tbl)) if a != b]
                assert not bad, "%s step %d part %d: entries differ (index, mirror, predicted): %s" % (h.name, i, p_no, bad[:4])


def test_lookup_scenarios_fail_when_an_edge_is_lost(monkeypatch):
    """a changed capacity rule (tables twice as large) takes the scenarios' edges away: the builder says so instead of testing less"""
    monkeypatch.setattr(lstkeys, "capacity", lambda n: 2 * lstkeys.next_pow2(max(16, 4 * n)))
    with pytest.raises(lstkeys.ScenarioError, match="no longer reaches its edge"):
        lstkeys.scenario_a()
