"""Roll-up digests and distinct counts of the services a filter selects, per group (gys_rollup_filtered_dev, gys_set_service_groups; kernels
in gyeeta_amd/csrc/gys_rollsel.hpp).  Worlds: the 12 uneven hosts in 3 clusters of tests/test_gpu_hll_rollup.py; 300 hosts of 5 services in
which one label group and the GYS_GROUP_NONE group exceed 1 024 members (several chunks); 4 200 hosts of 3 services with 9 000 labels (group
domains above the 4 096 groups a workgroup counts in LDS: the wave-joined global atomics, several tiles of the scan).  Response events feed the digests and the
registers, partha_listener_state records the state columns; an OracleEngine is fed the same response events with the same td_pend_cap.
  * host groups of all services == the fixed roll-ups bit for bit (slabs, files, estimates);
  * cluster / no-group / label groups: slabs == oracle.rollup_services over the members' oracle state, files == the byte-wise maximum of the
    members' exported rows == gyo_hll_merge, estimates within EST_RTOL of gyo_hll_estimate (the bound of tests/test_gpu_hll_rollup.py), an
    all-zero file exactly 0;
  * membership == gys_query_svcstate_scan / _aggr for several filters; a state record two windows old is out without GYS_RF_ANY_STATE, in with it;
  * levels 0 .. 3 == the maximum of gys_export_svc_hll_level rows == gys_hll_rollup_level_dev(HOST) for full host groups;
  * no side effects, the error codes, all-or-nothing labels, relabelling, maxrows below the rows;
  * quantiles 0.001 .. 0.999 of group slabs within the rank-error bound tests/test_gpu_rollup_accuracy.py applies (its _check, its constant)."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers
from tests.test_gpu_hll_rollup import EST_RTOL, SVCS, _close, _oracle_est, _oracle_merge
from tests.test_gpu_hll_rollup import torch_mod  # noqa: F401 -- the fixture
from tests.test_gpu_rollup_accuracy import _check, _same_slab

pytestmark = pytest.mark.gpu

NONE, HOST, CLUSTER, LABEL = capi.GROUP_NONE, capi.GROUP_HOST, capi.GROUP_CLUSTER, capi.GROUP_LABEL


class World:
    """hosts with svcs[h] services each, cluster h % 3; the engine, the oracle engine, slots and the accepted latencies per slot"""

    def __init__(self, oracle, svcs, td_cap=0, P=8, levels=0, seed=1):
        from gyeeta_amd.engine import SketchEngine
        self.oracle, self.svcs, self.P, self.m = oracle, svcs, P, 1 << P
        nh, nsvc = len(svcs), sum(svcs)
        self.eng = SketchEngine(max_hosts=nh + 1, max_services=nsvc + 8, max_batch_events=1 << 18, max_clusters=4, svc_hll_p=P, td_pend_cap=td_cap, svc_hll_levels=levels)
        self.orc = oracle.OracleEngine(nsvc + 8, td_cap=td_cap)
        self.rng = np.random.default_rng(seed)
        for c in range(3):
            self.eng.register_cluster("cluster%d" % c)
        self.mid, self.hslot, self.gids, self.slots = {}, {}, {}, {}
        for h, n in enumerate(svcs):
            self.mid[h] = wire.machine_id(h)
            self.hslot[h] = self.eng.register_host(self.mid[h], "cluster%d" % (h % 3))
            s = np.arange(n)
            self.gids[h] = wire.glob_id(np.full(n, h), s)
            if n:
                ns, pt = wire.listener_netns(h, s), wire.listener_port(s)
                self.eng.register_listeners_np(self.mid[h], self.gids[h], ns, pt)
                for i in range(n):
                    self.orc.register(self.hslot[h], int(self.gids[h][i]), int(ns[i]), int(pt[i]))
            self.slots[h] = [self.eng.lookup(int(g)) for g in self.gids[h]]
        self.nsvc = self.eng.num_services()
        assert self.nsvc == nsvc
        self.host_of = np.zeros(nsvc, dtype=np.int64)
        for h in self.slots:
            self.host_of[self.slots[h]] = h
        self.vals = [[] for _ in range(nsvc)]

    def feed(self, counts, lat_mu=None):
        for h, n in counts.items():
            sp = self.svcs[h]
            if not sp:
                continue
            ev = helpers.make_resp_events(self.rng, h, n, sp, lat_mu=float(self.rng.uniform(1.0, 7.0)) if lat_mu is None else lat_mu)
            self.eng.handle_resp_events(self.mid[h], ev)
            self.orc.resp_batch(ev.tobytes(), [self.hslot[h]], [0])
            lat = (ev["lsndtime"].astype(np.uint32) - ev["lrcvtime"].astype(np.uint32)).astype(np.uint32)
            svc = ev["sport_be"].astype(np.int64) - 1024
            ok = (lat <= 1000000) & (svc >= 0) & (svc < sp)
            for s in np.unique(svc[ok]):
                self.vals[self.slots[h][int(s)]].append(lat[ok & (svc == s)].astype(np.int64))

    def states(self, hosts, edit=None):
        for h in hosts:
            if self.svcs[h]:
                r = wire.synth_listener_states(self.rng, h, np.arange(self.svcs[h]))
                if edit:
                    edit(h, r)
                self.eng.partha_listener_state(self.mid[h], r.tobytes(), len(r))

    def pooled(self, slots):
        v = [x for s in slots for x in self.vals[s]]
        return np.concatenate(v) if v else np.zeros(0, dtype=np.int64)

    def check_groups(self, what, rows, out, members, rank_error=(), slab_rows=None):
        """rows / out of rollup_filtered against `members` {group: slots}: the rows, every slab against the oracle's direct union of the member
        services (slab_rows: of these rows only, where there are thousands), every file against the maximum of the exported rows and
        gyo_hll_merge, every estimate against gyo_hll_estimate"""
        o = self.oracle
        assert rows == [(g, len(members[g])) for g in sorted(members)], (what, rows[:5], sorted((g, len(s)) for g, s in members.items())[:5])
        files = self.eng.export_svc_hll()
        for r, (g, n) in enumerate(rows):
            sl = members[g]
            if "slabs" in out and (slab_rows is None or r in slab_rows or g in rank_error):
                assert _same_slab(out["slabs"][r], o.rollup_services([self.orc.td(s) for s in sl])), f"{what}: slab of group {g} ({n} members) differs from the oracle's"
                if g in rank_error:
                    _check(f"{what} group {g}", self.eng, out["slabs_dev"], r, out["slabs"][r], self.pooled(sl))
            if "regs" in out:
                want = np.maximum.reduce(files[sl])
                assert (out["regs"][r] == want).all() and (want == _oracle_merge(o, files[sl], self.P)).all(), f"{what}: file of group {g}"
            if "est" in out and "regs" in out:
                w = _oracle_est(o, out["regs"][r], self.P)
                assert _close(out["est"][r], w), f"{what}: estimate of group {g}: {out['est'][r]!r}, oracle {w!r}"
                if not out["regs"][r].any():
                    assert out["est"][r].tobytes() == np.float64(0.0).tobytes()


COUNTS = {0: 900, 1: 30, 2: 2500, 4: 6000, 5: 40, 6: 9000, 8: 12, 9: 3000, 10: 200, 11: 1500}  # (host 3 has no service, host 7 gets no events)


@pytest.mark.parametrize("td_cap", [0, 1920])
def test_groups_of_the_uneven_world(torch_mod, oracle, td_cap):
    """checks 1, 2, 3 and 6 of the issue on the 12 uneven hosts"""
    w = World(oracle, SVCS, td_cap=td_cap, seed=31 + td_cap)
    eng = w.eng
    # host 9 reports its states first, two windows pass (its records go stale); then the others report into the open window; then the events
    w.states([9])
    eng.window_close()
    eng.window_close()

    def edit(h, r):
        r["curr_state"] = np.arange(len(r)) % 6

    w.states([h for h in range(len(SVCS)) if h not in (9, 5)], edit)  # (host 5 never reports)
    for rnd in range(3):
        w.feed(COUNTS)
    eng.sync()
    assert max(w.orc.td(i).npend for i in range(w.nsvc)) > 64
    allslots = {h: w.slots[h] for h in w.slots if w.slots[h]}
    # 1. host groups of every service == the fixed roll-ups, bit for bit
    rows, nrows, out = eng.rollup_filtered(HOST, any_state=True)
    assert nrows == len(rows) == len(allslots) and rows == [(w.hslot[h], len(allslots[h])) for h in sorted(allslots, key=lambda x: w.hslot[x])]
    _, rec_h = eng.tdigest_rollup(capi.ROLLUP_HOST)
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    for r, (g, n) in enumerate(rows):
        assert out["slabs"][r].tobytes() == rec_h[g].tobytes(), f"host {g}: slab differs from gys_tdigest_rollup_dev(HOST)"
        assert (out["regs"][r] == hf[g]).all() and out["est"][r].tobytes() == he[g].tobytes(), f"host {g}: file / estimate differ from gys_hll_rollup_dev(HOST)"
    w.check_groups("hosts", rows, out, {w.hslot[h]: s for h, s in allslots.items()})
    # 2. cluster, no-group and label groups of every service
    cl = {c: [s for h in allslots if h % 3 == c for s in allslots[h]] for c in range(3)}
    rows, nrows, out = eng.rollup_filtered(CLUSTER, any_state=True)
    w.check_groups("clusters", rows, out, cl, rank_error=(0, 1, 2))
    cf, ce = eng.hll_rollup(capi.ROLLUP_CLUSTER)
    assert (out["regs"] == cf).all() and out["est"].tobytes() == ce.tobytes()
    rows, nrows, out = eng.rollup_filtered(NONE, any_state=True)
    w.check_groups("all", rows, out, {0: list(range(w.nsvc))}, rank_error=(0,))
    gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    assert (out["regs"] == gf).all() and out["est"].tobytes() == ge.tobytes()
    assert eng.rollup_filtered(LABEL, any_state=True)[:2] == ([], 0)  # no label was set
    # labels: "the same service on all its hosts" (service index % 5), label 77 for host 7's services alone (no events: an all-zero file)
    ids = np.concatenate([w.gids[h] for h in allslots])
    lab = np.concatenate([np.where(np.full(len(w.gids[h]), h == 7), 77, np.arange(len(w.gids[h])) % 5) for h in allslots]).astype(np.uint32)
    lab[3] = capi.NO_GROUP
    eng.set_service_groups(ids, lab)
    lm = {}
    for g, l in zip(ids.tolist(), lab.tolist()):
        if l != capi.NO_GROUP:
            lm.setdefault(l, []).append(eng.lookup(g))
    rows, nrows, out = eng.rollup_filtered(LABEL, any_state=True)
    w.check_groups("labels", rows, out, lm, rank_error=(0, 4))
    assert rows[-1][0] == 77 and not out["regs"][-1].any() and out["est"][-1] == 0.0 and int(out["slabs"][-1]["cnt"].sum()) == 0
    # 3. membership against the scan and the aggregate for several filters; the digests and files of the slot sets
    filters = [dict(), dict(terms=[("state", ">=", 3), ("qps5s", ">", 2)]), dict(terms=[("state", "=", 1, 0), ("nconns", ">", 3, 0), ("state", "=", 4, 1), ("sererr", ">=", 0, 1)],
                                                                                group_oper=["or", "and"], top_oper="or"),
               dict(svcids=[int(w.gids[h][k]) for h, k in ((0, 1), (4, 16), (6, 39), (9, 2), (2, 0))] + [4242]), dict(machine_ids=[w.mid[6], w.mid[4], w.mid[9], wire.machine_id(99)]),
               dict(clusters=["cluster1", "nosuch"], terms=[("state", "!=", 0)]), dict(terms=[("qps5s", "<", 0)])]
    for fi, f in enumerate(filters):
        gs, gh, _, nm = eng.svcstate_scan(f.get("terms"), f.get("group_oper", ()), f.get("top_oper", "and"), None, True, w.nsvc, f.get("machine_ids"), f.get("svcids"),
                                          f.get("clusters"))
        assert len(gs) == nm
        assert not set(gs.tolist()) & set(w.slots[9] + w.slots[5])  # stale / never reported
        for group_by in (NONE, HOST, CLUSTER, LABEL):
            key = {NONE: lambda s, h: 0, HOST: lambda s, h: h, CLUSTER: lambda s, h: int(w.host_of[s]) % 3, LABEL: lambda s, h: w_label(eng, lm, s)}[group_by]
            mem = {}
            for s, h in zip(gs.tolist(), gh.tolist()):
                k = key(s, h)
                if k is not None:
                    mem.setdefault(k, []).append(s)
            rows, nrows, out = eng.rollup_filtered(group_by, f.get("terms"), f.get("group_oper", ()), f.get("top_oper", "and"), f.get("machine_ids"), f.get("svcids"),
                                                   f.get("clusters"))
            w.check_groups(f"filter {fi} group_by {group_by}", rows, out, mem, rank_error=(0,) if fi == 1 else ())
            assert nrows == len(mem)
            if group_by != LABEL:
                ag = eng.svcstate_aggr([], group_by, f.get("terms"), f.get("group_oper", ()), f.get("top_oper", "and"), f.get("machine_ids"), svcids=f.get("svcids"),
                                       clusters=f.get("clusters"), maxrows=64)
                assert [(g, n) for g, n, _ in ag] == rows and sum(n for _, n in rows) == nm
        if fi == len(filters) - 1:
            assert nm == 0
    assert sum(len(v) for v in lm.values()) > 0
    # the stale host: out without the flag, in with it (its kept records are evaluated)
    f9 = dict(machine_ids=[w.mid[9]])
    assert eng.rollup_filtered(HOST, **f9)[:2] == ([], 0)
    rows, nrows, out = eng.rollup_filtered(HOST, any_state=True, terms=[("nqry5s", ">=", 0)], **f9)
    w.check_groups("stale host", rows, out, {w.hslot[9]: w.slots[9]})
    rows, _, _ = eng.rollup_filtered(NONE, any_state=True, terms=[("nqry5s", ">", 0), ("state", ">", 5)], group_oper=["or"], machine_ids=[w.mid[5]])
    assert rows == []  # never reported: the kept record is all zero
    eng.close()


def w_label(eng, lm, slot):
    for l, sl in lm.items():
        if slot in sl:
            return l
    return None


def test_many_hosts_groups_of_several_chunks(torch_mod, oracle):
    """300 hosts of 5 services: the GYS_GROUP_NONE group (1 500) and one label group (1 100) span two chunks of 1 024 members; 290 label groups
    besides; maxrows below the rows; relabelling; the rank error of the large groups"""
    nh, sp = 300, 5
    w = World(oracle, [sp] * nh, td_cap=1920, P=4, seed=5)
    eng = w.eng
    for rnd in range(2):
        w.feed({h: int(w.rng.integers(150, 400)) for h in range(nh)})
    eng.sync()
    ids = np.concatenate([w.gids[h] for h in range(nh)])
    slots = np.array([s for h in range(nh) for s in w.slots[h]])
    perm = w.rng.permutation(len(ids))
    lab = np.empty(len(ids), dtype=np.uint32)
    lab[perm[:1100]] = 1400                    # the large group, scattered over the hosts
    lab[perm[1100:1400]] = np.arange(300) + 7  # 290 distinct small groups ...
    lab[perm[1390:1400]] = 9                   # ... (ten of them relabelled into one)
    lab[perm[1400:]] = capi.NO_GROUP
    eng.set_service_groups(ids, lab)
    lm = {}
    for s, l in zip(slots.tolist(), lab.tolist()):
        if l != capi.NO_GROUP:
            lm.setdefault(l, []).append(s)
    assert len(lm[1400]) == 1100
    rows, nrows, out = eng.rollup_filtered(LABEL, any_state=True)
    w.check_groups("labels", rows, out, lm, rank_error=(1400,))
    rows, nrows, out = eng.rollup_filtered(NONE, any_state=True)
    w.check_groups("all", rows, out, {0: list(range(w.nsvc))}, rank_error=(0,))
    rows, nrows, out = eng.rollup_filtered(HOST, any_state=True, want=("regs", "est"))
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    assert nrows == nh and (out["regs"] == hf).all() and out["est"].tobytes() == he.tobytes()
    # maxrows below the rows: the first groups only, the total reported
    full_rows, _, full = eng.rollup_filtered(LABEL, any_state=True)
    rows, nrows, out = eng.rollup_filtered(LABEL, any_state=True, maxrows=17)
    assert nrows == len(lm) and rows == full_rows[:17] and out["slabs"].tobytes() == full["slabs"][:17].tobytes() and (out["regs"] == full["regs"][:17]).all()
    assert out["est"].tobytes() == full["est"][:17].tobytes()
    # all-or-nothing on an unknown id; relabelling changes the next answer
    with pytest.raises(capi.GysError) as e:
        eng.set_service_groups(np.array([ids[0], 123456789], dtype=np.uint64), np.array([5, 5], dtype=np.uint32))
    assert e.value.code == capi.ERR_INVAL
    with pytest.raises(capi.GysError):
        eng.set_service_groups(ids[:1], np.array([w.nsvc + 8], dtype=np.uint32))  # a group that is not below max_services
    assert eng.rollup_filtered(LABEL, any_state=True, want=("est",))[0] == full_rows
    eng.set_service_groups(ids[perm[:100]], np.full(100, 2, dtype=np.uint32))
    for s in slots[perm[:100]].tolist():
        lm[1400].remove(s)
        lm.setdefault(2, []).append(s)
    rows, nrows, out = eng.rollup_filtered(LABEL, any_state=True)
    w.check_groups("relabelled", rows, out, lm)
    eng.close()


def test_group_domains_above_the_lds_tables(torch_mod, oracle):
    """4 200 hosts of 3 services and labels scattered up to 9 000 with one heavy label of 3 000 members: group domains above 4 096, where
    k_rollsel_count and k_rollsel_scatter join a wave's equal groups by ballots and lane reads and go to the global counters, and the scan over
    the domain takes several tiles.  Labels and hosts against the same references as the small domains; membership of a filtered host grouping
    against the aggregate query; maxrows below the rows"""
    nh, sp = 4200, 3
    w = World(oracle, [sp] * nh, td_cap=1920, P=4, seed=12)
    eng = w.eng
    fed = [h for h in range(nh) if h % 3 != 1]
    w.feed({h: int(w.rng.integers(40, 120)) for h in fed})

    def edit(h, r):
        r["curr_state"] = (np.arange(len(r)) + h) % 6

    w.states(range(0, nh, 7), edit)
    eng.sync()
    # hosts: a domain of 4 200 groups
    rows, nrows, out = eng.rollup_filtered(HOST, any_state=True)
    assert nrows == nh and rows == [(h, sp) for h in range(nh)]
    _, rec_h = eng.tdigest_rollup(capi.ROLLUP_HOST)
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    assert out["slabs"].tobytes() == rec_h.tobytes() and (out["regs"] == hf).all() and out["est"].tobytes() == he.tobytes()
    w.check_groups("4200 hosts", rows, out, {w.hslot[h]: w.slots[h] for h in range(nh)}, slab_rows=range(0, nh, 97))
    rows, nrows, out = eng.rollup_filtered(HOST, [("nqry5s", ">=", 0)], want=("est",))  # the hosts whose states are current
    ag = eng.svcstate_aggr([], 1, [("nqry5s", ">=", 0)], maxrows=nh)
    assert rows == [(g, n) for g, n, _ in ag] == [(w.hslot[h], sp) for h in range(0, nh, 7)]
    # labels: a domain of 9 000, most groups of one or two members, label 8 000 with 3 000 members on all hosts, some services unlabelled
    ids = np.concatenate([w.gids[h] for h in range(nh)])
    slots = np.array([s for h in range(nh) for s in w.slots[h]])
    perm = w.rng.permutation(len(ids))
    lab = w.rng.integers(0, 9000, len(ids)).astype(np.uint32)
    lab[perm[:3000]] = 8000
    lab[perm[3000:3600]] = capi.NO_GROUP
    lab[perm[3600]] = 8999
    eng.set_service_groups(ids, lab)
    lm = {}
    for s_, l in zip(slots.tolist(), lab.tolist()):
        if l != capi.NO_GROUP:
            lm.setdefault(l, []).append(s_)
    assert len(lm) > 4096 and len(lm[8000]) >= 3000
    rows, nrows, out = eng.rollup_filtered(LABEL, any_state=True)
    assert nrows == len(lm)
    w.check_groups("9000 labels", rows, out, lm, rank_error=(8000,), slab_rows=range(0, len(lm), 61))
    cut_rows, cut_n, cut = eng.rollup_filtered(LABEL, any_state=True, maxrows=100)
    assert cut_n == len(lm) and cut_rows == rows[:100] and cut["slabs"].tobytes() == out["slabs"][:100].tobytes() and (cut["regs"] == out["regs"][:100]).all()
    assert cut["est"].tobytes() == out["est"][:100].tobytes()
    # a filter on top: the labelled services of the hosts whose states are current and whose state is bad
    gs, gh, _, nm = eng.svcstate_scan([("state", ">=", 2)], maxrecs=w.nsvc)
    mem = {}
    lab_of = dict(zip(slots.tolist(), lab.tolist()))
    for s_ in gs.tolist():
        if lab_of[s_] != capi.NO_GROUP:
            mem.setdefault(lab_of[s_], []).append(s_)
    assert len(mem) > 100
    rows, nrows, out = eng.rollup_filtered(LABEL, [("state", ">=", 2)])
    w.check_groups("9000 labels, filtered", rows, out, mem, slab_rows=range(0, len(mem), 13))
    eng.close()


def test_levels(torch_mod, oracle):
    """hll_level 0 .. 3: == the maximum of gys_export_svc_hll_level rows over the members == gys_hll_rollup_level_dev(HOST) for full host groups"""
    w = World(oracle, SVCS, P=8, levels=1, seed=9)
    eng = w.eng
    t = 1_700_000_000
    for k, step in enumerate([5, 5, 30, 301, 5]):
        w.feed({h: max(3, n // 10) for h, n in COUNTS.items() if (h + k) % 3})
        t += step
        eng.window_close(t * 1_000_000)
    w.feed({0: 50, 6: 500})  # the open window
    eng.sync()
    ids = np.concatenate([w.gids[h] for h in range(len(SVCS))])
    eng.set_service_groups(ids, (np.arange(len(ids)) % 4).astype(np.uint32))
    lm = {l: [eng.lookup(int(g)) for g in ids[l::4]] for l in range(4)}
    hosts = {w.hslot[h]: w.slots[h] for h in w.slots if w.slots[h]}
    seen = 0
    for level in range(4):
        for tq in (t, t + 3, t + 200):
            tus = tq * 1_000_000
            files = eng.export_svc_hll_level(level, tus)
            rows, _, out = eng.rollup_filtered(LABEL, any_state=True, hll_level=level, tusec=tus, want=("regs", "est"))
            assert rows == [(l, len(lm[l])) for l in range(4)]
            for r in range(4):
                assert (out["regs"][r] == np.maximum.reduce(files[lm[r]])).all(), (level, tq, r)
                assert _close(out["est"][r], _oracle_est(oracle, out["regs"][r], w.P))
            rows, _, out = eng.rollup_filtered(HOST, any_state=True, hll_level=level, tusec=tus, want=("regs", "est"))
            hf, he = eng.hll_rollup_level(capi.ROLLUP_HOST, level, tus)
            assert [g for g, _ in rows] == sorted(hosts)
            for r, (g, _) in enumerate(rows):
                assert (out["regs"][r] == hf[g]).all() and out["est"][r].tobytes() == he[g].tobytes(), (level, tq, g)
            seen += int(out["regs"].any())
    assert seen >= 6
    # the open window is another thing
    rows, _, out = eng.rollup_filtered(HOST, any_state=True, want=("regs",))
    assert (out["regs"] == eng.hll_rollup(capi.ROLLUP_HOST)[0][[g for g, _ in rows]]).all()
    eng.close()


def test_no_side_effects_and_error_codes(torch_mod, oracle):
    from gyeeta_amd.engine import SketchEngine
    w = World(oracle, SVCS, P=4, seed=3)
    eng, L = w.eng, w.eng.L
    w.states(range(len(SVCS)))
    w.feed(COUNTS)
    eng.sync()

    def snapshot():
        return [x.tobytes() for x in eng.export_tdigest()] + [x.tobytes() for x in eng.export_tdigest_pending()] + [eng.export_svc_hll().tobytes(), eng.export_hist(1).tobytes()]

    before = snapshot()
    eng.set_service_groups(w.gids[6], np.arange(len(w.gids[6]), dtype=np.uint32) % 3)
    for group_by in (NONE, HOST, CLUSTER, LABEL):
        for any_state in (False, True):
            rows, nrows, out = eng.rollup_filtered(group_by, [("state", "<=", 5)], any_state=any_state)
            assert nrows == len(rows) > 0
    assert snapshot() == before
    # the error codes
    f, keep = eng._svc_filter(None)
    rows = (capi.RollupRow * 16)()
    n = C.c_uint32()
    est = torch_mod.zeros(16, dtype=torch_mod.float64, device=eng.device)
    slabs = torch_mod.zeros(16 * C.sizeof(capi.TDigestSlab), dtype=torch_mod.uint8, device=eng.device)
    regs = torch_mod.zeros(16 * 16 + 16, dtype=torch_mod.uint8, device=eng.device)
    pe, ps, pr = C.c_void_p(est.data_ptr()), C.c_void_p(slabs.data_ptr()), C.c_void_p(regs.data_ptr())

    def call(e=eng, filt=C.byref(f), flags=0, group_by=HOST, level=-1, rows_=rows, nrows_=C.byref(n), s=ps, r=pr, d=pe):
        return L.gys_rollup_filtered_dev(e.h, filt, flags, group_by, level, 0, rows_, 16, nrows_, s, r, d)

    assert call() == capi.OK and n.value == len([x for x in SVCS if x])
    assert call(filt=None) == capi.ERR_INVAL and call(rows_=None) == capi.ERR_INVAL and call(nrows_=None) == capi.ERR_INVAL
    assert call(group_by=4) == capi.ERR_INVAL and call(group_by=-1) == capi.ERR_INVAL and call(flags=2) == capi.ERR_INVAL
    assert call(level=4) == capi.ERR_INVAL and call(level=-2) == capi.ERR_INVAL
    assert call(s=None, r=None, d=None) == capi.ERR_INVAL
    assert call(r=C.c_void_p(regs.data_ptr() + 4)) == capi.ERR_INVAL  # a file array that is not 16-byte aligned
    assert call(level=0) == capi.ERR_STATE and call(level=3, s=None, r=None) == capi.ERR_STATE  # svc_hll_levels = 0
    assert call(level=2, r=None, d=None) == capi.OK  # (digests only: the level is not looked at)
    assert call(s=None, d=None) == capi.OK and call(s=None, r=None) == capi.OK and call(r=None, d=None) == capi.OK
    nohll = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10)
    assert call(e=nohll, s=None) == capi.ERR_STATE and call(e=nohll, r=None, d=None) == capi.OK and n.value == 0
    bad, keep2 = nohll._svc_filter([("qps5s", ">", 1, 9)])  # a criteria group out of range: refused although nothing is registered
    assert call(e=nohll, filt=C.byref(bad), r=None, d=None) == capi.ERR_INVAL
    nohll.close()
    notd = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10, enable_tdigest=False, svc_hll_p=4)
    assert call(e=notd) == capi.ERR_STATE and call(e=notd, s=None) == capi.OK
    notd.close()
    eng.close()
