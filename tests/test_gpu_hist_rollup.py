"""Group response-time histograms of the four levels (gys_hist_rollup_level_dev, gys_hist_rollup_filtered_dev; kernel k_hist_level_union in
gyeeta_amd/csrc/gys_histroll.hpp).  The reference sum of every check is computed in numpy from gys_export_hist_level of the members at the same
tusec (k_level_view: other device code, pinned to the ring oracle by tests/test_gpu_levels.py): counts added as 64-bit words (int64 adds wrap
like u64 adds), sums as int64, the maximum on [15][1]; no member: all zero with max_val_seen = INT64_MIN.  Everything is compared bit for bit.
  1. fixed scopes over time, lazily folded (enable_tdigest) and eager records: 6 hosts of 1, 3, 5, 17, 70 and 0 services in 3 clusters (one
     holds only the service-less host); 5-s steps, a step over a 30-s boundary, a gap above 300 s, a step over a 12-h boundary; queries at
     every close, 3 s and 7 s later, and with events in the open window; HOST / CLUSTER / GLOBAL x levels 0 .. 3; cluster == sum of its
     hosts; GLOBAL level 3 == all-time records minus the open window; the lazy run also against the summed RingOracle; p25 / 50 / 95 / 99 of
     gys_hist_percentiles_dev on the group records == oracle.hist_percentiles of the summed records; one group's sum through gyo_hist_merge
     (the _ref glue has no call that loads a record into a reference histogram);
  2. hosts of 1 024, 1 025 and 2 100 services (one, two and three chunks);
  3. filtered: all four group_by values with and without GYS_RF_ANY_STATE, a term filter, a svcid selection, labels with a GYS_NO_GROUP
     service, a label domain above 4 096, maxrows below the rows; rows == those of gys_rollup_filtered_dev; all-selecting HOST / CLUSTER
     calls == the fixed scopes;
  4. the error codes, no side effects, and an engine that made the calls mid-stream against a twin that did not."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

NONE, HOST, CLUSTER, LABEL = capi.GROUP_NONE, capi.GROUP_HOST, capi.GROUP_CLUSTER, capi.GROUP_LABEL
SCOPES = (capi.ROLLUP_HOST, capi.ROLLUP_CLUSTER, capi.ROLLUP_GLOBAL)
I64MIN = np.iinfo(np.int64).min
NB = 10
T0 = 1_700_000_003
SVCS = [1, 3, 5, 17, 70, 0]
CLUSTER_OF = [0, 1, 0, 1, 0, 2]  # (cluster 2 holds only the service-less host)
PCTS = [25.0, 50.0, 95.0, 99.0]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


class RingOracle:
    """one gyo_mlhist per service (the class of tests/test_gpu_levels.py, close and level only)"""

    def __init__(self, oracle, nsvc):
        self.o, self.L, self.n = oracle, oracle.lib(), nsvc
        self.h = [oracle.MLHist() for _ in range(nsvc)]
        for h in self.h:
            self.L.gyo_mlh_init(C.byref(h), oracle.RESP_TIME_HASH, NB)

    def close(self, t, win_hist):
        for s, h in enumerate(self.h):
            st = np.zeros(16, dtype=self.o.HIST_SERIAL_DT)
            st["count"][:15] = win_hist[s, :15, 0]
            st["sum"][:15] = win_hist[s, :15, 1]
            self.L.gyo_mlh_add_hist(C.byref(h), t, st.ctypes.data, 1)
            self.L.gyo_mlh_flush(C.byref(h), t)

    def level(self, level, tq):
        out = np.zeros((self.n, 15, 2), dtype=np.int64)
        buf = np.zeros(16, dtype=self.o.HIST_SERIAL_DT)
        for s, h in enumerate(self.h):
            hc = self.o.MLHist.from_buffer_copy(h)
            self.L.gyo_mlh_flush(C.byref(hc), tq)
            self.L.gyo_mlh_level(C.byref(hc), level, buf.ctypes.data)
            out[s, :, 0] = buf["count"][:15].astype(np.int64)
            out[s, :, 1] = buf["sum"][:15]
        return out


class World:
    """hosts with svcs[h] services each in cluster cluster_of[h]; the engine, an oracle engine that holds the open window's histograms"""

    def __init__(self, oracle, svcs, cluster_of, seed=1, **kw):
        from gyeeta_amd.engine import SketchEngine
        nh, nsvc = len(svcs), sum(svcs)
        self.svcs, self.cluster_of, self.ncl = svcs, cluster_of, max(cluster_of) + 1
        kw.setdefault("max_services", nsvc + 8)
        self.eng = SketchEngine(max_hosts=nh + 1, max_batch_events=1 << 16, max_clusters=4, **kw)
        self.orc_win = oracle.OracleEngine(kw["max_services"], enable_td=False) if oracle is not None else None
        self.rng = np.random.default_rng(seed)
        for c in range(self.ncl):
            assert self.eng.register_cluster("cluster%d" % c) == c
        self.mid, self.hslot, self.gids, self.slots = {}, {}, {}, {}
        for h, n in enumerate(svcs):
            self.mid[h] = wire.machine_id(h)
            self.hslot[h] = self.eng.register_host(self.mid[h], "cluster%d" % cluster_of[h])
            s = np.arange(n)
            self.gids[h] = wire.glob_id(np.full(n, h), s)
            if n:
                ns, pt = wire.listener_netns(h, s), wire.listener_port(s)
                self.eng.register_listeners_np(self.mid[h], self.gids[h], ns, pt)
                if self.orc_win is not None:
                    for i in range(n):
                        self.orc_win.register(self.hslot[h], int(self.gids[h][i]), int(ns[i]), int(pt[i]))
            self.slots[h] = [self.eng.lookup(int(g)) for g in self.gids[h]]
        self.nsvc = self.eng.num_services()
        assert self.nsvc == nsvc
        self.host_members = {self.hslot[h]: self.slots[h] for h in range(nh)}
        self.cluster_members = {c: [s for h in range(nh) if cluster_of[h] == c for s in self.slots[h]] for c in range(self.ncl)}

    def feed(self, counts, lat_mu=None):
        for h, n in counts.items():
            sp = self.svcs[h]
            if not sp or not n:
                continue
            # (events for the first `live` services only: some services idle in some windows)
            live = int(self.rng.integers(1, sp + 1))
            ev = helpers.make_resp_events(self.rng, h, n, live, lat_mu=float(self.rng.uniform(1.0, 7.0)) if lat_mu is None else lat_mu)
            self.eng.handle_resp_events(self.mid[h], ev)
            if self.orc_win is not None:
                self.orc_win.resp_batch(ev.tobytes(), [self.hslot[h]], [0])

    def states(self, hosts, edit=None):
        for h in hosts:
            if self.svcs[h]:
                r = wire.synth_listener_states(self.rng, h, np.arange(self.svcs[h]))
                if edit:
                    edit(h, r)
                self.kept = getattr(self, "kept", {})
                self.kept[h] = r.copy()  # (the record the engine keeps per service, whatever its age)
                self.eng.partha_listener_state(self.mid[h], r.tobytes(), len(r))


def np_sum(recs):
    """GY_HISTOGRAM::add_histogram over [n][16][2] int64 records (n may be 0)"""
    out = np.zeros((16, 2), dtype=np.int64)
    out[15, 1] = I64MIN
    if len(recs):
        with np.errstate(over="ignore"):
            out = recs.sum(axis=0, dtype=np.int64)
        out[15, 1] = recs[:, 15, 1].max()
    return out


def group_sums(recs, members, ngroups):
    return np.stack([np_sum(recs[members.get(g, [])]) for g in range(ngroups)]) if ngroups else np.zeros((0, 16, 2), dtype=np.int64)


def oracle_merge(oracle, recs):
    """the same sum through gyo_hist_merge, member by member"""
    L = oracle.lib()
    acc = oracle.Hist()
    L.gyo_hist_init(C.byref(acc), oracle.RESP_TIME_HASH)
    for r in recs:
        h = oracle.Hist()
        L.gyo_hist_init(C.byref(h), oracle.RESP_TIME_HASH)
        for b in range(15):
            h.stats[b].count, h.stats[b].sum = int(r[b, 0]), int(r[b, 1])
        h.total_count, h.max_val_seen = int(r[15, 0]), int(r[15, 1])
        L.gyo_hist_merge(C.byref(acc), C.byref(h))
    out = np.zeros((16, 2), dtype=np.int64)
    for b in range(15):
        out[b] = (acc.stats[b].count, acc.stats[b].sum)
    out[15] = (acc.total_count, acc.max_val_seen)
    return out


def check_fixed(w, oracle, tq, levels=(0, 1, 2, 3), ring=None, pcts=False):
    """HOST / CLUSTER / GLOBAL records of `levels` at tq against the numpy sums of the members' exported level records"""
    eng, nh = w.eng, len(w.svcs)
    seen = 0
    for lv in levels:
        tus = tq * 1_000_000 + 1234
        recs = eng.export_hist_level(lv, tus)
        want_h = group_sums(recs, w.host_members, nh)
        want_c = group_sums(recs, w.cluster_members, w.ncl)
        want_g = np_sum(recs)[None]
        got = {}
        for scope, want in zip(SCOPES, (want_h, want_c, want_g)):
            if pcts:
                got[scope], gp = eng.hist_rollup_level(scope, lv, tus, pcts=PCTS)
                for g in range(len(want)):
                    ov, _, _, _ = oracle.hist_percentiles(0, want[g][:15], want[g][15][0], PCTS)
                    assert gp[g].tolist() == ov, (lv, tq, scope, g, gp[g].tolist(), ov)
            else:
                got[scope] = eng.hist_rollup_level(scope, lv, tus)
            bad = np.argwhere(got[scope] != want)
            assert bad.size == 0, f"level {lv} at t={tq} scope {scope}: {bad[:4].tolist()} got {got[scope][tuple(bad[0][:2])]} want {want[tuple(bad[0][:2])]}"
        # the cluster record is the sum of its hosts' records, the rank's record the sum of all hosts'
        hosts_of = {c: [w.hslot[h] for h in range(nh) if w.cluster_of[h] == c] for c in range(w.ncl)}
        assert (group_sums(got[capi.ROLLUP_HOST], hosts_of, w.ncl) == got[capi.ROLLUP_CLUSTER]).all()
        assert (np_sum(got[capi.ROLLUP_HOST]) == got[capi.ROLLUP_GLOBAL][0]).all()
        if ring is not None:
            o = ring.level(lv, tq)
            for g, sl in w.host_members.items():
                assert (got[capi.ROLLUP_HOST][g, :15] == o[sl].sum(axis=0)).all(), (lv, tq, g)
            assert (got[capi.ROLLUP_GLOBAL][0, :15] == o.sum(axis=0)).all(), (lv, tq)
        seen += int(got[capi.ROLLUP_GLOBAL][0, 15, 0] > 0)
    return seen


@pytest.mark.parametrize("enable_td", [True, False], ids=["lazy", "eager"])
def test_fixed_scopes_over_time(torch_mod, oracle, enable_td):
    w = World(oracle, SVCS, CLUSTER_OF, seed=11 + enable_td, enable_tdigest=enable_td, enable_levels=True)
    eng = w.eng
    ring = RingOracle(oracle, w.nsvc) if enable_td else None
    # 5-s steps (T0 + 25 .. T0 + 30 crosses a 30-s boundary, as does the 13-s step), a gap above 300 s, a step over a 12-h boundary
    steps = [5, 5, 5, 5, 5, 5, 13, 5, 311, 5, 43200 - 7, 5]
    t = T0
    seen = np.zeros(4, dtype=np.int64)
    assert check_fixed(w, oracle, t) == 0  # before any close: empty records, max_val_seen = INT64_MIN
    assert (eng.hist_rollup_level(capi.ROLLUP_HOST, 3, 0)[:, 15, 1] == I64MIN).all()
    for k, dt in enumerate(steps):
        t += dt
        if k % 5 != 3:
            w.feed({h: int(w.rng.integers(20, 150)) for h in range(len(SVCS)) if w.rng.random() < 0.8})
        win = np.array(w.orc_win.hist()[:w.nsvc])
        eng.window_close(t * 1_000_000)
        if ring is not None:
            ring.close(t, win)
        w.orc_win.window_clear(clear_hist=True)
        for lv in range(4):
            seen[lv] += check_fixed(w, oracle, t, (lv,), ring, pcts=k % 4 == 1)
        check_fixed(w, oracle, t + 3, ring=ring)
        assert check_fixed(w, oracle, t + 7, (0,), ring) == 0  # level 0 has expired
        check_fixed(w, oracle, t + 7, (1, 2, 3), ring)
        if k in (2, 8):
            # events already ingested into the open window must not count
            w.feed({h: 60 for h in range(len(SVCS))})
            check_fixed(w, oracle, t + 1, ring=ring, pcts=True)
            allrec, openrec = eng.export_hist(1), eng.export_hist(0)
            assert openrec[:, 15, 0].sum() > 0
            g3 = eng.hist_rollup_level(capi.ROLLUP_GLOBAL, 3, (t + 1) * 1_000_000)[0]
            assert (g3[:15] == allrec[:, :15].sum(axis=0) - openrec[:, :15].sum(axis=0)).all()
            assert g3[15, 1] == allrec[:, 15, 1].max()
    assert (seen >= 3).all(), seen
    # one group's sum through the oracle's add_histogram
    tus = t * 1_000_000
    recs = eng.export_hist_level(1, tus)
    assert (eng.hist_rollup_level(capi.ROLLUP_HOST, 1, tus)[w.hslot[4]] == oracle_merge(oracle, recs[w.slots[4]])).all()
    eng.close()


def test_several_chunks(torch_mod):
    svcs = [1024, 1025, 2100]
    w = World(None, svcs, [0, 1, 0], seed=4, max_services=8192, enable_levels=True)
    eng = w.eng
    t = T0
    for k in range(2):
        for h, n in enumerate(svcs):  # (every service of the host may get events)
            ev = helpers.make_resp_events(w.rng, h, 6000, n, lat_mu=3.0 + k)
            eng.handle_resp_events(w.mid[h], ev)
        t += 5
        eng.window_close(t * 1_000_000)
    for lv in (0, 1, 3):
        tus = t * 1_000_000
        recs = eng.export_hist_level(lv, tus)
        got_h, got_g = eng.hist_rollup_level(capi.ROLLUP_HOST, lv, tus), eng.hist_rollup_level(capi.ROLLUP_GLOBAL, lv, tus)
        assert (got_h == group_sums(recs, w.host_members, 3)).all(), lv
        assert (got_g[0] == np_sum(recs)).all() and got_g[0, 15, 0] > 5000, lv
    eng.close()


def _label_of(lm, slot):
    for l, sl in lm.items():
        if slot in sl:
            return l
    return None


def test_filtered(torch_mod):
    w = World(None, SVCS, CLUSTER_OF, seed=21, max_services=6000, enable_levels=True, svc_hll_p=4)
    eng = w.eng
    nh = len(SVCS)
    t = T0
    # host 3 reports its states first and two windows pass (its records go stale); then the others report into the open window
    w.states([3])
    for k in range(2):
        w.feed({h: 100 for h in range(nh)})
        t += 5
        eng.window_close(t * 1_000_000)

    def edit(h, r):
        r["curr_state"] = np.arange(len(r)) % 6

    w.states([h for h in range(nh) if h != 3], edit)
    w.feed({h: 50 for h in range(nh)})  # the open window: in no level
    eng.sync()
    tus = t * 1_000_000
    allslots = {h: w.slots[h] for h in range(nh) if w.slots[h]}
    ids = np.concatenate([w.gids[h] for h in allslots])
    lab = (np.arange(len(ids)) % 5).astype(np.uint32)
    lab[3] = capi.NO_GROUP
    lab[-1] = 5000  # a label domain above 4 096
    eng.set_service_groups(ids, lab)
    lm = {}
    for g, l in zip(ids.tolist(), lab.tolist()):
        if l != capi.NO_GROUP:
            lm.setdefault(l, []).append(eng.lookup(g))
    host_of = {s: h for h in allslots for s in allslots[h]}
    filters = [dict(), dict(terms=[("state", ">=", 3)]), dict(svcids=[int(w.gids[h][k]) for h, k in ((0, 0), (4, 16), (4, 69), (3, 2), (2, 0))] + [4242])]
    checked = 0
    for level in range(4):
        recs = eng.export_hist_level(level, tus)
        for f in filters:
            for any_state in (False, True):
                gs, gh, _, nm = eng.svcstate_scan(f.get("terms"), maxrecs=w.nsvc, svcids=f.get("svcids"))
                if any_state:  # every registered service is a candidate; the terms are evaluated on the kept record, the lists select as before
                    sel = sorted(allslots[h][k] for h in allslots for k in range(len(allslots[h]))
                                 if (not f.get("svcids") or int(w.gids[h][k]) in f["svcids"]) and (not f.get("terms") or int(w.kept[h]["curr_state"][k]) >= 3))
                    assert set(gs.tolist()) == set(sel) - set(w.slots[3])  # (the scan: the same services minus the stale host's)
                else:
                    sel = gs.tolist()
                    assert not set(sel) & set(w.slots[3])  # stale
                for group_by in (NONE, HOST, CLUSTER, LABEL):
                    key = {NONE: lambda s: 0, HOST: lambda s: w.hslot[host_of[s]], CLUSTER: lambda s: w.cluster_of[host_of[s]], LABEL: lambda s: _label_of(lm, s)}[group_by]
                    mem = {}
                    for s in sel:
                        if key(s) is not None:
                            mem.setdefault(key(s), []).append(s)
                    kw = dict(terms=f.get("terms"), svcids=f.get("svcids"), any_state=any_state)
                    rows, nrows, got = eng.hist_rollup_filtered(group_by, level, tus, **kw)
                    rrows, rn, _ = eng.rollup_filtered(group_by, want=("est",), **kw)
                    assert rows == rrows and nrows == rn
                    assert rows == [(g, len(mem[g])) for g in sorted(mem)], (level, f, any_state, group_by, rows[:4])
                    for r, (g, n) in enumerate(rows):
                        assert (got[r] == np_sum(recs[mem[g]])).all(), (level, f, any_state, group_by, g)
                        checked += int(got[r][15, 0] > 0)
        # an all-selecting host / cluster call == the fixed scopes (rows exist for the groups that have a member)
        rows, _, got = eng.hist_rollup_filtered(HOST, level, tus, any_state=True)
        fixed = eng.hist_rollup_level(capi.ROLLUP_HOST, level, tus)
        assert [g for g, _ in rows] == sorted(w.hslot[h] for h in allslots) and (got == fixed[[g for g, _ in rows]]).all()
        rows, _, got = eng.hist_rollup_filtered(CLUSTER, level, tus, any_state=True)
        fixed = eng.hist_rollup_level(capi.ROLLUP_CLUSTER, level, tus)
        assert [g for g, _ in rows] == [0, 1] and (got == fixed[:2]).all() and fixed[2, 15, 1] == I64MIN and not fixed[2, :15].any()
    assert checked > 40
    # maxrows below the rows: the first groups only, the total reported; percentiles of the rows
    full_rows, full_n, full, fp = eng.hist_rollup_filtered(LABEL, 3, tus, any_state=True, pcts=PCTS)
    rows, nrows, got = eng.hist_rollup_filtered(LABEL, 3, tus, any_state=True, maxrows=3)
    assert full_n == nrows == len(lm) == 6 and rows == full_rows[:3] and (got == full[:3]).all() and full_rows[-1] == (5000, 1)
    assert fp.shape == (6, 4) and (fp[:, 0] <= fp[:, 3]).all()
    eng.close()


def test_errors_and_no_side_effects(torch_mod):
    from gyeeta_amd.engine import SketchEngine
    w = World(None, SVCS, CLUSTER_OF, seed=3, enable_levels=True)
    twin = World(None, SVCS, CLUSTER_OF, seed=3, enable_levels=True)
    t = T0
    for x in (w, twin):
        x.states(range(len(SVCS)))
        x.feed({h: 200 for h in range(len(SVCS))})
        x.eng.window_close((t + 5) * 1_000_000)
        x.feed({h: 100 for h in range(len(SVCS))})
        x.eng.sync()
    eng, L = w.eng, w.eng.L
    tus = (t + 6) * 1_000_000

    def snapshot(e):
        return ([x.tobytes() for x in e.export_tdigest()] + [x.tobytes() for x in e.export_tdigest_pending()] +
                [e.export_hist(0).tobytes(), e.export_hist(1).tobytes()] + [e.export_hist_level(lv, tus).tobytes() for lv in range(4)])

    before = snapshot(eng)
    eng.set_service_groups(w.gids[4], np.arange(len(w.gids[4]), dtype=np.uint32) % 3)
    twin.eng.set_service_groups(twin.gids[4], np.arange(len(twin.gids[4]), dtype=np.uint32) % 3)
    for lv in range(4):
        for scope in SCOPES:
            eng.hist_rollup_level(scope, lv, tus)
        for group_by in (NONE, HOST, CLUSTER, LABEL):
            rows, nrows, _ = eng.hist_rollup_filtered(group_by, lv, tus, any_state=True)
            assert nrows == len(rows) > 0
    assert snapshot(eng) == before
    # the calls made mid-stream change nothing that later windows show
    for k in range(2):
        for x in (w, twin):
            x.feed({h: 150 for h in range(len(SVCS))})
            x.eng.window_close((t + 10 + 5 * k) * 1_000_000)
        eng.hist_rollup_level(capi.ROLLUP_CLUSTER, 1, (t + 10 + 5 * k) * 1_000_000)
    tus = (t + 15) * 1_000_000
    assert snapshot(eng) == snapshot(twin.eng)
    twin.eng.close()
    # the error codes
    f, keep = eng._svc_filter(None)
    rows = (capi.RollupRow * 16)()
    n = C.c_uint32()
    recs = torch_mod.zeros((16, 16, 2), dtype=torch_mod.int64, device=eng.device)
    pr = C.c_void_p(recs.data_ptr())

    def fixed(e=eng, scope=capi.ROLLUP_HOST, level=1, out=pr):
        return L.gys_hist_rollup_level_dev(e.h, scope, level, tus, out)

    def filt(e=eng, filt_=C.byref(f), flags=capi.RF_ANY_STATE, group_by=HOST, level=1, rows_=rows, nrows_=C.byref(n), out=pr):
        return L.gys_hist_rollup_filtered_dev(e.h, filt_, flags, group_by, level, tus, rows_, 16, nrows_, out)

    assert fixed() == capi.OK and filt() == capi.OK and n.value == len([x for x in SVCS if x])
    assert fixed(level=4) == capi.ERR_INVAL and fixed(level=-1) == capi.ERR_INVAL and fixed(scope=3) == capi.ERR_INVAL and fixed(scope=-1) == capi.ERR_INVAL
    assert fixed(out=None) == capi.ERR_INVAL
    assert filt(level=4) == capi.ERR_INVAL and filt(level=-1) == capi.ERR_INVAL and filt(group_by=4) == capi.ERR_INVAL and filt(group_by=-1) == capi.ERR_INVAL
    assert filt(flags=2) == capi.ERR_INVAL and filt(filt_=None) == capi.ERR_INVAL and filt(rows_=None) == capi.ERR_INVAL and filt(nrows_=None) == capi.ERR_INVAL
    assert filt(out=None) == capi.ERR_INVAL
    eng.close()
    nolv = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10)
    assert fixed(e=nolv) == capi.ERR_STATE and filt(e=nolv) == capi.ERR_STATE
    nolv.close()
    lv2 = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10, enable_levels=2)
    assert fixed(e=lv2, level=0) == capi.ERR_STATE and filt(e=lv2, level=0) == capi.ERR_STATE
    # without services: GYS_OK and no rows; without a label: a label domain of 0
    n.value = 7
    assert filt(e=lv2, level=1) == capi.OK and n.value == 0
    assert fixed(e=lv2, level=1) == capi.OK and fixed(e=lv2, scope=capi.ROLLUP_GLOBAL, level=3) == capi.OK
    lv2.sync()
    assert not recs[0, :15].any() and int(recs[0, 15, 1]) == I64MIN  # the rank's record without a member
    lv2.close()
    # lists are built without the digests and the registers (enable_tdigest = 0, svc_hll_p = 0), and a label domain of 0 gives no rows
    plain = World(None, [2, 3], [0, 1], seed=2, enable_levels=True, enable_tdigest=False)
    plain.feed({0: 50, 1: 50})
    plain.eng.window_close((t + 5) * 1_000_000)
    r = plain.eng.export_hist_level(3, tus)
    assert (plain.eng.hist_rollup_level(capi.ROLLUP_CLUSTER, 3, tus) == group_sums(r, plain.cluster_members, 2)).all() and r[:, 15, 0].sum() > 0
    assert plain.eng.hist_rollup_filtered(LABEL, 3, tus, any_state=True)[:2] == ([], 0)
    plain.eng.close()
