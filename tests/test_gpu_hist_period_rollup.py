"""Group response-time histograms for any period, group QPS / active-connection histograms and day statistics per group
(gys_hist_rollup_period_dev / _filtered_dev, gys_svc_hist_rollup_dev / _filtered_dev, gys_day_stats_rollup_dev / _filtered_dev; kernel
k_hist_period_union in gyeeta_amd/csrc/gys_histroll.hpp).  The reference sum of every check is computed in numpy from the per-service
exports of the members at the same arguments (gys_export_hist_period: k_level_period, pinned to the ring oracle by tests/test_gpu_levels.py;
gys_export_svc_hist; gys_export_hist_level): counts added as 64-bit words, sums as int64, the maximum on [15][1]; no member: all zero with
max_val_seen = INT64_MIN.  Everything is compared bit for bit; there is no tolerance anywhere.
  1. fixed scopes over time, lazily folded (enable_tdigest) and eager records, the world and the steps of
     tests/test_gpu_hist_rollup.py::test_fixed_scopes_over_time; at every close, 3 s and 7 s later the spans of _check_periods in
     tests/test_gpu_levels.py; HOST / CLUSTER / GLOBAL == the numpy sums, level_used equal, cluster == sum of its hosts; the lazy run also
     against gyo_mlh_period of the per-service ring oracle summed over the members; at least one span per run where the host records differ
     from the shortcut "scale the group's summed ring buckets" (a ring oracle fed the hosts' summed windows); events in the open window do
     not count; percentiles through pcts= == oracle.hist_percentiles of the summed record;
  2. hosts of 1 024, 1 025 and 2 100 services (one, two and three chunks), a whole span and a partly covered one;
  3. filtered: all four group_by values with and without GYS_RF_ANY_STATE, a term filter, an svcid selection, labels with a GYS_NO_GROUP
     service, maxrows below the rows; rows == those of gys_hist_rollup_filtered_dev; all-selecting HOST / CLUSTER calls == the fixed scopes;
  4. group QPS / active-connection histograms == numpy sums of export_svc_hist; day statistics == k_day_stats' rule in numpy on the summed
     records, glob_id = the group index, an empty group: INT64_MIN records and zero statistics;
  5. the error codes, no side effects, and an engine that made every new call mid-stream against a twin that did not."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi
from tests import helpers
from tests.test_gpu_hist_rollup import CLUSTER_OF, PCTS, SVCS, T0, World, _label_of, group_sums, np_sum
from tests.test_gpu_levels import RingOracle

pytestmark = pytest.mark.gpu

NONE, HOST, CLUSTER, LABEL = capi.GROUP_NONE, capi.GROUP_HOST, capi.GROUP_CLUSTER, capi.GROUP_LABEL
SCOPES = (capi.ROLLUP_HOST, capi.ROLLUP_CLUSTER, capi.ROLLUP_GLOBAL)
I64MIN = np.iinfo(np.int64).min
I32MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def period_spans(tq, rng):
    """the spans of _check_periods (tests/test_gpu_levels.py): inside one ring bucket, across several, past the ring, ending in the future,
    one per answering level, and four random ones"""
    spans = [(tq - 4, tq), (tq - 5, tq), (tq - 17, tq - 3), (tq - 60, tq), (tq - 299, tq - 31), (tq - 300, tq), (tq - 301, tq), (tq - 1000, tq - 200),
             (tq - 43200, tq), (tq - 100000, tq - 50000), (tq - 432000, tq + 10), (tq - 432001, tq), (tq - 10**7, tq - 100), (0, tq + 5),
             (tq + 3, tq + 9), (tq - 10**6, tq - 432000 - 50)]
    for _ in range(4):
        a = tq - int(rng.integers(0, 500000))
        spans.append((a, a + int(rng.integers(0, 500000))))
    return spans


def check_fixed(w, oracle, rng, tq, ring=None, gring=None, pcts=False):
    """HOST / CLUSTER / GLOBAL records of every span at tq against the numpy sums of the members' exported period records; returns
    (levels seen with data, spans whose host records differ from scaling the hosts' summed ring buckets)"""
    eng, nh = w.eng, len(w.svcs)
    seen, truncated = set(), 0
    tus = tq * 1_000_000 + 1234
    hosts_of = {c: [w.hslot[h] for h in range(nh) if w.cluster_of[h] == c] for c in range(w.ncl)}
    for a, b in period_spans(tq, rng):
        recs, lv = eng.export_hist_period(a, b, tus)
        wants = (group_sums(recs, w.host_members, nh), group_sums(recs, w.cluster_members, w.ncl), np_sum(recs)[None])
        got = {}
        for scope, want in zip(SCOPES, wants):
            if pcts:
                got[scope], glv, gp = eng.hist_rollup_period(scope, a, b, tus, pcts=PCTS)
                for g in range(len(want)):
                    ov, _, _, _ = oracle.hist_percentiles(0, want[g][:15], want[g][15][0], PCTS)
                    assert gp[g].tolist() == ov, (a - tq, b - tq, scope, g, gp[g].tolist(), ov)
            else:
                got[scope], glv = eng.hist_rollup_period(scope, a, b, tus)
            assert glv == lv, (a - tq, b - tq, scope, glv, lv)
            bad = np.argwhere(got[scope] != want)
            assert bad.size == 0, f"period [{a - tq}, {b - tq}] level {lv} at t={tq} scope {scope}: {bad[:4].tolist()} got {got[scope][tuple(bad[0][:2])]} want {want[tuple(bad[0][:2])]}"
            assert (got[scope][:, 15, 0] == got[scope][:, :15, 0].sum(axis=1)).all()  # total_count = the sum of the group's 15 counts
        # the cluster record is the sum of its hosts' records, the rank's record the sum of all hosts'
        assert (group_sums(got[capi.ROLLUP_HOST], hosts_of, w.ncl) == got[capi.ROLLUP_CLUSTER]).all()
        assert (np_sum(got[capi.ROLLUP_HOST]) == got[capi.ROLLUP_GLOBAL][0]).all()
        if ring is not None:
            o, olv = ring.period(a, b, tq)
            assert olv == lv, (a - tq, b - tq, lv, olv)
            for g, sl in w.host_members.items():
                assert (got[capi.ROLLUP_HOST][g, :15] == o[sl].sum(axis=0)).all(), (a - tq, b - tq, lv, g)
            assert (got[capi.ROLLUP_GLOBAL][0, :15] == o.sum(axis=0)).all(), (a - tq, b - tq, lv)
        if gring is not None and lv in (1, 2):
            # the shortcut: folly's own answer on the series of the hosts' SUMMED windows = the summed ring buckets, scaled once per host
            so, _ = gring.period(a, b, tq)
            truncated += int((got[capi.ROLLUP_HOST][:, :15] != so).any())
        if got[capi.ROLLUP_GLOBAL][0, 15, 0] > 0:
            seen.add(lv)
    return seen, truncated


@pytest.mark.parametrize("enable_td", [True, False], ids=["lazy", "eager"])
def test_fixed_scopes_over_time(torch_mod, oracle, enable_td):
    w = World(oracle, SVCS, CLUSTER_OF, seed=11 + enable_td, enable_tdigest=enable_td, enable_levels=True)
    eng, nh = w.eng, len(SVCS)
    rng = np.random.default_rng(5)
    ring = RingOracle(oracle, w.nsvc) if enable_td else None
    gring = RingOracle(oracle, nh)  # one series per host slot, fed the hosts' summed windows: the shortcut the group records must NOT equal
    steps = [5, 5, 5, 5, 5, 5, 13, 5, 311, 5, 43200 - 7, 5]
    t = T0
    seen, truncated = set(), 0
    s0, _ = check_fixed(w, oracle, rng, t)  # before any close: empty records, max_val_seen = INT64_MIN
    assert not s0 and (eng.hist_rollup_period(capi.ROLLUP_HOST, 0, t, 0)[0][:, 15, 1] == I64MIN).all()
    for k, dt in enumerate(steps):
        t += dt
        if k % 5 != 3:
            w.feed({h: int(w.rng.integers(20, 150)) for h in range(nh) if w.rng.random() < 0.8})
        win = np.array(w.orc_win.hist()[:w.nsvc])
        eng.window_close(t * 1_000_000)
        if ring is not None:
            ring.close(t, win)
        gwin = np.zeros((nh, 16, 2), dtype=np.int64)
        for g, sl in w.host_members.items():
            gwin[g] = win[sl].sum(axis=0) if sl else 0
        gring.close(t, gwin)
        w.orc_win.window_clear(clear_hist=True)
        for dq in (0, 3, 7):
            s, tr = check_fixed(w, oracle, rng, t + dq, ring if dq == 0 or k % 3 == 0 else None, gring, pcts=dq == 0 and k % 4 == 1)
            seen |= s
            truncated += tr
        if k in (2, 8):
            # events already ingested into the open window must not count
            tus = (t + 1) * 1_000_000
            before = [eng.hist_rollup_period(capi.ROLLUP_GLOBAL, a, b, tus)[0] for a, b in ((t - 60, t + 1), (t - 3, t + 1), (0, t + 5))]
            w.feed({h: 60 for h in range(nh)})
            assert eng.export_hist(0)[:, 15, 0].sum() > 0
            after = [eng.hist_rollup_period(capi.ROLLUP_GLOBAL, a, b, tus)[0] for a, b in ((t - 60, t + 1), (t - 3, t + 1), (0, t + 5))]
            print("closed-window totals before / after the open window's events:", [int(x[0, 15, 0]) for x in before], [int(y[0, 15, 0]) for y in after])
            assert all((x[:, :15] == y[:, :15]).all() for x, y in zip(before, after))
            assert before[2][0, 15, 0] > 0  # (the since-start span: every closed window)
            check_fixed(w, oracle, rng, t + 1, ring, pcts=True)
    assert seen == {0, 1, 2, 3}, seen
    assert truncated > 0  # the test can tell the per-member rule from scaling the group's summed ring buckets
    eng.close()


def test_several_chunks(torch_mod):
    svcs = [1024, 1025, 2100]
    w = World(None, svcs, [0, 1, 0], seed=4, max_services=8192, enable_levels=True)
    eng = w.eng
    t = T0
    for k in range(2):  # closes at T0 + 5 and T0 + 10: either side of a 30-s boundary (T0 % 30 == 23)
        for h, n in enumerate(svcs):  # (every service of the host may get events)
            ev = helpers.make_resp_events(w.rng, h, 6000, n, lat_mu=3.0 + k)
            eng.handle_resp_events(w.mid[h], ev)
        t += 5
        eng.window_close(t * 1_000_000)
    tus = t * 1_000_000
    scaled = 0
    for a, b, want_lv in ((t - 60, t, 1), (t - 7, t - 2, 1), (0, t + 5, 3)):  # whole ring buckets; two partly covered ones; since start
        recs, lv = eng.export_hist_period(a, b, tus)
        assert lv == want_lv
        got_h, lh = eng.hist_rollup_period(capi.ROLLUP_HOST, a, b, tus)
        got_c, _ = eng.hist_rollup_period(capi.ROLLUP_CLUSTER, a, b, tus)
        got_g, lg = eng.hist_rollup_period(capi.ROLLUP_GLOBAL, a, b, tus)
        assert lh == lg == lv
        assert (got_h == group_sums(recs, w.host_members, 3)).all(), (a, b)
        assert (got_c == group_sums(recs, w.cluster_members, 2)).all(), (a, b)
        assert (got_g[0] == np_sum(recs)).all() and got_g[0, 15, 0] > (5000 if a != t - 7 else 500), (a, b, got_g[0, 15, 0])
        whole = eng.hist_rollup_period(capi.ROLLUP_HOST, t - 60, t, tus)[0]
        scaled += int(a == t - 7 and (got_h[:, 15, 0] < whole[:, 15, 0]).all())
    assert scaled == 1  # (the partly covered span saw less than the whole buckets: the scales were applied)
    eng.close()


def test_filtered(torch_mod):
    w = World(None, SVCS, CLUSTER_OF, seed=21, enable_levels=True)
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
    w.feed({h: 50 for h in range(nh)})  # the open window: in no period
    eng.sync()
    tus = t * 1_000_000
    allslots = {h: w.slots[h] for h in range(nh) if w.slots[h]}
    ids = np.concatenate([w.gids[h] for h in allslots])
    lab = (np.arange(len(ids)) % 5).astype(np.uint32)
    lab[3] = capi.NO_GROUP
    eng.set_service_groups(ids, lab)
    lm = {}
    for g, l in zip(ids.tolist(), lab.tolist()):
        if l != capi.NO_GROUP:
            lm.setdefault(l, []).append(eng.lookup(g))
    host_of = {s: h for h in allslots for s in allslots[h]}
    filters = [dict(), dict(terms=[("state", ">=", 3)]), dict(svcids=[int(w.gids[h][k]) for h, k in ((0, 0), (4, 16), (4, 69), (3, 2), (2, 0))] + [4242])]
    spans = [(t - 60, t), (t - 7, t - 2), (t - 4, t)]  # level 1 whole, level 1 partly covered, level 0
    checked = 0
    for a, b in spans:
        recs, lv = eng.export_hist_period(a, b, tus)
        for f in filters:
            for any_state in (False, True):
                kw = dict(terms=f.get("terms"), svcids=f.get("svcids"), any_state=any_state)
                for group_by in (NONE, HOST, CLUSTER, LABEL):
                    lrows, ln, _ = eng.hist_rollup_filtered(group_by, 1, tus, **kw)
                    rows, nrows, got, glv = eng.hist_rollup_period_filtered(group_by, a, b, tus, **kw)
                    assert rows == lrows and nrows == ln and glv == lv
                    # the members of the rows: the services the filter selects (the scan's, or with any_state every candidate), by group
                    gs = eng.svcstate_scan(f.get("terms"), maxrecs=w.nsvc, svcids=f.get("svcids"))[0].tolist()
                    if any_state:
                        gs = sorted(allslots[h][k] for h in allslots for k in range(len(allslots[h]))
                                    if (not f.get("svcids") or int(w.gids[h][k]) in f["svcids"]) and (not f.get("terms") or int(w.kept[h]["curr_state"][k]) >= 3))
                    key = {NONE: lambda s: 0, HOST: lambda s: w.hslot[host_of[s]], CLUSTER: lambda s: w.cluster_of[host_of[s]], LABEL: lambda s: _label_of(lm, s)}[group_by]
                    mem = {}
                    for s in gs:
                        if key(s) is not None:
                            mem.setdefault(key(s), []).append(s)
                    assert rows == [(g, len(mem[g])) for g in sorted(mem)], (a, b, f, any_state, group_by, rows[:4])
                    for r, (g, n) in enumerate(rows):
                        assert (got[r] == np_sum(recs[mem[g]])).all(), (a, b, f, any_state, group_by, g)
                        checked += int(got[r][15, 0] > 0)
        # an all-selecting host / cluster call == the fixed scopes (rows exist for the groups that have a member)
        rows, _, got, _ = eng.hist_rollup_period_filtered(HOST, a, b, tus, any_state=True)
        fixed, _ = eng.hist_rollup_period(capi.ROLLUP_HOST, a, b, tus)
        assert [g for g, _ in rows] == sorted(w.hslot[h] for h in allslots) and (got == fixed[[g for g, _ in rows]]).all()
        rows, _, got, _ = eng.hist_rollup_period_filtered(CLUSTER, a, b, tus, any_state=True)
        fixed, _ = eng.hist_rollup_period(capi.ROLLUP_CLUSTER, a, b, tus)
        assert [g for g, _ in rows] == [0, 1] and (got == fixed[:2]).all() and fixed[2, 15, 1] == I64MIN and not fixed[2, :15].any()
    assert checked > 40
    # maxrows below the rows: the first groups only, the total reported; percentiles of the rows
    full_rows, full_n, full, _, fp = eng.hist_rollup_period_filtered(LABEL, t - 60, t, tus, any_state=True, pcts=PCTS)
    rows, nrows, got, _ = eng.hist_rollup_period_filtered(LABEL, t - 60, t, tus, any_state=True, maxrows=3)
    assert full_n == nrows == len(lm) == 5 and rows == full_rows[:3] and (got == full[:3]).all()
    assert fp.shape == (5, 4) and (fp[:, 0] <= fp[:, 3]).all()
    eng.close()


def day_stats_rule(oracle, glob_id, r, q, a):
    """k_day_stats' rule on one group's 5-day response record r, QPS record q and active-connection record a ([16][2] int64)"""
    L = oracle.lib()
    if q[15, 1] == I64MIN:  # no member
        return (glob_id, 0, 0, 0, 0, 0, 0, 0, 0)
    cnt = np.ascontiguousarray(r[:15, 0]).astype(np.uint64)
    resp = [max(0, L.gyo_bucket_max_threshold(0, L.gyo_slab_percentile_idx(oracle.ptr(cnt, oracle.u64p), 15, p / 100.0))) for p in (95.0, 25.0)]
    qv = oracle.hist_percentiles(oracle.KINDS["SEMI_LOG_HASH_LO"], q[:15], q[15][0], [95.0, 25.0])[0]
    av = oracle.hist_percentiles(oracle.KINDS["HASH_1_3000"], a[:15], a[15][0], [95.0, 25.0])[0]
    return (glob_id, int(r[15, 0]), int(r[:15, 1].sum()), resp[0], resp[1]) + tuple(v & 0xFFFFFFFF for v in qv + av)


def test_svc_hists_and_day_stats(torch_mod, oracle):
    w = World(None, SVCS, CLUSTER_OF, seed=9, enable_levels=True)
    eng, nh = w.eng, len(SVCS)
    t = T0
    for k in range(6):
        w.feed({h: 300 for h in range(nh)})
        w.states([h for h in range(nh) if h != 1 and (h != 2 or k % 2)])  # host 1 never reports; host 2 every other window
        t += 5
        eng.window_close(t * 1_000_000)
    tus = t * 1_000_000
    ids = np.concatenate([w.gids[h] for h in range(nh) if w.svcs[h]])
    lab = (np.arange(len(ids)) % 4).astype(np.uint32) + 2  # (labels 2 .. 5: glob_id is the row's group, not its index)
    eng.set_service_groups(ids, lab)
    lm = {}
    for g, l in zip(ids.tolist(), lab.tolist()):
        lm.setdefault(l, []).append(eng.lookup(g))
    members = {capi.ROLLUP_HOST: (w.host_members, nh), capi.ROLLUP_CLUSTER: (w.cluster_members, w.ncl), capi.ROLLUP_GLOBAL: ({0: list(range(w.nsvc))}, 1)}
    svc = [eng.export_svc_hist(0), eng.export_svc_hist(1)]
    lvl2 = eng.export_hist_level(2, tus)
    assert svc[0][:, 15, 0].sum() > 0 and svc[1][:, 15, 0].sum() > 0 and (svc[0][w.slots[1], 15, 1] == I32MIN).all()
    for scope in SCOPES:
        mem, ng = members[scope]
        want = [group_sums(svc[which], mem, ng) for which in (0, 1)]
        for which in (0, 1):
            got, gp = eng.svc_hist_rollup(scope, which, pcts=PCTS)
            assert (got == want[which]).all(), (scope, which)
            for g in range(ng):
                ov = oracle.hist_percentiles(oracle.KINDS["HASH_1_3000" if which else "SEMI_LOG_HASH_LO"], want[which][g][:15], want[which][g][15][0], PCTS)[0]
                assert gp[g].tolist() == ov, (scope, which, g)
        ds = eng.day_stats_rollup(scope, tus)
        r5 = group_sums(lvl2, mem, ng)
        assert len(ds) == ng
        for g in range(ng):
            assert tuple(int(x) for x in ds[g]) == day_stats_rule(oracle, g, r5[g], want[0][g], want[1][g]), (scope, g, ds[g])
    # a host whose services never reported: INT32_MIN, the maximum gys_create leaves; an empty group: INT64_MIN records and zero statistics
    hq = eng.svc_hist_rollup(capi.ROLLUP_HOST, 0)
    assert hq[w.hslot[1], 15, 1] == I32MIN and not hq[w.hslot[1], :15].any()
    assert hq[w.hslot[5], 15, 1] == I64MIN and not hq[w.hslot[5], :15].any() and not hq[w.hslot[5], 15, 0]
    assert eng.svc_hist_rollup(capi.ROLLUP_CLUSTER, 1)[2, 15, 1] == I64MIN
    ds = eng.day_stats_rollup(capi.ROLLUP_HOST, tus)
    assert tuple(int(x) for x in ds[w.hslot[5]]) == (w.hslot[5], 0, 0, 0, 0, 0, 0, 0, 0)
    assert ds["tcount_5d"].sum() > 0 and ds["p95_qps"][w.hslot[4]] > 0
    # filtered: rows as gys_hist_rollup_filtered_dev gives them, records and statistics of the rows' members
    host_of = {s: h for h in range(nh) for s in w.slots[h]}
    for group_by, mem in ((NONE, {0: list(range(w.nsvc))}), (HOST, {w.hslot[h]: w.slots[h] for h in range(nh) if w.slots[h]}),
                          (CLUSTER, {c: m for c, m in w.cluster_members.items() if m}), (LABEL, lm)):
        lrows, ln, _ = eng.hist_rollup_filtered(group_by, 2, tus, any_state=True)
        assert lrows == [(g, len(mem[g])) for g in sorted(mem)]
        want = []
        for which in (0, 1):
            rows, nrows, got = eng.svc_hist_rollup_filtered(group_by, which, any_state=True)
            assert rows == lrows and nrows == ln
            want.append(np.stack([np_sum(svc[which][mem[g]]) for g, _ in rows]))
            assert (got == want[which]).all(), (group_by, which)
        rows, nrows, ds = eng.day_stats_rollup_filtered(group_by, tus, any_state=True)
        assert rows == lrows and nrows == ln and len(ds) == len(rows)
        for r, (g, _) in enumerate(rows):
            assert tuple(int(x) for x in ds[r]) == day_stats_rule(oracle, g, np_sum(lvl2[mem[g]]), want[0][r], want[1][r]), (group_by, g)
    # without GYS_RF_ANY_STATE only the services with a fresh record; maxrows below the rows
    gs = eng.svcstate_scan(None, maxrecs=w.nsvc)[0].tolist()
    rows, nrows, got = eng.svc_hist_rollup_filtered(HOST, 0)
    hm = {}
    for s in gs:
        hm.setdefault(w.hslot[host_of[s]], []).append(s)
    assert rows == [(g, len(hm[g])) for g in sorted(hm)] and all((got[r] == np_sum(svc[0][hm[g]])).all() for r, (g, _) in enumerate(rows))
    rows, nrows, ds = eng.day_stats_rollup_filtered(LABEL, tus, any_state=True, maxrows=2)
    assert nrows == 4 and [g for g, _ in rows] == [2, 3] and ds["glob_id"].tolist() == [2, 3]
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
                [e.export_hist(0).tobytes(), e.export_hist(1).tobytes(), e.export_svc_hist(0).tobytes(), e.export_svc_hist(1).tobytes()] +
                [e.export_hist_level(lv, tus).tobytes() for lv in range(4)] + [e.export_hist_period(t - 100, t + 6, tus)[0].tobytes(), bytes(e.export_day_stats(tus))])

    def every_new_call(e, tu, tq):
        for scope in SCOPES:
            for a, b in ((tq - 3, tq), (tq - 100, tq - 2), (0, tq)):
                e.hist_rollup_period(scope, a, b, tu)
            e.svc_hist_rollup(scope, 0)
            e.svc_hist_rollup(scope, 1)
            e.day_stats_rollup(scope, tu)
        for group_by in (NONE, HOST, CLUSTER, LABEL):
            rows, nrows, _, _ = e.hist_rollup_period_filtered(group_by, tq - 100, tq - 2, tu, any_state=True)
            assert nrows == len(rows) > 0
            assert e.svc_hist_rollup_filtered(group_by, 1, any_state=True)[0] == rows
            assert e.day_stats_rollup_filtered(group_by, tu, any_state=True)[0] == rows

    before = snapshot(eng)
    eng.set_service_groups(w.gids[4], np.arange(len(w.gids[4]), dtype=np.uint32) % 3)
    twin.eng.set_service_groups(twin.gids[4], np.arange(len(twin.gids[4]), dtype=np.uint32) % 3)
    every_new_call(eng, tus, t + 6)
    assert snapshot(eng) == before
    # the calls made mid-stream change nothing that later windows show
    for k in range(2):
        for x in (w, twin):
            x.feed({h: 150 for h in range(len(SVCS))})
            x.states(range(len(SVCS)))
            x.eng.window_close((t + 10 + 5 * k) * 1_000_000)
        every_new_call(eng, (t + 10 + 5 * k) * 1_000_000, t + 10 + 5 * k)
    tus = (t + 15) * 1_000_000
    assert snapshot(eng) == snapshot(twin.eng)
    twin.eng.close()
    # the error codes
    f, keep = eng._svc_filter(None)
    rows = (capi.RollupRow * 16)()
    n = C.c_uint32()
    lvu = C.c_int(-1)
    recs = torch_mod.zeros((16, 16, 2), dtype=torch_mod.int64, device=eng.device)
    pr = C.c_void_p(recs.data_ptr())

    def period(e=eng, scope=capi.ROLLUP_HOST, out=pr, lv=C.byref(lvu)):
        return L.gys_hist_rollup_period_dev(e.h, scope, t - 100, t + 6, tus, out, lv)

    def period_f(e=eng, filt_=C.byref(f), flags=capi.RF_ANY_STATE, group_by=HOST, rows_=rows, nrows_=C.byref(n), out=pr, lv=C.byref(lvu)):
        return L.gys_hist_rollup_period_filtered_dev(e.h, filt_, flags, group_by, t - 100, t + 6, tus, rows_, 16, nrows_, out, lv)

    def svch(e=eng, scope=capi.ROLLUP_HOST, which=0, out=pr):
        return L.gys_svc_hist_rollup_dev(e.h, scope, which, out)

    def svch_f(e=eng, filt_=C.byref(f), flags=capi.RF_ANY_STATE, group_by=HOST, which=0, rows_=rows, nrows_=C.byref(n), out=pr):
        return L.gys_svc_hist_rollup_filtered_dev(e.h, filt_, flags, group_by, which, rows_, 16, nrows_, out)

    def days(e=eng, scope=capi.ROLLUP_HOST, out=pr):
        return L.gys_day_stats_rollup_dev(e.h, scope, tus, out)

    def days_f(e=eng, filt_=C.byref(f), flags=capi.RF_ANY_STATE, group_by=HOST, rows_=rows, nrows_=C.byref(n), out=pr):
        return L.gys_day_stats_rollup_filtered_dev(e.h, filt_, flags, group_by, tus, rows_, 16, nrows_, out)

    nlive = len([x for x in SVCS if x])
    for fixed, filt in ((period, period_f), (svch, svch_f), (days, days_f)):
        assert fixed() == capi.OK and filt() == capi.OK and n.value == nlive
        assert fixed(scope=3) == capi.ERR_INVAL and fixed(scope=-1) == capi.ERR_INVAL and fixed(out=None) == capi.ERR_INVAL
        assert filt(group_by=4) == capi.ERR_INVAL and filt(group_by=-1) == capi.ERR_INVAL and filt(flags=2) == capi.ERR_INVAL
        assert filt(filt_=None) == capi.ERR_INVAL and filt(rows_=None) == capi.ERR_INVAL and filt(nrows_=None) == capi.ERR_INVAL and filt(out=None) == capi.ERR_INVAL
    assert svch(which=2) == capi.ERR_INVAL and svch(which=-1) == capi.ERR_INVAL and svch_f(which=2) == capi.ERR_INVAL and svch_f(which=-1) == capi.ERR_INVAL
    assert period(lv=None) == capi.OK and period_f(lv=None) == capi.OK  # level_used may be NULL
    assert lvu.value == 1
    eng.close()
    nolv = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10)
    for call in (period, period_f, svch, svch_f, days, days_f):
        assert call(e=nolv) == capi.ERR_STATE
    nolv.close()
    # enable_levels = 2: no 5-s level, the 300-s ring answers; without services: GYS_OK and no rows, the rank's record that of no member
    lv2 = SketchEngine(max_hosts=2, max_services=4, max_batch_events=1 << 10, enable_levels=2)
    n.value = 7
    assert period_f(e=lv2) == capi.OK and n.value == 0
    n.value = 7
    assert svch_f(e=lv2) == capi.OK and n.value == 0
    n.value = 7
    assert days_f(e=lv2) == capi.OK and n.value == 0
    assert L.gys_hist_rollup_period_dev(lv2.h, capi.ROLLUP_GLOBAL, t + 3, t + 6, tus, pr, C.byref(lvu)) == capi.OK and lvu.value == 1
    assert period(e=lv2) == capi.OK and svch(e=lv2) == capi.OK and days(e=lv2) == capi.OK
    lv2.sync()
    assert not recs[0, :15].any() and int(recs[0, 15, 1]) == I64MIN  # the rank's record without a member
    lv2.close()
