"""Issue resolution on the GPU (gyeeta_amd/csrc/gys_svcresol.hpp): gys_svc_resolve_issues / _dev against a level-by-level search in
Python written here from the definition ("Issue resolution" in include/gysketch.h).  States are set by LISTENER_STATE_NOTIFY records with
chosen curr_state / curr_issue, the graph by ACTIVE_CONN_STATS rows and gys_set_listener_tasks.  Every comparison is exact: all
gys_num_services records, the stats, the impact column (NaN positions included) and the host rows."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

RING = 3  # GYS_ACT_RING
T0 = 1_700_000_000_000_000
IDLE, GOOD, OK, BAD, SEVERE, DOWN = range(6)
DEP = 7  # ISSUE_DEPENDENT_SERVER_LISTENER
NOSLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


class World:
    """an engine, and the model beside it: the registry (glob_id -> slot, host), the bindings (every listener a task group of its own
    unless bound otherwise), the live rows and the kept state of every slot"""

    def __init__(self, nh, sp, cap=4096, spare=4):
        from gyeeta_amd.engine import SketchEngine
        self.eng = SketchEngine(max_hosts=nh, max_services=nh * sp + spare, enable_tdigest=False, actconn_pair_cap=cap)
        self.info, self.gids = helpers.register_world(self.eng, None, range(nh), sp)
        self.svc = [int(g) for h in range(nh) for g in self.gids[h]]
        self.host_of = {int(g): h for h in range(nh) for g in self.gids[h]}
        self.slot_of = {g: self.eng.lookup(g) for g in self.svc}
        self.task = {g: 0xA000 + self.slot_of[g] for g in self.svc}
        self.rows = {}   # (listener id, client task) -> window of the last report
        self.kept = {}   # glob_id -> (state, issue, window) or None (a delete record)
        self.epoch = 1
        self.nclose = 0
        if cap:
            self.bind()

    def close_engine(self):
        self.eng.close()

    def bind(self):
        assert self.eng.set_listener_tasks(list(self.task), list(self.task.values())) == capi.OK

    def calls(self, pairs):
        """pairs of (caller id, callee id): one row per pair naming the caller's task group as the client"""
        n = len(pairs)
        rec = np.zeros(n, dtype=wire.ACTIVE_CONN_STATS)
        rec["listener_glob_id"] = np.array([v for _u, v in pairs], dtype=np.uint64)
        rec["cli_aggr_task_id"] = np.array([self.task[u] for u, _v in pairs], dtype=np.uint64)
        rec["active_conns"] = 1
        self.eng.handle_partha_active_conns(self.info[0][0], rec.tobytes(), n)
        for u, v in pairs:
            self.rows[(v, self.task[u])] = self.epoch

    def states(self, items):
        """items: glob_id -> (state, issue), or None for a LISTEN_FLAG_DELETE record"""
        by_host = {}
        for g, v in items.items():
            by_host.setdefault(self.host_of[g], []).append((g, v))
        for h, lst in by_host.items():
            for i in range(0, len(lst), 512):
                part = lst[i:i + 512]
                rec = np.zeros(len(part), dtype=wire.LISTENER_STATE_NOTIFY)
                rec["glob_id"] = np.array([g for g, _ in part], dtype=np.uint64)
                rec["curr_state"] = [v[0] if v else 0 for _, v in part]
                rec["curr_issue"] = [v[1] if v else 0 for _, v in part]
                rec["query_flags"] = [0 if v else wire.LISTEN_FLAG_DELETE for _, v in part]
                rec["nqrys_5s"] = 10
                self.eng.partha_listener_state(self.info[h][0], rec.tobytes(), len(part))
        for g, v in items.items():
            if v is None:
                self.kept[g] = None
            elif v[0] <= 5:  # (a record with a state above 5 is skipped by the ingest: what was kept stays)
                self.kept[g] = (v[0], v[1], self.epoch)

    def window_close(self):
        self.eng.window_close(T0 + self.nclose * 5_000_000)
        self.nclose += 1
        self.epoch += 1

    def delete(self, gid):
        assert self.eng.delete_listeners([gid]) == 1
        del self.slot_of[gid]
        self.kept.pop(gid, None)
        self.task.pop(gid, None)

    # ---- the definition
    def edges(self):
        bound = {}
        for g, t in self.task.items():
            if g in self.slot_of:
                bound.setdefault(t, []).append(self.slot_of[g])
        out, n = set(), 0
        for (lid, cid), win in self.rows.items():
            if self.epoch - win > RING or lid not in self.slot_of or cid not in bound:
                continue
            for u in bound[cid]:
                out.add((u, self.slot_of[lid]))
                n += 1
        return out, n

    def kept_states(self):
        """slot -> (state, issue) of the slots with a current record"""
        st = {}
        for g, v in self.kept.items():
            if v is not None and g in self.slot_of and v[2] + 1 >= self.epoch:
                st[self.slot_of[g]] = (v[0], v[1])
        return st


def klass(st, s):
    if s not in st or st[s][0] > 5:
        return "none"
    state, issue = st[s]
    if state >= 3:
        return "dep" if issue == DEP else "src"
    return "ok" if state == 2 else "opaque"


def model(eng, nsvc, st, edges, nedges, max_tiers):
    """level by level from the definition -> (records, impact, stats, slots whose candidates at their tier named different sources)"""
    tiers = max_tiers or 8
    cl = {s: klass(st, s) for s in range(nsvc)}
    tier = {s: 0 for s in range(nsvc) if cl[s] == "src"}
    src = {s: s for s in tier}
    via = {}
    competing = 0
    for t in range(tiers):
        cand = {}
        for u, v in edges:
            if tier.get(v) == t and u not in tier and cl[u] in ("dep", "ok"):
                cand.setdefault(u, set()).add((src[v], v))
        for u, c in cand.items():
            tier[u] = t + 1
            src[u], via[u] = min(c)
            competing += len({a for a, _ in c}) > 1
    rec = np.zeros(nsvc, dtype=eng.SVC_RESOL_DT)
    rec["src_slot"] = rec["via_slot"] = NOSLOT
    stats = dict(with_state=0, sources=0, resolved=0, unresolved=0, carriers=0, edges=nedges, resolved_at_tier=[0] * 8)
    for s in range(nsvc):
        r = rec[s]
        if cl[s] != "none":
            r["state"], r["issue"] = st[s]
            stats["with_state"] += 1
        if cl[s] == "src":
            r["role"], r["src_slot"] = capi.RS_SOURCE, s
            stats["sources"] += 1
        elif s in tier:
            r["role"] = capi.RS_RESOLVED if cl[s] == "dep" else capi.RS_CARRIER
            r["tier"], r["src_slot"], r["via_slot"] = tier[s], src[s], via[s]
            if cl[s] == "dep":
                stats["resolved"] += 1
                stats["resolved_at_tier"][tier[s] - 1] += 1
                rec[src[s]]["nresolved"] += 1
            else:
                stats["carriers"] += 1
        elif cl[s] == "dep":
            r["role"] = capi.RS_UNRESOLVED
            stats["unresolved"] += 1
    impact = np.where(rec["role"] == capi.RS_SOURCE, rec["nresolved"].astype(np.float64), np.nan)
    return rec, impact, stats, competing


def check(w, dec=None, dec_states=None, max_tiers=0, masks=(0, 0x1F, 0x02, 0x14)):
    """both forms against the model; dec (numpy DECISION_DT) replaces the kept states, dec_states = what the definition sees then"""
    eng = w.eng
    nsvc = eng.num_services()
    edges, nedges = w.edges()
    st = w.kept_states() if dec is None else dec_states
    rec, impact, stats, competing = model(eng, nsvc, st, edges, nedges, max_tiers)
    got, gimp, gst = eng.resolve_issues_np(dec, max_tiers)
    bad = np.flatnonzero(got != rec)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], rec[bad[:8]])
    assert got.tobytes() == rec.tobytes()
    assert gst == stats, (gst, stats)
    assert np.array_equal(np.isnan(gimp), np.isnan(impact)) and np.array_equal(gimp[~np.isnan(impact)], impact[~np.isnan(impact)])
    gid_of = {s: g for g, s in w.slot_of.items()}
    for mask in masks:
        want = [s for s in range(nsvc) if ((mask or 0x1E) >> int(rec[s]["role"])) & 1]
        rc, rows, nmatch, rst = eng.resolve_issues(dec, max_tiers, mask)
        assert rc == capi.OK and nmatch == len(want) and rst == stats, (mask, rc, nmatch, len(want))
        exp = np.zeros(len(want), dtype=eng.SVC_RESOL_ROW_DT)
        for i, s in enumerate(want):
            r, e = rec[s], exp[i]
            e["glob_id"], e["slot"] = gid_of.get(s, 0), s
            for f in ("src_slot", "via_slot", "nresolved", "role", "tier", "state", "issue"):
                e[f] = r[f]
            if r["src_slot"] != NOSLOT:
                e["src_glob_id"], e["src_state"], e["src_issue"] = gid_of[int(r["src_slot"])], rec[r["src_slot"]]["state"], rec[r["src_slot"]]["issue"]
            if r["via_slot"] != NOSLOT:
                e["via_glob_id"] = gid_of[int(r["via_slot"])]
        assert rows.tobytes() == exp.tobytes(), (mask, np.flatnonzero(rows != exp)[:8])
        if want:
            rc, rows, nmatch, rst = eng.resolve_issues(dec, max_tiers, mask, cap=len(want) - 1)
            assert rc == capi.ERR_NOMEM and nmatch == len(want) and len(rows) == 0 and rst == stats
    return rec, stats, competing


def chain(w, ids):
    """ids[0] <- ids[1] <- ...: every service calls the one in front of it"""
    w.calls([(ids[i + 1], ids[i]) for i in range(len(ids) - 1)])


def test_tier_cap(torch_mod):
    w = World(2, 8)
    try:
        s = w.svc[:11]
        sl = [w.slot_of[g] for g in s]
        chain(w, s)
        w.states({s[0]: (BAD, 2), **{g: (BAD, DEP) for g in s[1:]}})
        rec, st, _ = check(w)
        for i in range(1, 9):
            assert tuple(rec[sl[i]][["role", "tier", "src_slot", "via_slot"]]) == (capi.RS_RESOLVED, i, sl[0], sl[i - 1])
        assert rec[sl[9]]["role"] == rec[sl[10]]["role"] == capi.RS_UNRESOLVED and rec[sl[0]]["nresolved"] == 8 and st["resolved_at_tier"] == [1] * 8
        rec3, st3, _ = check(w, max_tiers=3)
        assert [int(rec3[x]["role"]) for x in sl] == [capi.RS_SOURCE] + [capi.RS_RESOLVED] * 3 + [capi.RS_UNRESOLVED] * 7 and st3["unresolved"] == 7
        rec8, st8, _ = check(w, max_tiers=8)
        assert rec8.tobytes() == rec.tobytes() and st8 == st
        d = torch_mod.zeros(1024, dtype=torch_mod.uint8, device=w.eng.device)
        assert w.eng.L.gys_svc_resolve_issues_dev(w.eng.h, None, 9, C.c_void_p(d.data_ptr()), None, None) == capi.ERR_INVAL
        n32, m32 = C.c_uint32(), C.c_uint32()
        assert w.eng.L.gys_svc_resolve_issues(w.eng.h, None, 9, 0, None, 0, C.byref(n32), C.byref(m32), None) == capi.ERR_INVAL
    finally:
        w.close_engine()


def test_ties_and_distance(torch_mod):
    w = World(2, 12)
    try:
        g, sl = w.svc, w.slot_of
        # two sources at equal distance: 9 calls 5 and 2
        w.calls([(g[9], g[5]), (g[9], g[2])])
        # one source through two neighbours: 13 calls 12 and 11, both call 10
        w.calls([(g[12], g[10]), (g[11], g[10]), (g[13], g[12]), (g[13], g[11])])
        # a nearer source beats a lower-numbered farther one: 17 -> 16 -> 15 -> 14 (source), 17 -> 18 (source)
        w.calls([(g[15], g[14]), (g[16], g[15]), (g[17], g[16]), (g[17], g[18])])
        w.states({g[i]: (BAD, 1) for i in (5, 2, 10, 14, 18)})
        w.states({g[i]: (SEVERE, DEP) for i in (9, 11, 12, 13, 15, 16, 17)})
        rec, _, competing = check(w)
        assert (rec[sl[g[9]]]["src_slot"], rec[sl[g[9]]]["via_slot"]) == (sl[g[2]], sl[g[2]])
        assert (rec[sl[g[13]]]["src_slot"], rec[sl[g[13]]]["via_slot"], rec[sl[g[13]]]["tier"]) == (sl[g[10]], sl[g[11]], 2)
        assert (rec[sl[g[17]]]["src_slot"], rec[sl[g[17]]]["tier"]) == (sl[g[18]], 1)
        assert competing == 1
    finally:
        w.close_engine()


def test_a_task_group_of_70_and_1500_callers_of_two_sources(torch_mod):
    w = World(4, 450)
    try:
        g, sl = w.svc, w.slot_of
        for x in g[100:170]:
            w.task[x] = 0x7070
        w.bind()
        w.calls([(g[100], g[3])])  # one entry: 70 callers attributed in one level
        w.calls([(x, y) for x in g[200:1700] for y in (g[40], g[7])])
        w.states({g[3]: (BAD, 2), g[40]: (BAD, 2), g[7]: (DOWN, 0)})
        w.states({x: (BAD, DEP) for x in g[100:170] + g[200:1700]})
        rec, st, competing = check(w, masks=(0,))
        assert rec[sl[g[3]]]["nresolved"] == 70 and rec[sl[g[7]]]["nresolved"] == 1500 and rec[sl[g[40]]]["nresolved"] == 0
        assert st["resolved"] == st["resolved_at_tier"][0] == 1570 and competing == 1500
        assert (rec["src_slot"][[sl[x] for x in g[200:1700]]] == sl[g[7]]).all()
    finally:
        w.close_engine()


def test_blocking_and_cycles(torch_mod):
    w = World(2, 30)
    try:
        g, sl = w.svc, w.slot_of
        mids = {0: (GOOD, 0), 1: (IDLE, 0), 2: None, 3: (OK, 0), 4: (BAD, 2)}
        items = {}
        for k, mid in mids.items():
            s, m, f = g[3 * k], g[3 * k + 1], g[3 * k + 2]
            chain(w, [s, m, f])
            items[s], items[f] = (BAD, 1), (BAD, DEP)
            if mid:
                items[m] = mid
        items[g[20]] = (OK, 0)                       # an OK slot nobody reaches
        items[g[21]], items[g[22]] = (BAD, 3), (DOWN, DEP)
        w.calls([(g[22], g[21])])
        items[g[25]] = (BAD, DEP)                    # a self edge without a source
        w.calls([(g[25], g[25])])
        for base in (30, 40):                        # a ring of four, twice; 40 also calls the source 45
            w.calls([(g[base + i], g[base + (i + 1) % 4]) for i in range(4)])
            items.update({g[base + i]: (BAD, DEP) for i in range(4)})
        w.calls([(g[40], g[45])])
        items[g[45]] = (SEVERE, 4)
        w.states(items)
        rec, st, _ = check(w)
        role = lambda i: int(rec[sl[g[i]]]["role"])
        assert role(2) == role(5) == role(8) == capi.RS_UNRESOLVED and role(1) == role(4) == role(7) == capi.RS_NONE
        assert role(10) == capi.RS_CARRIER and role(11) == capi.RS_RESOLVED and rec[sl[g[11]]]["tier"] == 2 and rec[sl[g[9]]]["nresolved"] == 1
        assert role(13) == capi.RS_SOURCE and rec[sl[g[14]]]["src_slot"] == sl[g[13]] and rec[sl[g[12]]]["nresolved"] == 0
        assert role(20) == capi.RS_NONE and rec[sl[g[20]]]["state"] == OK and role(22) == capi.RS_RESOLVED and role(25) == capi.RS_UNRESOLVED
        assert [role(30 + i) for i in range(4)] == [capi.RS_UNRESOLVED] * 4
        assert [int(rec[sl[g[40 + i]]]["tier"]) for i in range(4)] == [1, 4, 3, 2]
    finally:
        w.close_engine()


def test_currency_delete_and_reuse(torch_mod):
    w = World(2, 10)
    try:
        g, sl = w.svc, w.slot_of
        chain(w, g[0:4])
        chain(w, g[5:9])
        w.states({g[0]: (BAD, 1), g[5]: (BAD, 1), **{x: (BAD, DEP) for x in g[1:4] + g[6:9]}})
        rec0, st0, _ = check(w)
        assert st0["resolved"] == 6
        w.window_close()
        rec1, st1, _ = check(w)
        assert rec1.tobytes() == rec0.tobytes() and st1 == st0
        w.states({g[2]: None})  # a LISTEN_FLAG_DELETE record: the slot is OPAQUE, the chain behind it is cut
        rec, st, _ = check(w)
        assert rec[sl[g[2]]]["role"] == capi.RS_NONE and rec[sl[g[2]]]["state"] == 0 and rec[sl[g[3]]]["role"] == capi.RS_UNRESOLVED
        w.states({x: (BAD, DEP) for x in g[6:9]})  # the second chain reports again, the first does not
        via = sl[g[6]]
        w.delete(g[6])  # a via slot leaves: the path is cut
        rec, st, _ = check(w)
        assert rec[via]["role"] == capi.RS_NONE and rec[sl[g[7]]]["role"] == capi.RS_UNRESOLVED and rec[sl[g[5]]]["nresolved"] == 0
        new = w.eng.register_listeners_slots(w.info[1][0], [g[6]], wire.listener_netns(1, np.array([77])), wire.listener_port(np.array([77])))
        assert int(new[0]) == via  # the slot is handed out again: it starts with no state and unbound
        w.slot_of[g[6]], w.host_of[g[6]] = via, 1
        rec, st, _ = check(w)
        assert rec[via]["role"] == capi.RS_NONE and rec[via]["state"] == 0
        w.task[g[6]] = 0xA000 + via
        w.bind()
        w.states({g[6]: (BAD, DEP)})
        rec, st, _ = check(w)
        assert rec[via]["role"] == capi.RS_RESOLVED and rec[sl[g[8]]]["tier"] == 3
        w.window_close()
        w.window_close()  # two closes without new state records: nothing is current
        rec, st, _ = check(w)
        assert not rec["role"].any() and st["edges"] == 6 and {k: v for k, v in st.items() if k != "edges"} == dict(
            with_state=0, sources=0, resolved=0, unresolved=0, carriers=0, resolved_at_tier=[0] * 8)
    finally:
        w.close_engine()


def test_decisions_replace_the_kept_states(torch_mod):
    w = World(2, 10)
    try:
        g, sl = w.svc, w.slot_of
        chain(w, g[0:5])
        chain(w, g[10:14])
        w.states({g[0]: (BAD, 1), g[1]: (BAD, DEP), g[2]: (OK, 0), g[3]: (BAD, DEP), g[4]: (GOOD, 0)})
        w.window_close()
        w.window_close()
        w.states({g[10]: (SEVERE, 2), g[11]: (BAD, DEP), g[12]: (BAD, DEP)})  # (the first chain's records are stale now)
        nsvc = w.eng.num_services()
        rec0, st0, _ = check(w)
        assert st0["with_state"] == 3 and st0["resolved"] == 2
        dec = np.zeros(nsvc, dtype=w.eng.DECISION_DT)
        dec["state"], dec["decided_line"] = 9, 2866  # (a state above 5: no state)
        same = w.kept_states()
        for s, (a, b) in same.items():
            dec[s]["state"], dec[s]["issue"] = a, b
        rec1, st1, _ = check(w, dec, same)
        assert rec1.tobytes() == rec0.tobytes() and st1 == st0
        other = {sl[g[0]]: (DOWN, 3), sl[g[1]]: (BAD, DEP), sl[g[2]]: (OK, 5), sl[g[3]]: (SEVERE, DEP), sl[g[10]]: (GOOD, 0), sl[g[11]]: (BAD, DEP)}
        dec["state"], dec["issue"] = 9, 0
        for s, (a, b) in other.items():
            dec[s]["state"], dec[s]["issue"] = a, b
        rec2, st2, _ = check(w, dec, other)
        assert rec2[sl[g[3]]]["tier"] == 3 and rec2[sl[g[2]]]["role"] == capi.RS_CARRIER and rec2[sl[g[11]]]["role"] == capi.RS_UNRESOLVED and st2["sources"] == 1
    finally:
        w.close_engine()


@pytest.fixture(scope="module")
def random_world(torch_mod):
    """600 services (6 hosts x 100: not a multiple of 256), slots 0 .. 69 one task group, 2 000 random rows, random classes"""
    w = World(6, 100)
    rng = np.random.default_rng(20250607)
    g = w.svc
    by_slot = sorted(g, key=lambda x: w.slot_of[x])
    for x in by_slot[:70]:
        w.task[x] = 0x7070
    w.bind()
    pairs = [(g[int(rng.integers(600))], g[int(rng.integers(600))]) for _ in range(2000)]
    w.calls(pairs[:1000])
    w.calls(pairs[1000:])
    items = {}
    for x in g:
        r = rng.random()
        if r < 0.05:
            items[x] = (int(rng.integers(3, 6)), int(rng.integers(0, 7)))
        elif r < 0.40:
            items[x] = (int(rng.integers(3, 6)), DEP)
        elif r < 0.70:
            items[x] = (OK, int(rng.integers(0, 16)))
        elif r < 0.95:
            items[x] = (int(rng.integers(0, 2)), 0)
    w.states(items)
    yield w
    w.close_engine()


def test_random_world(random_world):
    w = random_world
    nsvc = w.eng.num_services()
    assert nsvc == 600 and nsvc % 256
    edges, nedges = w.edges()
    rec, _, stats, competing = model(w.eng, nsvc, w.kept_states(), edges, nedges, 0)
    # the witnesses, on the model
    for role in (1, 2, 3, 4):
        assert (rec["role"] == role).sum() >= 10, role
    assert sum(n >= 5 for n in stats["resolved_at_tier"]) >= 4, stats
    assert competing >= 20, competing
    for mt in (0, 1, 4):
        check(w, max_tiers=mt)


def test_top_sources(random_world):
    w = random_world
    eng = w.eng
    nsvc = eng.num_services()
    rec, imp, _ = eng.resolve_issues_np()
    out, d_imp, _ = eng.resolve_issues_dev()
    top, nelig = eng.topk(d_imp, 5)
    srcs = np.flatnonzero(rec["role"] == capi.RS_SOURCE)
    order = sorted(srcs, key=lambda s: (-int(rec[s]["nresolved"]), s))[:5]
    assert nelig == len(srcs) and [int(r) for r in top["row"]] == [int(s) for s in order]
    assert [float(v) for v in top["value"]] == [float(rec[s]["nresolved"]) for s in order] and rec[order[0]]["nresolved"] > 0


def test_errors_and_purity(torch_mod, random_world):
    off = World(1, 4, cap=0)
    try:
        L, h = off.eng.L, off.eng.h
        d = torch_mod.zeros(4096, dtype=torch_mod.uint8, device=off.eng.device)
        dp = C.c_void_p(d.data_ptr())
        n32, m32, st = C.c_uint32(), C.c_uint32(), capi.SvcResolStats()
        row = (capi.SvcResolRow * 8)()
        assert L.gys_svc_resolve_issues_dev(h, None, 0, dp, None, C.byref(st)) == capi.ERR_STATE
        assert L.gys_svc_resolve_issues(h, None, 0, 0, row, 8, C.byref(n32), C.byref(m32), C.byref(st)) == capi.ERR_STATE
    finally:
        off.close_engine()
    w = random_world
    eng = w.eng
    L, h = eng.L, eng.h
    d = torch_mod.zeros(600 * 16, dtype=torch_mod.uint8, device=eng.device)
    dp = C.c_void_p(d.data_ptr())
    assert L.gys_svc_resolve_issues_dev(h, None, 0, None, None, None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues_dev(h, None, 9, dp, None, None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues(h, None, 0, 0, row, 8, None, C.byref(m32), None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues(h, None, 0, 0, row, 8, C.byref(n32), None, None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues(h, None, 0, 0, None, 8, C.byref(n32), C.byref(m32), None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues(h, None, 9, 0, row, 8, C.byref(n32), C.byref(m32), None) == capi.ERR_INVAL
    assert L.gys_svc_resolve_issues(h, None, 0, 0x20, row, 8, C.byref(n32), C.byref(m32), None) == capi.ERR_INVAL
    # purity: the service records before and after; a room too small writes nothing; two calls give equal bytes
    blob_bytes = eng.service_blob_bytes(600)
    before = eng.pack_services().tobytes()
    a, ia, sa = eng.resolve_issues_np()
    b, ib, sb = eng.resolve_issues_np()
    assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes() and sa == sb
    marker = bytes(row)
    st = capi.SvcResolStats()
    assert L.gys_svc_resolve_issues(h, None, 0, 0, row, 8, C.byref(n32), C.byref(m32), C.byref(st)) == capi.ERR_NOMEM
    assert n32.value == 0 and m32.value == int((a["role"] != 0).sum()) > 8 and bytes(row) == marker and eng._resol_stats(st) == sa
    r1, r2 = eng.resolve_issues(), eng.resolve_issues()
    assert r1[0] == capi.OK and r1[1].tobytes() == r2[1].tobytes() and r1[2:] == r2[2:]
    assert eng.pack_services().tobytes() == before and eng.service_blob_bytes(600) == blob_bytes
