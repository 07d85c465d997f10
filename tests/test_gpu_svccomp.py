"""Service components on the GPU (gyeeta_amd/csrc/gys_svccomp.hpp): gys_svc_components_dev, gys_svc_components and
gys_label_service_components against the Python edge dictionary of the definition ("Service dependency graph" in include/gysketch.h) and a
Python union-find over it ("Service components").  Every comparison is exact.  World A: 3 hosts x 9 services; world B: 4 hosts x 80
services.  The small model class is a copy of the one in tests/test_gpu_svcdeps.py, with the components added."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

RING = 3  # GYS_ACT_RING
T0 = 1_700_000_000_000_000


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


class World:
    """an engine, and the model beside it: the row table (key -> latest report), the registry (glob_id -> slot) and the bindings"""

    def __init__(self, nh, sp, cap, spare=8, **kw):
        from gyeeta_amd.engine import SketchEngine
        self.eng = SketchEngine(max_hosts=nh, max_services=nh * sp + spare, enable_tdigest=False, actconn_pair_cap=cap, **kw)
        self.nh, self.sp = nh, sp
        self.info, self.gids = helpers.register_world(self.eng, None, range(nh), sp)
        self.svc = [int(g) for h in range(nh) for g in self.gids[h]]
        self.slot_of = {g: self.eng.lookup(g) for g in self.svc}
        self.task = {}
        self.ent = {}
        self.epoch = 1
        self.rng = np.random.default_rng(nh * 1000 + sp)
        self.nclose = 0

    def close_engine(self):
        self.eng.close()

    def bind(self, ids, tasks):
        assert self.eng.set_listener_tasks(ids, tasks) == capi.OK
        for g, t in zip(ids, tasks):
            self.task[int(g)] = int(t)

    def report(self, keys, host=0):
        """one call with one row per (listener id, client id, kind) of `keys`, random figures"""
        n = len(keys)
        rec = np.zeros(n, dtype=wire.ACTIVE_CONN_STATS)
        rec["listener_glob_id"] = np.array([k[0] for k in keys], dtype=np.uint64)
        rec["cli_aggr_task_id"] = np.array([k[1] for k in keys], dtype=np.uint64)
        rec["bytes_sent"] = self.rng.integers(0, 1 << 40, n)
        rec["bytes_received"] = self.rng.integers(0, 1 << 40, n)
        rec["active_conns"] = self.rng.integers(0, 500, n)
        rec["flags"] = np.array([wire.ACTIVE_FLAG_REMOTE_LISTEN if k[2] else 0 for k in keys], dtype=np.uint8)
        self.eng.handle_partha_active_conns(self.info[host][0], rec.tobytes(), n)
        for r in rec:
            k = (int(r["listener_glob_id"]), int(r["cli_aggr_task_id"]), (int(r["flags"]) >> 1) & 1)
            e = self.ent.get(k)
            if e is None or e["window"] != self.epoch:
                e = self.ent[k] = dict(window=self.epoch, active_conns=0, bytes_sent=0, bytes_received=0)
            e["active_conns"] += int(r["active_conns"])
            e["bytes_sent"] += int(r["bytes_sent"])
            e["bytes_received"] += int(r["bytes_received"])

    def window_close(self):
        self.eng.window_close(T0 + self.nclose * 5_000_000)
        self.nclose += 1
        self.epoch += 1

    def delete(self, gid):
        assert self.eng.delete_listeners([gid]) == 1
        del self.slot_of[gid]
        self.task.pop(gid, None)

    # ---- the definition
    def entries(self):
        """the live entries that give an edge: (listener slot v, the caller slots, the entry)"""
        bound = defaultdict(list)
        for g, t in self.task.items():
            if t and g in self.slot_of:
                bound[t].append(self.slot_of[g])
        for (lid, cid, _kind), e in self.ent.items():
            if self.epoch - e["window"] > RING or lid not in self.slot_of or cid == 0 or cid not in bound:
                continue
            yield self.slot_of[lid], bound[cid], e

    def components(self):
        """slot -> the lowest slot of its component (a union-find over the edges, either direction); root -> the component's figures"""
        par = {s: s for s in self.slot_of.values()}

        def find(x):
            while par[x] != x:
                par[x] = par[par[x]]
                x = par[x]
            return x

        ents = list(self.entries())
        for v, callers, _e in ents:
            for u in callers:
                a, b = find(u), find(v)
                if a != b:
                    par[max(a, b)] = min(a, b)  # (the lower root stays: the root of a set is its lowest slot)
        comp = {s: find(s) for s in par}
        assert all(comp[s] <= s and comp[comp[s]] == comp[s] for s in comp)
        fig = {r: dict(nservices=0, nrows=0, nedges=0, active_conns=0, bytes_sent=0, bytes_received=0) for r in set(comp.values())}
        for s, r in comp.items():
            fig[r]["nservices"] += 1
        for v, callers, e in ents:
            f = fig[comp[v]]
            f["nrows"] += 1
            f["nedges"] += len(callers)
            for k in ("active_conns", "bytes_sent", "bytes_received"):
                f[k] = (f[k] + e[k]) & 0xFFFFFFFFFFFFFFFF
        return comp, fig


def _check_comp(w):
    """comp[] and the two counts of gys_svc_components_dev, with and without the counts"""
    eng = w.eng
    comp, fig = w.components()
    nsvc = eng.num_services()
    exp = np.full(nsvc, capi.NOSLOT, dtype=np.uint32)
    for s, r in comp.items():
        exp[s] = r
    t, ncomp, nlinked = eng.svc_components_dev()
    eng.sync()
    got = t.cpu().numpy().view(np.uint32)[:nsvc]
    assert np.array_equal(got, exp), (np.flatnonzero(got != exp)[:8], got[got != exp][:8], exp[got != exp][:8])
    assert ncomp == len(fig) and nlinked == sum(f["nservices"] >= 2 for f in fig.values()), (ncomp, nlinked, len(fig))
    t2, a, b = eng.svc_components_dev(counts=False)
    eng.sync()
    assert a is None and b is None and np.array_equal(t2.cpu().numpy().view(np.uint32)[:nsvc], exp)
    return comp, fig


def _check_list(w, fig, min_services):
    """rows, order and every figure of gys_svc_components; one short of room"""
    eng = w.eng
    gid_of = {s: g for g, s in w.slot_of.items()}
    want = sorted((r for r, f in fig.items() if f["nservices"] >= min_services), key=lambda r: (-fig[r]["nservices"], r))
    rc, rows, nmatch, ncomp = eng.svc_components(min_services)
    assert rc == capi.OK and nmatch == len(want) and ncomp == len(fig) and len(rows) == len(want), (min_services, rc, nmatch, len(want), ncomp, len(fig))
    assert [int(x) for x in rows["root_slot"]] == want
    for r, root in zip(rows, want):
        assert int(r["root_glob_id"]) == gid_of[root] and int(r["reserved"]) == 0
        for k, v in fig[root].items():
            assert int(r[k]) == v, (min_services, root, k, int(r[k]), v)
    if want:
        out = (capi.SvcComponent * len(want))()
        C.memset(out, 0x5A, C.sizeof(out))
        nout, nm, nc = C.c_uint32(9), C.c_uint32(), C.c_uint32()
        assert eng.L.gys_svc_components(eng.h, min_services, out, len(want) - 1, C.byref(nout), C.byref(nm), C.byref(nc)) == capi.ERR_NOMEM
        assert nout.value == 0 and nm.value == len(want) and nc.value == len(fig) and bytes(out) == b"\x5a" * C.sizeof(out)
    return rows


# ---------------------------------------------------------------------------------------------------------------- world A
def _world_a(cap=512, **kw):
    w = World(3, 9, cap, **kw)
    g = w.gids
    w.T = {s: 0xA000 + w.slot_of[s] for s in w.svc}
    for s in (int(g[1][0]), int(g[1][1])):
        w.T[s] = 0xBEEF  # one task group with two listeners
    del w.T[int(g[2][8])]  # never bound
    w.bind(list(w.T), list(w.T.values()))
    return w


def _shapes(w):
    g = w.gids
    A, B, Cc, D = (int(g[0][i]) for i in range(4))
    T = w.T
    keys = [(B, T[A], 0), (Cc, T[B], 0), (D, T[Cc], 0)]                          # the chain A -> B -> C -> D
    keys += [(int(g[1][k]), T[A], 0) for k in range(2, 4)]                       # a fan-out of A
    keys += [(int(g[2][0]), 0xBEEF, 0)]                                           # both listeners of the group are callers: one entry, two edges
    keys += [(Cc, 0xDEAD, 0), (0x1234567, T[A], 0), (B, 0, 0)]                    # rows that give no edge
    keys += [(int(g[2][1]), T[int(g[2][3])], 1), (int(g[2][1]), T[int(g[2][3])], 0)]  # a pair of their own, in both kinds: two entries
    keys += [(int(g[2][2]), T[int(g[2][2])], 0)]                                  # only a self-call: alone
    keys += [(int(g[1][6]), T[int(g[1][7])], 1)]                                  # a pair joined by a kind-1 row alone
    return keys, (A, B, Cc, D)


def test_components_follow_rows_closes_a_delete_and_a_reused_slot(torch_mod):
    w = _world_a()
    try:
        g, sl = w.gids, w.slot_of
        keys, (A, B, Cc, D) = _shapes(w)
        comp, fig = _check_comp(w)  # nothing reported: everyone alone
        assert len(fig) == 27 and all(f["nservices"] == 1 for f in fig.values())
        w.report(keys[:7], host=0)
        w.report(keys[7:], host=2)
        comp, fig = _check_comp(w)
        assert comp[sl[D]] == comp[sl[A]] == comp[sl[int(g[1][3])]] and comp[sl[int(g[2][2])]] == sl[int(g[2][2])]
        assert comp[sl[int(g[1][0])]] == comp[sl[int(g[1][1])]] == comp[sl[int(g[2][0])]] and fig[comp[sl[int(g[2][0])]]]["nservices"] == 3
        assert fig[comp[sl[int(g[2][1])]]]["nrows"] == 2 and fig[comp[sl[int(g[2][2])]]]["nedges"] == 1 and comp[sl[int(g[1][6])]] == comp[sl[int(g[1][7])]]
        for ms in (0, 1, 2, 5, 28):
            _check_list(w, fig, ms)
        # random rows of both kinds on top, then a window close: the graph stays while the rows live
        rk = [(w.svc[int(w.rng.integers(27))], 0xA000 + int(w.rng.integers(27)), int(w.rng.random() < 0.4)) for _ in range(12)]
        w.report(rk, host=1)
        _, fig = _check_comp(w)
        _check_list(w, fig, 0)
        w.window_close()
        _, fig2 = _check_comp(w)
        assert fig2 == fig
        for _ in range(3):
            w.window_close()
        comp, fig = _check_comp(w)  # every row expired: every registered slot is its own root
        assert all(comp[s] == s for s in comp) and len(fig) == 27
        assert w.eng.svc_components_dev()[2] == 0
        rc, rows, nmatch, ncomp = w.eng.svc_components(2)
        assert rc == capi.OK and nmatch == 0 and ncomp == 27 and len(rows) == 0
        # a delete in the middle of the chain: the component splits, the free slot reads GYS_NOSLOT
        w.report(keys)
        comp, _ = _check_comp(w)
        assert comp[sl[D]] == comp[sl[A]]
        cslot = sl[Cc]
        w.delete(Cc)
        comp, fig = _check_comp(w)
        assert cslot not in comp and comp[sl[D]] == sl[D] and comp[sl[B]] == comp[sl[A]]
        t, _, _ = w.eng.svc_components_dev()
        assert int(t[cslot].item()) == -1
        _check_list(w, fig, 0)
        # C comes back into the freed slot: it is called again (the rows name its id), it is unbound, so D stays alone
        new = w.eng.register_listeners_slots(w.info[1][0], [Cc], wire.listener_netns(1, np.array([40])), wire.listener_port(np.array([40])))
        assert int(new[0]) == cslot
        w.slot_of[Cc] = cslot
        comp, fig = _check_comp(w)
        assert comp[cslot] == comp[sl[A]] and comp[sl[D]] == sl[D]
        w.delete(Cc)  # ... and registered without a row naming it, it starts alone
        Cn = 0x777001
        new = w.eng.register_listeners_slots(w.info[1][0], [Cn], wire.listener_netns(1, np.array([41])), wire.listener_port(np.array([41])))
        assert int(new[0]) == cslot
        w.slot_of[Cn] = cslot
        comp, fig = _check_comp(w)
        assert comp[cslot] == cslot and fig[cslot]["nservices"] == 1 and fig[cslot]["nrows"] == 0
        w.bind([Cn], [w.T[Cc]])  # bound to C's old group it calls D again (the row (D, T[C]) is still live)
        comp, fig = _check_comp(w)
        assert comp[sl[D]] == comp[cslot] == min(cslot, sl[D])
        _check_list(w, fig, 2)
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- world B
def test_4096_edges_inside_one_component_the_bfs_and_the_list(torch_mod):
    w = World(4, 80, 4096)
    try:
        # task groups of 20 .. 40 listeners over the first 300 services, the last 20 each with a group of their own
        T, i, k = {}, 0, 0
        while i < 300:
            n = min(20 + (7 * k) % 21, 300 - i)
            for s in w.svc[i:i + n]:
                T[s] = 0xB000 + k
            i, k = i + n, k + 1
        for s in w.svc[300:]:
            T[s] = 0xC000 + w.slot_of[s]
        w.bind(list(T), list(T.values()))
        rng = np.random.default_rng(5)
        groups = sorted(set(T[s] for s in w.svc[:300]))
        keys = {(w.svc[int(rng.integers(280))], groups[int(rng.integers(len(groups)))], int(rng.random() < 0.25)) for _ in range(300)}
        keys |= {(w.svc[301], T[w.svc[302]], 0), (w.svc[303], T[w.svc[302]], 1), (w.svc[310], T[w.svc[310]], 0)}  # small components beside it
        keys |= {(0x5000 + j, groups[0], 0) for j in range(10)} | {(w.svc[5], 0xDEAD00 + j, 0) for j in range(10)}
        keys = sorted(keys)
        w.report(keys[:160], host=0)
        w.report(keys[160:], host=3)
        comp, fig = _check_comp(w)
        big = max(fig, key=lambda r: fig[r]["nedges"])
        assert fig[big]["nedges"] >= 4096 and fig[big]["nservices"] >= 280, fig[big]
        st = w.eng.svcgraph_stats()
        rows = {ms: _check_list(w, fig, ms) for ms in (0, 2, 5)}
        assert int(rows[0]["nedges"].sum()) == st["edges"] and int(rows[0]["nservices"].sum()) == len(w.slot_of) == 320
        assert int(rows[0]["nrows"].sum()) == st["live_rows"] - len([1 for lid, cid, _ in keys if lid not in w.slot_of or cid not in set(T.values())])
        assert len(rows[2]) == 2 and len(rows[5]) == 1 and int(rows[2]["nservices"][1]) == 3
        # the members of X's component are what the search from X reaches, either way at every step
        gid_of = {s: g for g, s in w.slot_of.items()}
        for x in [w.svc[int(j)] for j in rng.integers(0, 320, 5)] + [w.svc[302]]:
            rc, ids, hops, n = w.eng.svc_deps([x], capi.DEP_BOTH, 0)
            assert rc == capi.OK
            members = sorted(s for s, r in comp.items() if r == comp[w.slot_of[x]])
            assert sorted(w.slot_of[int(g)] for g in ids) == members and n == len(members) == fig[comp[w.slot_of[x]]]["nservices"], x
            assert [gid_of[s] for s in members][0] == gid_of[comp[w.slot_of[x]]]
    finally:
        w.close_engine()


def test_a_path_of_300_services_in_shuffled_slot_order(torch_mod):
    w = World(4, 80, 4096)
    try:
        T = {s: 0xA000 + w.slot_of[s] for s in w.svc}
        w.bind(list(T), list(T.values()))
        order = [w.svc[int(j)] for j in np.random.default_rng(17).permutation(320)[:300]]
        w.report([(order[i + 1], T[order[i]], i & 1) for i in range(299)])
        comp, fig = _check_comp(w)
        root = min(w.slot_of[s] for s in order)
        assert fig[root]["nservices"] == 300 and fig[root]["nedges"] == fig[root]["nrows"] == 299 and len(fig) == 21
        rows = _check_list(w, fig, 2)
        assert len(rows) == 1 and int(rows["root_slot"][0]) == root
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- labels
def _label_rollups(eng):
    out = []
    for which in (0, 1):
        rows, nrows, recs = eng.svc_hist_rollup_filtered(capi.GROUP_LABEL, which, any_state=True)
        out.append((rows, nrows, recs.tobytes()))
    return out


def test_labels_make_the_components_roll_up_groups(torch_mod):
    w = _world_a(enable_levels=True)
    try:
        eng = w.eng
        for h in range(3):  # a QPS / active-connection histogram per service to roll up
            r = wire.synth_listener_states(w.rng, h, np.arange(9))
            eng.partha_listener_state(w.info[h][0], r.tobytes(), len(r))
        w.window_close()
        keys, _ = _shapes(w)
        w.report(keys)
        comp, fig = _check_comp(w)
        linked = sorted(r for r, f in fig.items() if f["nservices"] >= 2)
        assert len(linked) == 4
        eng.set_service_groups(w.svc, np.full(len(w.svc), 7, dtype=np.uint32))  # whatever labels there were are gone afterwards
        assert eng.label_service_components(2) == len(linked)
        got = _label_rollups(eng)
        for rows, nrows, recs in got:
            assert nrows == len(linked) and rows == [(r, fig[r]["nservices"]) for r in linked]
        svc = [eng.export_svc_hist(0), eng.export_svc_hist(1)]
        assert svc[0][:, 15, 0].sum() > 0
        for which in (0, 1):  # the records are those of the components' members
            recs = np.frombuffer(got[which][2], dtype=np.int64).reshape(-1, 16, 2)
            for i, r in enumerate(linked):
                mem = [s for s, c in comp.items() if c == r]
                assert (recs[i, :15] == svc[which][mem].sum(axis=0)[:15]).all(), (which, r)
        _check_comp(w)  # (labelling changed nothing of the graph)
        # the same assignment by hand: byte-identical rows and records
        eng.set_service_groups(w.svc, np.full(len(w.svc), 3, dtype=np.uint32))
        lab = np.array([comp[w.slot_of[g]] if fig[comp[w.slot_of[g]]]["nservices"] >= 2 else capi.NO_GROUP for g in w.svc], dtype=np.uint32)
        eng.set_service_groups(w.svc, lab)
        assert _label_rollups(eng) == got
        # min_services 0: every component is a group, the lone services too; a value above the largest: no group
        assert eng.label_service_components(0) == len(fig)
        rows, nrows, _ = eng.svc_hist_rollup_filtered(capi.GROUP_LABEL, 0, any_state=True)
        assert rows == [(r, fig[r]["nservices"]) for r in sorted(fig)]
        assert eng.label_service_components(28) == 0
        rows, nrows, _ = eng.svc_hist_rollup_filtered(capi.GROUP_LABEL, 0, any_state=True)
        assert rows == [] and nrows == 0
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_an_empty_engine_and_nothing_is_modified(torch_mod):
    from gyeeta_amd.engine import SketchEngine
    off = World(3, 9, 0)
    on = _world_a(64)
    empty = SketchEngine(max_hosts=2, max_services=16, enable_tdigest=False, actconn_pair_cap=64)
    try:
        n1, n2, n3 = C.c_uint32(5), C.c_uint32(5), C.c_uint32(5)
        out = (capi.SvcComponent * 4)()
        d = torch_mod.zeros(1024, dtype=torch_mod.int32, device=off.eng.device)
        dp = C.c_void_p(d.data_ptr())
        L, h = off.eng.L, off.eng.h
        assert L.gys_svc_components_dev(h, dp, C.byref(n1), C.byref(n2)) == capi.ERR_STATE
        assert L.gys_svc_components(h, 0, out, 4, C.byref(n1), C.byref(n2), C.byref(n3)) == capi.ERR_STATE
        assert L.gys_label_service_components(h, 2, C.byref(n1)) == capi.ERR_STATE
        L, h = on.eng.L, on.eng.h
        assert L.gys_svc_components_dev(h, None, C.byref(n1), C.byref(n2)) == capi.ERR_INVAL
        assert L.gys_svc_components(h, 0, out, 4, None, C.byref(n2), C.byref(n3)) == capi.ERR_INVAL
        assert L.gys_svc_components(h, 0, out, 4, C.byref(n1), None, C.byref(n3)) == capi.ERR_INVAL
        assert L.gys_svc_components(h, 0, None, 4, C.byref(n1), C.byref(n2), C.byref(n3)) == capi.ERR_INVAL
        assert L.gys_svc_components(h, 0, None, 0, C.byref(n1), C.byref(n2), None) == capi.ERR_NOMEM and n2.value == 27 and n1.value == 0  # (a count)
        assert L.gys_svc_components_dev(h, dp, None, None) == capi.OK
        assert L.gys_svc_components_dev(h, dp, None, C.byref(n2)) == capi.OK and n2.value == 0
        assert L.gys_label_service_components(h, 2, None) == capi.OK
        # an engine with no service answers with zeros
        L, h = empty.L, empty.h
        n1, n2, n3 = C.c_uint32(5), C.c_uint32(5), C.c_uint32(5)
        assert L.gys_svc_components_dev(h, dp, C.byref(n1), C.byref(n2)) == capi.OK and n1.value == 0 and n2.value == 0
        n1, n2, n3 = C.c_uint32(5), C.c_uint32(5), C.c_uint32(5)
        assert L.gys_svc_components(h, 0, out, 4, C.byref(n1), C.byref(n2), C.byref(n3)) == capi.OK and (n1.value, n2.value, n3.value) == (0, 0, 0)
        n1 = C.c_uint32(5)
        assert L.gys_label_service_components(h, 0, C.byref(n1)) == capi.OK and n1.value == 0
        # the two query calls modify nothing: the table's counters and an edge listing are what they were
        keys, _ = _shapes(on)
        on.report(keys)
        ts, edges = on.eng.actconn_table_stats(), on.eng.svc_edges()[1].tobytes()
        _, fig = _check_comp(on)
        _check_list(on, fig, 0)
        assert on.eng.actconn_table_stats() == ts and on.eng.svc_edges()[1].tobytes() == edges and len(edges) > 0
    finally:
        off.close_engine()
        on.close_engine()
        empty.close()
