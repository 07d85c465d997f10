"""The service dependency graph on the GPU (gyeeta_amd/csrc/gys_svcdeps.hpp): gys_set_listener_tasks, gys_svc_edges / _dev,
gys_svcgraph_stats, gys_svc_deps / _dev against a Python dict of edges and a deque BFS written here from the definition ("Service dependency
graph" in include/gysketch.h).  Every comparison is exact.  World A: 3 hosts x 9 services; world B: 4 hosts x 80 services."""
import ctypes as C
from collections import defaultdict, deque

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

    def __init__(self, nh, sp, cap, spare=8):
        from gyeeta_amd.engine import SketchEngine
        self.eng = SketchEngine(max_hosts=nh, max_services=nh * sp + spare, enable_tdigest=False, actconn_pair_cap=cap)
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

    def bind(self, ids, tasks, expect=capi.OK):
        assert self.eng.set_listener_tasks(ids, tasks) == expect
        if expect == capi.OK:
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
        fl = np.array([wire.ACTIVE_FLAG_REMOTE_LISTEN if k[2] else 0 for k in keys], dtype=np.uint8)
        fl |= np.where(self.rng.random(n) < 0.3, wire.ACTIVE_FLAG_CLI_LISTENER_PROC, 0).astype(np.uint8)
        rec["flags"] = fl
        self.eng.handle_partha_active_conns(self.info[host][0], rec.tobytes(), n)
        for r in rec:
            k = (int(r["listener_glob_id"]), int(r["cli_aggr_task_id"]), (int(r["flags"]) >> 1) & 1)
            e = self.ent.get(k)
            if e is None or e["window"] != self.epoch:
                e = self.ent[k] = dict(window=self.epoch, active_conns=0, bytes_sent=0, bytes_received=0, nrows=0, flags=0)
            e["active_conns"] += int(r["active_conns"])
            e["bytes_sent"] += int(r["bytes_sent"])
            e["bytes_received"] += int(r["bytes_received"])
            e["nrows"] += 1
            e["flags"] |= int(r["flags"])

    def window_close(self):
        self.eng.window_close(T0 + self.nclose * 5_000_000)
        self.nclose += 1
        self.epoch += 1

    def delete(self, gid):
        assert self.eng.delete_listeners([gid]) == 1
        del self.slot_of[gid]
        self.task.pop(gid, None)

    # ---- the definition
    def edges(self):
        """(src slot, dst slot, kind) -> (listener id, client id, the entry), and the counters"""
        bound = defaultdict(list)
        for g, t in self.task.items():
            if t and g in self.slot_of:
                bound[t].append(self.slot_of[g])
        out = {}
        st = dict(live_rows=0, rows_no_listener=0, rows_no_client=0, edges=0, bound_services=sum(len(v) for v in bound.values()), bound_tasks=len(bound))
        for (lid, cid, kind), e in self.ent.items():
            if self.epoch - e["window"] > RING:
                continue
            st["live_rows"] += 1
            nol, noc = lid not in self.slot_of, cid == 0 or cid not in bound
            st["rows_no_listener"] += nol
            st["rows_no_client"] += noc
            if nol or noc:
                continue
            for u in bound[cid]:
                k = (u, self.slot_of[lid], kind)
                assert k not in out
                out[k] = (lid, cid, e)
        st["edges"] = len(out)
        return out, st

    def hops(self, edges, roots, direction, max_hops):
        """slot -> least number of edges from a root (deque BFS)"""
        adj = defaultdict(set)
        for (u, v, _k) in edges:
            if direction & 1:
                adj[u].add(v)
            if direction & 2:
                adj[v].add(u)
        dist = {}
        q = deque()
        for r in roots:
            if r in self.slot_of and self.slot_of[r] not in dist:
                dist[self.slot_of[r]] = 0
                q.append(self.slot_of[r])
        while q:
            u = q.popleft()
            if max_hops and dist[u] >= max_hops:
                continue
            for v in sorted(adj[u]):
                if v not in dist:
                    dist[v] = dist[u] + 1
                    q.append(v)
        return dist


def _check_edge_rows(w, rows, want):
    keys = [(int(r["src_slot"]), int(r["dst_slot"]), int(r["kind"])) for r in rows]
    assert keys == sorted(want), (len(keys), len(want))
    gid_of = {s: g for g, s in w.slot_of.items()}
    for r, k in zip(rows, keys):
        lid, cid, e = want[k]
        assert int(r["src_glob_id"]) == gid_of[k[0]] and int(r["dst_glob_id"]) == lid == gid_of[k[1]] and int(r["cli_aggr_task_id"]) == cid, k
        for f in ("window", "active_conns", "bytes_sent", "bytes_received", "nrows", "flags"):
            assert int(r[f]) == e[f], (k, f, int(r[f]), e[f])
        assert not r["pad"].any()


def _check_edges(w, sels=()):
    eng = w.eng
    want, st = w.edges()
    rc, rows, nmatch = eng.svc_edges()
    assert rc == capi.OK and nmatch == len(want)
    _check_edge_rows(w, rows, want)
    assert eng.svcgraph_stats() == st
    gid_of = {s: g for g, s in w.slot_of.items()}
    for kw in sels:
        sub = {k: v for k, v in want.items() if ("src" not in kw or gid_of[k[0]] == kw["src"]) and ("dst" not in kw or gid_of[k[1]] == kw["dst"])}
        sel = eng.svc_edge_sel(**kw)
        rc, rows, nmatch = eng.svc_edges(sel)
        assert rc == capi.OK and nmatch == len(sub), (kw, nmatch, len(sub))
        _check_edge_rows(w, rows, sub)
        if sub:
            rc, rows, nmatch = eng.svc_edges(sel, cap=len(sub) - 1)
            assert rc == capi.ERR_NOMEM and nmatch == len(sub) and len(rows) == 0, kw
        for cap in (len(sub) + 3, len(sub) // 2):  # the device form: any order, min(matches, cap) rows
            t, nm = eng.svc_edges_dev(sel, cap)
            eng.sync()
            assert nm == len(sub)
            got = np.frombuffer(t.cpu().numpy().tobytes(), dtype=eng.SVC_EDGE_DT)
            nw = min(cap, len(sub))
            gk = {(int(r["src_slot"]), int(r["dst_slot"]), int(r["kind"])) for r in got[:nw]}
            assert len(gk) == nw and gk <= set(sub), kw
            assert not t[nw:].any().item(), "rows beyond min(matches, cap) were written"
            if cap >= len(sub):
                _check_edge_rows(w, np.sort(got[:nw], order=["src_slot", "dst_slot", "kind"]), sub)
    return want, st


def _check_deps(w, want_edges, roots, direction, max_hops):
    eng = w.eng
    dist = w.hops(want_edges, roots, direction, max_hops)
    nsvc = eng.num_services()
    exp = np.full(nsvc, capi.NOSLOT, dtype=np.uint32)
    for s, d in dist.items():
        exp[s] = d
    t, n = eng.svc_deps_dev(roots, direction, max_hops)
    eng.sync()
    got = t.cpu().numpy().view(np.uint32)[:nsvc]
    assert n == len(dist) and np.array_equal(got, exp), (roots, direction, max_hops, n, len(dist), np.flatnonzero(got != exp)[:8])
    gid_of = {s: g for g, s in w.slot_of.items()}
    order = sorted(dist, key=lambda s: (dist[s], s))
    rc, ids, hops, n = eng.svc_deps(roots, direction, max_hops)
    assert rc == capi.OK and n == len(dist)
    assert [int(x) for x in ids] == [gid_of[s] for s in order] and [int(x) for x in hops] == [dist[s] for s in order]
    if dist:
        rc, ids, hops, n = eng.svc_deps(roots, direction, max_hops, cap=len(dist) - 1)
        assert rc == capi.ERR_NOMEM and n == len(dist) and len(ids) == 0 and len(hops) == 0
    return dist


# ---------------------------------------------------------------------------------------------------------------- world A
def _world_a(cap=512):
    w = World(3, 9, cap)
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
    keys = [(B, T[A], 0), (Cc, T[B], 0), (D, T[Cc], 0), (B, T[D], 0)]            # the chain A -> B -> C -> D and the back edge D -> B
    keys += [(int(g[1][k]), T[A], 0) for k in range(2, 6)]                       # a fan-out of A
    keys += [(int(g[2][0]), 0xBEEF, 0)]                                           # both listeners of the group are callers
    keys += [(Cc, 0xDEAD, 0)]                                                     # a client group bound to nothing
    keys += [(0x1234567, T[A], 0)]                                                # a listener that is not registered
    keys += [(int(g[2][1]), T[D], 1), (int(g[2][1]), T[D], 0)]                    # kind 1 naming a listener of another host; the same pair as kind 0
    keys += [(0x7654321, T[D], 1)]                                                # kind 1 naming an unregistered listener
    keys += [(int(g[2][2]), T[int(g[2][2])], 0)]                                  # a self-call
    keys += [(B, 0, 0)]                                                           # client id 0
    return keys, (A, B, Cc, D)


def test_one_graph_of_every_shape(torch_mod):
    w = _world_a()
    try:
        g = w.gids
        keys, (A, B, Cc, D) = _shapes(w)
        w.report(keys[:9], host=0)
        w.report(keys[9:], host=2)
        sels = [dict(src=A), dict(dst=B), dict(src=D, dst=int(g[2][1])), dict(src=int(g[1][1])), dict(src=int(g[2][8])), dict(dst=0x1234567), dict(src=0x99)]
        want, st = _check_edges(w, sels)
        sl = w.slot_of
        assert st["edges"] == 13 and st["rows_no_listener"] == 2 and st["rows_no_client"] == 2 and st["live_rows"] == 16
        assert (sl[int(g[1][0])], sl[int(g[2][0])], 0) in want and (sl[int(g[1][1])], sl[int(g[2][0])], 0) in want
        assert (sl[D], sl[int(g[2][1])], 1) in want and (sl[D], sl[int(g[2][1])], 0) in want and (sl[int(g[2][2])], sl[int(g[2][2])], 0) in want
        assert st["bound_services"] == 26 and st["bound_tasks"] == 25
        for roots in ([A], [B, int(g[2][0])], [A, A, 0x999], [int(g[1][0]), D], [0x999], []):
            for direction in (capi.DEP_CALLEES, capi.DEP_CALLERS, capi.DEP_BOTH):
                for max_hops in (0, 1, 2):
                    _check_deps(w, want, roots, direction, max_hops)
        d = _check_deps(w, want, [A], capi.DEP_CALLEES, 0)
        assert d[sl[D]] == 3 and d[sl[int(g[2][1])]] == 4 and sl[int(g[2][0])] not in d
        assert _check_deps(w, want, [B], capi.DEP_CALLERS, 1) == {sl[B]: 0, sl[A]: 1, sl[D]: 1}
    finally:
        w.close_engine()


def test_edges_follow_the_liveness_of_the_rows(torch_mod):
    w = _world_a()
    try:
        keys, (A, B, Cc, D) = _shapes(w)
        w.report(keys)
        for i in range(4):
            want, st = _check_edges(w)
            assert st["edges"] == 13, i  # the open window and three closes
            w.window_close()
        want, st = _check_edges(w)
        assert st["edges"] == 0 and st["live_rows"] == 0
        assert _check_deps(w, want, [A], capi.DEP_CALLEES, 0) == {w.slot_of[A]: 0}
        w.report(keys[:4])
        want, st = _check_edges(w)
        assert st["edges"] == 4
        assert len(_check_deps(w, want, [A], capi.DEP_CALLEES, 0)) == 4
    finally:
        w.close_engine()


def test_delete_breaks_the_chain_and_a_reused_slot_starts_unbound(torch_mod):
    w = _world_a()
    try:
        keys, (A, B, Cc, D) = _shapes(w)
        w.report(keys)
        want, _ = _check_edges(w)
        assert w.slot_of[D] in _check_deps(w, want, [A], capi.DEP_CALLEES, 0)
        cslot = w.slot_of[Cc]
        w.delete(Cc)
        want, st = _check_edges(w, [dict(src=Cc), dict(dst=Cc)])
        assert not any(cslot in k[:2] for k in want)
        d = _check_deps(w, want, [A, Cc], capi.DEP_CALLEES, 0)  # (C is an unknown root now)
        assert w.slot_of[D] not in d and w.slot_of[B] in d
        # C comes back under host 1 and takes the free slot: it is called again (the rows name its id), it calls nothing until it is bound
        new = w.eng.register_listeners_slots(w.info[1][0], [Cc], wire.listener_netns(1, np.array([40])), wire.listener_port(np.array([40])))
        assert int(new[0]) == cslot
        w.slot_of[Cc] = cslot
        want, st = _check_edges(w, [dict(src=Cc), dict(dst=Cc)])
        assert (w.slot_of[B], cslot, 0) in want and not any(k[0] == cslot for k in want)
        assert w.slot_of[D] not in _check_deps(w, want, [A], capi.DEP_CALLEES, 0)
        w.bind([Cc], [w.T[Cc]])
        want, st = _check_edges(w, [dict(src=Cc)])
        assert (cslot, w.slot_of[D], 0) in want
        assert _check_deps(w, want, [A], capi.DEP_CALLEES, 0)[w.slot_of[D]] == 3
    finally:
        w.close_engine()


def test_set_listener_tasks_later_entry_wins_zero_clears_unknown_changes_nothing(torch_mod):
    w = _world_a()
    try:
        keys, (A, B, Cc, D) = _shapes(w)
        w.report(keys)
        want0, _ = _check_edges(w)
        # A named twice: the later value stays -- A becomes a member of D's group, so it calls what D calls and nothing of its own
        assert w.eng.set_listener_tasks([A, B, A], [0x5555, w.T[B], w.T[D]]) == capi.OK
        w.task[A] = w.T[D]
        want, _ = _check_edges(w, [dict(src=A)])
        assert (w.slot_of[A], w.slot_of[w.svc[19]], 1) in want and (w.slot_of[A], w.slot_of[w.svc[19]], 1) not in want0  # (svc[19] = g[2][1])
        assert (w.slot_of[A], w.slot_of[w.svc[11]], 0) in want0 and (w.slot_of[A], w.slot_of[w.svc[11]], 0) not in want  # (svc[11] = g[1][2]: the fan-out)
        # an unknown id behind a valid entry: GYS_ERR_INVAL, and the valid entry was not applied either
        before = w.eng.svc_edges()[1].tobytes()
        w.bind([B, 0x424242], [0, 7], expect=capi.ERR_INVAL)
        assert b"unknown glob_id" in w.eng.L.gys_last_error()
        assert w.eng.svc_edges()[1].tobytes() == before
        _check_edges(w)
        # 0 clears
        w.bind([A, B], [0, 0])
        want, st = _check_edges(w, [dict(src=B)])
        assert not any(k[0] in (w.slot_of[A], w.slot_of[B]) for k in want) and st["bound_services"] == 24
        w.bind([A], [w.T[A]])
        _check_edges(w)
    finally:
        w.close_engine()


def test_errors_and_the_service_record_does_not_move(torch_mod):
    off = World(3, 9, 0)
    on = World(3, 9, 64)
    try:
        L, h = off.eng.L, off.eng.h
        n32, m32 = C.c_uint32(), C.c_uint32()
        ids = (C.c_uint64 * 2)(off.svc[0], off.svc[1])
        hops = (C.c_uint32 * 4)()
        out = (C.c_uint64 * 4)()
        row = (capi.SvcEdge * 4)()
        st = capi.SvcGraphStats()
        d = torch_mod.zeros(1024, dtype=torch_mod.uint8, device=off.eng.device)
        dp = C.c_void_p(d.data_ptr())
        assert L.gys_set_listener_tasks(h, ids, ids, 2) == capi.ERR_STATE
        assert L.gys_svc_edges_dev(h, None, dp, 4, C.byref(n32)) == capi.ERR_STATE
        assert L.gys_svc_edges(h, None, row, 4, C.byref(n32), C.byref(m32)) == capi.ERR_STATE
        assert L.gys_svcgraph_stats(h, C.byref(st)) == capi.ERR_STATE
        assert L.gys_svc_deps_dev(h, ids, 2, 1, 0, dp, C.byref(n32)) == capi.ERR_STATE
        assert L.gys_svc_deps(h, ids, 2, 1, 0, out, hops, 4, C.byref(n32), C.byref(m32)) == capi.ERR_STATE
        L, h = on.eng.L, on.eng.h
        ids = (C.c_uint64 * 2)(on.svc[0], on.svc[1])
        d = torch_mod.zeros(1024, dtype=torch_mod.uint8, device=on.eng.device)
        dp = C.c_void_p(d.data_ptr())
        blob, state = on.eng.service_blob_bytes(5), on.eng.svc_state_bytes()
        on.bind(on.svc[:6], [7, 7, 8, 9, 10, 11])
        assert on.eng.service_blob_bytes(5) == blob and on.eng.svc_state_bytes() == state
        for bad_dir in (0, 4):
            assert L.gys_svc_deps_dev(h, ids, 2, bad_dir, 0, dp, C.byref(n32)) == capi.ERR_INVAL
            assert L.gys_svc_deps(h, ids, 2, bad_dir, 0, out, hops, 4, C.byref(n32), C.byref(m32)) == capi.ERR_INVAL
        assert L.gys_svc_deps_dev(h, ids, 2, 1, 0, None, C.byref(n32)) == capi.ERR_INVAL
        assert L.gys_svc_deps_dev(h, ids, 2, 1, 0, dp, None) == capi.ERR_INVAL
        assert L.gys_svc_deps_dev(h, None, 1, 1, 0, dp, C.byref(n32)) == capi.ERR_INVAL
        assert L.gys_svc_deps_dev(h, None, 0, 1, 0, dp, C.byref(n32)) == capi.OK and n32.value == 0
        assert L.gys_svc_deps(h, None, 1, 1, 0, out, hops, 4, C.byref(n32), C.byref(m32)) == capi.ERR_INVAL
        assert L.gys_svc_deps(h, ids, 2, 1, 0, out, hops, 4, None, C.byref(m32)) == capi.ERR_INVAL
        assert L.gys_svc_deps(h, ids, 2, 1, 0, out, hops, 4, C.byref(n32), None) == capi.ERR_INVAL
        sel = on.eng.svc_edge_sel(src=on.svc[0])
        sel.struct_size = 8
        assert L.gys_svc_edges_dev(h, C.byref(sel), dp, 4, C.byref(n32)) == capi.ERR_INVAL
        sel = on.eng.svc_edge_sel(src=on.svc[0])
        sel.flags |= 4
        assert L.gys_svc_edges(h, C.byref(sel), row, 4, C.byref(n32), C.byref(m32)) == capi.ERR_INVAL
        assert L.gys_svc_edges_dev(h, None, None, 4, C.byref(n32)) == capi.ERR_INVAL
        assert L.gys_svc_edges_dev(h, None, dp, 4, None) == capi.ERR_INVAL
        assert L.gys_svc_edges(h, None, None, 4, C.byref(n32), C.byref(m32)) == capi.ERR_INVAL
        assert L.gys_svcgraph_stats(h, None) == capi.ERR_INVAL
        assert L.gys_set_listener_tasks(h, None, ids, 2) == capi.ERR_INVAL
        # a graph with nothing in it answers, too
        assert L.gys_svc_deps(h, ids, 2, 3, 0, out, hops, 4, C.byref(n32), C.byref(m32)) == capi.OK and n32.value == 2 and list(hops)[:2] == [0, 0]
        _check_edges(on)
    finally:
        off.close_engine()
        on.close_engine()


# ---------------------------------------------------------------------------------------------------------------- world B
def _world_b(cap):
    w = World(4, 80, cap)
    w.T = {s: 0xA000 + w.slot_of[s] for s in w.svc}
    return w


def test_2000_random_rows_and_a_group_of_70_listeners(torch_mod):
    w = _world_b(4096)
    try:
        for s in w.svc[100:170]:
            w.T[s] = 0x7070  # 70 callers from one row: more than a wave of emits
        for s in w.svc[300:310]:
            del w.T[s]
        w.bind(list(w.T), list(w.T.values()))
        rng = np.random.default_rng(77)
        lids = w.svc + [0x5000 + i for i in range(20)]
        cids = sorted(set(w.T.values())) + [0x7070] * 30 + [0xDEAD00 + i for i in range(20)] + [0]
        keys = [(lids[int(rng.integers(len(lids)))], cids[int(rng.integers(len(cids)))], int(rng.random() < 0.25)) for _ in range(2000)]
        w.report(keys[:1000], host=0)
        w.report(keys[1000:], host=3)  # (repeated keys add within the window)
        some = [w.svc[120], w.svc[5], w.svc[305], keys[0][0]]
        want, st = _check_edges(w, [dict(src=some[0]), dict(dst=some[1]), dict(src=some[2]), dict(dst=some[3])])
        assert st["edges"] > 4000 and st["rows_no_listener"] > 50 and st["rows_no_client"] > 50 and st["bound_tasks"] == 241 and st["bound_services"] == 310
        for roots in ([w.svc[0]], [w.svc[120], w.svc[7], w.svc[319]]):
            for direction in (1, 2, 3):
                for max_hops in (0, 1, 2, 3):
                    _check_deps(w, want, roots, direction, max_hops)
    finally:
        w.close_engine()


def test_a_chain_300_hops_long(torch_mod):
    w = _world_b(4096)
    try:
        w.bind(list(w.T), list(w.T.values()))
        order = [w.svc[(i * 37) % 320] for i in range(301)]  # (37 is prime to 320: 301 distinct services, in no slot order)
        assert len(set(order)) == 301
        w.report([(order[i + 1], w.T[order[i]], 0) for i in range(300)])
        want, st = _check_edges(w)
        assert st["edges"] == 300
        d = _check_deps(w, want, [order[0]], capi.DEP_CALLEES, 0)
        assert len(d) == 301 and d[w.slot_of[order[300]]] == 300
        d = _check_deps(w, want, [order[0]], capi.DEP_CALLEES, 299)
        assert len(d) == 300 and w.slot_of[order[300]] not in d
        d = _check_deps(w, want, [order[300]], capi.DEP_CALLERS, 0)
        assert d[w.slot_of[order[0]]] == 300
        d = _check_deps(w, want, [order[150]], capi.DEP_BOTH, 0)
        assert len(d) == 301 and max(d.values()) == 150
    finally:
        w.close_engine()


def test_a_table_rebuild_between_binding_and_query(torch_mod):
    w = _world_b(128)
    try:
        w.bind(list(w.T), list(w.T.values()))
        rng = np.random.default_rng(9)
        used = set()
        for win in range(12):
            keys = []
            while len(keys) < 32:
                k = (w.svc[int(rng.integers(320))], w.T[w.svc[int(rng.integers(320))]], int(rng.random() < 0.2))
                if k not in used:
                    used.add(k)
                    keys.append(k)
            w.report(keys, host=win % 4)
            want, st = _check_edges(w)
            assert st["edges"] == st["live_rows"] == min(win + 1, 4) * 32
            _check_deps(w, want, [keys[0][0], keys[5][0]], capi.DEP_BOTH, 0)
            _check_deps(w, want, [keys[1][0]], capi.DEP_CALLERS, 2)
            w.window_close()
        ts = w.eng.actconn_table_stats()
        assert ts["rebuilds"] >= 1 and ts["rows_dropped"] == 0, ts
    finally:
        w.close_engine()
