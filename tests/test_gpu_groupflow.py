"""Group flow map on the GPU (gyeeta_amd/csrc/gys_groupflow.hpp): gys_group_edges_dev, gys_group_edges, gys_group_deps_dev and
gys_group_deps against the Python edge dictionary of the definition ("Service dependency graph" and "Group flow map" in
include/gysketch.h) and a deque BFS over its group pairs.  Every comparison is exact.  World A: 3 hosts x 9 services in 2 clusters;
world B: 4 hosts x 80 services.  The small model class is a copy of the one in tests/test_gpu_svccomp.py, with the groups added.

A label at or above the label domain cannot be produced through the library's calls (gys_set_service_groups and
gys_label_service_components raise the domain above every label they set); that half of "in no group" is run by
tests/cpp/kemu/test_groupflow.cc on the kernels themselves.  Slots without a label are covered here."""
import ctypes as C
from collections import defaultdict, deque

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

RING = 3  # GYS_ACT_RING
T0 = 1_700_000_000_000_000
M64 = 0xFFFFFFFFFFFFFFFF
GROUPINGS = (capi.GROUP_HOST, capi.GROUP_CLUSTER, capi.GROUP_LABEL)  # (the order the groupings are checked in)
FIGS = ("nedges", "nrows", "active_conns", "bytes_sent", "bytes_received", "last_window", "kinds", "flags")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


class World:
    """an engine, and the model beside it: the row table (key -> latest report), the registry (glob_id -> slot), the bindings, the groups"""

    def __init__(self, nh, sp, cap, spare=8, cluster_of=None, **kw):
        from gyeeta_amd.engine import SketchEngine
        self.eng = SketchEngine(max_hosts=nh, max_services=nh * sp + spare, enable_tdigest=False, actconn_pair_cap=cap, **kw)
        self.nh, self.sp = nh, sp
        cluster_of = cluster_of or (lambda h: "cl%d" % (h % 2))
        self.info, self.gids = helpers.register_world(self.eng, None, range(nh), sp, cluster_of=cluster_of)
        self.svc = [int(g) for h in range(nh) for g in self.gids[h]]
        self.slot_of = {g: self.eng.lookup(g) for g in self.svc}
        self.host_of = {int(g): self.info[h][1] for h in range(nh) for g in self.gids[h]}  # glob_id -> host slot
        names = []
        for h in range(nh):  # (a cluster's index is the order of its first registration)
            if cluster_of(h) not in names:
                names.append(cluster_of(h))
        self.cluster_of_host = {self.info[h][1]: names.index(cluster_of(h)) for h in range(nh)}
        self.nclusters = len(names)
        self.label = {}  # glob_id -> label (absent: none)
        self.label_domain = 0
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

    def set_labels(self, ids, labels):
        self.eng.set_service_groups(ids, np.array(labels, dtype=np.uint32))
        for g, l in zip(ids, labels):
            if l == capi.NO_GROUP:
                self.label.pop(int(g), None)
            else:
                self.label[int(g)] = int(l)
                self.label_domain = max(self.label_domain, int(l) + 1)

    def report(self, keys, host=0):
        """one call with one row per (listener id, client id, kind[, more flag bits]) of `keys`, random figures"""
        n = len(keys)
        rec = np.zeros(n, dtype=wire.ACTIVE_CONN_STATS)
        rec["listener_glob_id"] = np.array([k[0] for k in keys], dtype=np.uint64)
        rec["cli_aggr_task_id"] = np.array([k[1] for k in keys], dtype=np.uint64)
        rec["bytes_sent"] = self.rng.integers(0, 1 << 40, n)
        rec["bytes_received"] = self.rng.integers(0, 1 << 40, n)
        rec["active_conns"] = self.rng.integers(0, 500, n)
        rec["flags"] = np.array([(wire.ACTIVE_FLAG_REMOTE_LISTEN if k[2] else 0) | (k[3] if len(k) > 3 else 0) for k in keys], dtype=np.uint8)
        self.eng.handle_partha_active_conns(self.info[host][0], rec.tobytes(), n)
        for r in rec:
            k = (int(r["listener_glob_id"]), int(r["cli_aggr_task_id"]), (int(r["flags"]) >> 1) & 1)
            e = self.ent.get(k)
            if e is None or e["window"] != self.epoch:
                e = self.ent[k] = dict(window=self.epoch, active_conns=0, bytes_sent=0, bytes_received=0, flags=0)
            e["active_conns"] += int(r["active_conns"])
            e["bytes_sent"] += int(r["bytes_sent"])
            e["bytes_received"] += int(r["bytes_received"])
            e["flags"] |= int(r["flags"])

    def window_close(self):
        self.eng.window_close(T0 + self.nclose * 5_000_000)
        self.nclose += 1
        self.epoch += 1

    def delete(self, gid):
        assert self.eng.delete_listeners([gid]) == 1
        del self.slot_of[gid]
        self.task.pop(gid, None)
        self.label.pop(gid, None)

    # ---- the definition
    def entries(self):
        """the live entries that give an edge: (listener slot v, the caller slots, the entry, its kind)"""
        bound = defaultdict(list)
        for g, t in self.task.items():
            if t and g in self.slot_of:
                bound[t].append(self.slot_of[g])
        for (lid, cid, kind), e in self.ent.items():
            if self.epoch - e["window"] > RING or lid not in self.slot_of or cid == 0 or cid not in bound:
                continue
            yield self.slot_of[lid], bound[cid], e, kind

    def domain(self, group_by):
        return {capi.GROUP_HOST: self.nh, capi.GROUP_CLUSTER: self.nclusters, capi.GROUP_LABEL: self.label_domain}[group_by]

    def groups(self, group_by):
        """slot -> group, of the slots that are in one"""
        out = {}
        for g, s in self.slot_of.items():
            if group_by == capi.GROUP_HOST:
                out[s] = self.host_of[g]
            elif group_by == capi.GROUP_CLUSTER:
                out[s] = self.cluster_of_host[self.host_of[g]]
            elif g in self.label and self.label[g] < self.label_domain:
                out[s] = self.label[g]
        return out

    def flow(self, group_by):
        """(gu, gv) -> the figures of the group edge; the stats"""
        grp = self.groups(group_by)
        gm, edges, nog = {}, 0, 0
        for v, callers, e, kind in self.entries():
            gv, seen = grp.get(v), set()
            for u in callers:
                edges += 1
                gu = grp.get(u)
                if gu is None or gv is None:
                    nog += 1
                    continue
                r = gm.setdefault((gu, gv), dict.fromkeys(FIGS, 0))
                r["nedges"] += 1
                seen.add(gu)
            for gu in seen:  # once per entry and group edge
                r = gm[(gu, gv)]
                r["nrows"] += 1
                for k in ("active_conns", "bytes_sent", "bytes_received"):
                    r[k] = (r[k] + e[k]) & M64
                r["last_window"] = max(r["last_window"], e["window"])
                r["kinds"] |= 1 << kind
                r["flags"] |= e["flags"]
        st = dict(edges=edges, edges_no_group=nog, group_edges=len(gm), self_group_edges=sum(a == b for a, b in gm))
        return gm, st


def _sel_match(src, dst, no_self, gu, gv):
    return (src is None or gu == src) and (dst is None or gv == dst) and not (no_self and gu == gv)


def _rows_equal(rows, want, gm):
    assert [(int(r["src_group"]), int(r["dst_group"])) for r in rows] == want
    for r in rows:
        key = (int(r["src_group"]), int(r["dst_group"]))
        assert int(r["reserved"]) == 0 and not r["pad"].any()
        for k in FIGS:
            assert int(r[k]) == gm[key][k], (key, k, int(r[k]), gm[key][k])


def _check(w, group_by, src=None, dst=None, no_self=False):
    """the device form, the count form and the host form (with its order) under one selection; the stats of the whole map"""
    eng = w.eng
    gm, st = w.flow(group_by)
    assert st["edges"] == eng.svcgraph_stats()["edges"]
    sel = None if (src is None and dst is None and not no_self) else eng.group_edge_sel(src, dst, no_self)
    want = sorted(k for k in gm if _sel_match(src, dst, no_self, *k))
    t, nmatch, dst_stats = eng.group_edges_dev(group_by, sel, cap=len(want) + 2)
    eng.sync()
    assert nmatch == len(want) and dst_stats == st, (group_by, nmatch, len(want), dst_stats, st)
    raw = np.frombuffer(t.cpu().numpy().tobytes(), dtype=eng.GROUP_EDGE_DT)
    rows = raw[:nmatch]
    _rows_equal(rows[np.lexsort((rows["dst_group"], rows["src_group"]))], want, gm)
    assert not raw[nmatch:].view(np.uint8).any()  # (nothing behind the matches)
    _, ncount, cst = eng.group_edges_dev(group_by, sel, 0)
    assert ncount == len(want) and cst == st
    rc, hrows, hmatch, hst = eng.group_edges(group_by, sel, cap=len(want))
    assert rc == capi.OK and hmatch == len(want) and hst == st
    _rows_equal(hrows, want, gm)
    if want:  # one short of room: nothing but the counts is written
        out = (capi.GroupEdge * len(want))()
        C.memset(out, 0x5A, C.sizeof(out))
        nout, nm, gst = C.c_uint32(9), C.c_uint32(), capi.GroupFlowStats()
        assert eng.L.gys_group_edges(eng.h, group_by, C.byref(sel) if sel is not None else None, out, len(want) - 1, C.byref(nout), C.byref(nm), C.byref(gst)) == capi.ERR_NOMEM
        assert nout.value == 0 and nm.value == len(want) and bytes(out) == b"\x5a" * C.sizeof(out)
    return gm, st


def _check_all(w):
    return [_check(w, gb) for gb in GROUPINGS]


def _bfs(gm, ndomain, roots, direction, max_hops):
    hops = {r: 0 for r in roots if r < ndomain}
    q = deque(sorted(hops))
    while q:
        x = q.popleft()
        if max_hops and hops[x] >= max_hops:
            continue
        for gu, gv in gm:
            if gu == gv:
                continue
            for a, b, bit in ((gu, gv, capi.DEP_CALLEES), (gv, gu, capi.DEP_CALLERS)):
                if (direction & bit) and a == x and b not in hops:
                    hops[b] = hops[x] + 1
                    q.append(b)
    return hops


def _check_deps(w, group_by, roots):
    eng = w.eng
    gm, _ = w.flow(group_by)
    nd = w.domain(group_by)
    for direction in (capi.DEP_CALLEES, capi.DEP_CALLERS, capi.DEP_BOTH):
        for max_hops in (0, 1, 2):
            want = _bfs(gm, nd, roots, direction, max_hops)
            t, n = eng.group_deps_dev(group_by, roots, direction, max_hops)
            eng.sync()
            got = t.cpu().numpy().view(np.uint32)
            exp = np.full(nd, capi.NOSLOT, dtype=np.uint32)
            for g, h in want.items():
                exp[g] = h
            assert len(got) == nd and np.array_equal(got, exp) and n == len(want), (group_by, roots, direction, max_hops, got, exp)
            rc, groups, hops, nr = eng.group_deps(group_by, roots, direction, max_hops)
            assert rc == capi.OK and nr == len(want)
            assert list(zip(hops.tolist(), groups.tolist())) == sorted((h, g) for g, h in want.items())
            if len(want) > 1:
                rc, groups, hops, nr = eng.group_deps(group_by, roots, direction, max_hops, cap=len(want) - 1)
                assert rc == capi.ERR_NOMEM and nr == len(want) and len(groups) == 0


# ---------------------------------------------------------------------------------------------------------------- world A
def _world_a(cap=512, **kw):
    w = World(3, 9, cap, **kw)
    g = w.gids
    w.T = {s: 0xA000 + w.slot_of[s] for s in w.svc}
    for s in (int(g[1][0]), int(g[1][1]), int(g[0][5])):
        w.T[s] = 0xBEEF  # one task group with listeners on two hosts, two of them on one host
    del w.T[int(g[2][8])]  # never bound
    w.bind(list(w.T), list(w.T.values()))
    return w


def _shapes(w):
    g = w.gids
    A, B, Cc, D = (int(g[0][i]) for i in range(4))
    T = w.T
    keys = [(B, T[A], 0), (Cc, T[B], 0), (D, T[Cc], 0)]                          # a chain on host 0: gu == gv with u != v
    keys += [(int(g[1][k]), T[A], 0) for k in range(2, 4)]                       # host 0 -> host 1, twice
    keys += [(int(g[2][0]), 0xBEEF, 0)]                                           # one entry, three edges: hosts 1, 1 and 0 call host 2
    keys += [(Cc, 0xDEAD, 0), (0x1234567, T[A], 0), (B, 0, 0)]                    # rows that give no edge
    keys += [(int(g[2][1]), T[int(g[1][3])], 1, 1), (int(g[2][1]), T[int(g[1][3])], 0, 4)]  # one pair in both kinds, other flag bits
    keys += [(int(g[2][2]), T[int(g[2][2])], 0)]                                  # u == v
    keys += [(int(g[1][6]), T[int(g[2][7])], 1)]                                  # host 2 -> host 1 by a kind-1 row alone
    return keys


def test_three_groupings_selections_expiry_deletes_and_a_new_binding(torch_mod):
    w = _world_a()
    try:
        g, sl, eng = w.gids, w.slot_of, w.eng
        keys = _shapes(w)
        for gb in GROUPINGS:  # nothing reported
            gm, st = _check(w, gb)
            assert not gm and st["edges"] == 0
        w.report(keys[:7], host=0)
        w.report(keys[7:], host=2)
        (hm, hst), (cm, cst), (lm, lst) = _check_all(w)
        h = {i: w.info[i][1] for i in range(3)}
        # the 0xBEEF entry: figures once per distinct pair, nedges per edge
        beef = w.ent[(int(g[2][0]), 0xBEEF, 0)]
        assert hm[(h[1], h[2])]["nedges"] >= 2 and hm[(h[0], h[2])]["nedges"] == 1 and hm[(h[0], h[2])]["nrows"] == 1
        assert hm[(h[0], h[2])]["bytes_sent"] == beef["bytes_sent"]
        both = hm[(h[1], h[2])]  # ... and the pair in both kinds sits in the same group edge
        assert both["kinds"] == 3 and both["flags"] & 7 == 7 and both["nrows"] == 3 and both["nedges"] == 4
        assert (h[0], h[0]) in hm and hm[(h[0], h[0])]["nedges"] == 3 and (h[2], h[2]) in hm and hst["self_group_edges"] == 2
        assert hst["edges"] == 12 and hst["edges_no_group"] == 0 and sorted(cm) == [(0, 0), (0, 1), (1, 0)] and cm[(1, 0)]["nedges"] == 4 and cm[(1, 0)]["nrows"] == 3
        # LABEL before any label was set: GYS_OK, zero rows, every edge in no group
        assert not lm and lst["edges_no_group"] == lst["edges"] == hst["edges"] > 0
        _check_deps(w, capi.GROUP_LABEL, [0, 3])
        # labels: a third of the services have none, and no service has label 5
        lab = [capi.NO_GROUP if i % 3 == 2 or (i * 7) % 11 == 5 else (i * 7) % 11 for i in range(len(w.svc))]
        w.set_labels(w.svc, lab)
        lm, lst = _check(w, capi.GROUP_LABEL)
        assert lm and 0 < lst["edges_no_group"] < lst["edges"] and w.label_domain == 11
        # selections: each flag, combined, a group that does not exist
        for gb, gm in ((capi.GROUP_HOST, hm), (capi.GROUP_CLUSTER, cm), (capi.GROUP_LABEL, lm)):
            a, z = min(gm)[0], max(gm)[1]
            for src, dst, ns in ((a, None, False), (None, z, False), (a, z, False), (None, None, True), (a, None, True), (None, z, True), (a, a, True),
                                 (w.domain(gb) + 3, None, False), (None, capi.NO_GROUP, False)):
                _check(w, gb, src, dst, ns)
        # the search: three directions, max_hops 0 / 1 / 2, a root named twice, a root outside the domain, a group with no member
        _check_deps(w, capi.GROUP_HOST, [h[0], h[0], 77])
        _check_deps(w, capi.GROUP_HOST, [h[2]])
        _check_deps(w, capi.GROUP_CLUSTER, [1, 5])
        lroots = [min(lm)[0], min(lm)[0], w.label_domain + 1]
        empty_label = [x for x in range(w.label_domain) if x not in set(w.label.values())]
        assert empty_label == [5]
        _check_deps(w, capi.GROUP_LABEL, lroots + empty_label)
        _check_deps(w, capi.GROUP_LABEL, [])
        # a window close changes nothing while the rows live; after four they have expired
        w.window_close()
        assert [m for m, _ in _check_all(w)] == [hm, cm, lm]
        for _ in range(3):
            w.window_close()
        for gm, st in _check_all(w):
            assert not gm and st == dict(edges=0, edges_no_group=0, group_edges=0, self_group_edges=0)
        # deletes: a caller (B calls C) and a listener (the one the 0xBEEF group calls)
        w.report(keys)
        before = _check_all(w)
        w.delete(int(g[0][1]))
        w.delete(int(g[2][0]))
        after = _check_all(w)
        assert after[0][1]["edges"] == before[0][1]["edges"] - 5 and (h[0], h[2]) not in after[0][0]
        # a new binding: the unbound service of host 2 joins the 0xBEEF group (a third host), which calls a host-1 service now
        w.bind([int(g[2][8])], [0xBEEF])
        w.report([(int(g[1][5]), 0xBEEF, 0)])
        hm2, _ = _check(w, capi.GROUP_HOST)
        assert hm2[(h[2], h[1])]["nedges"] == after[0][0][(h[2], h[1])]["nedges"] + 1 and hm2[(h[1], h[1])]["nedges"] == 2 and hm2[(h[1], h[1])]["nrows"] == 1
        _check(w, capi.GROUP_CLUSTER)
        _check(w, capi.GROUP_LABEL)
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- world B
def _world_b(cap=4096):
    w = World(4, 80, cap)
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
    w.T = T
    return w


def test_world_b_every_grouping_and_the_components_as_groups(torch_mod):
    w = _world_b()
    try:
        eng, T = w.eng, w.T
        rng = np.random.default_rng(5)
        groups = sorted(set(T[s] for s in w.svc[:300]))
        keys = {(w.svc[int(rng.integers(280))], groups[int(rng.integers(len(groups)))], int(rng.random() < 0.25)) for _ in range(300)}
        keys |= {(w.svc[301], T[w.svc[302]], 0), (w.svc[303], T[w.svc[302]], 1), (w.svc[310], T[w.svc[310]], 0)}
        keys |= {(0x5000 + j, groups[0], 0) for j in range(10)} | {(w.svc[5], 0xDEAD00 + j, 0) for j in range(10)}
        keys = sorted(keys)
        w.report(keys[:160], host=0)
        w.report(keys[160:], host=3)
        w.set_labels(w.svc, [capi.NO_GROUP if i % 5 == 4 else i % 37 for i in range(len(w.svc))])
        (hm, hst), (cm, cst), (lm, lst) = _check_all(w)
        assert hst["edges"] >= 4096 and len(hm) >= 9 and len(cm) == 4 and len(lm) > 500 and lst["edges_no_group"] > 0
        # (task groups straddle host boundaries: an entry counts once for each host its callers sit on)
        assert sum(r["nrows"] for r in hm.values()) > sum(1 for _ in w.entries())
        _check_deps(w, capi.GROUP_HOST, [w.info[3][1]])
        _check_deps(w, capi.GROUP_LABEL, [0, 36, 36])
        # the components as labels: every group edge stays inside a group, and a root's row carries the component's figures
        ngroups = eng.label_service_components(1)
        rc, comps, nmatch, ncomp = eng.svc_components(1)
        assert rc == capi.OK and ngroups == nmatch == ncomp
        rc, rows, nm, st = eng.group_edges(capi.GROUP_LABEL)
        assert rc == capi.OK and nm == len(rows) == st["group_edges"] == st["self_group_edges"] and st["edges_no_group"] == 0
        assert (rows["src_group"] == rows["dst_group"]).all()
        rc, none, nm0, _ = eng.group_edges(capi.GROUP_LABEL, eng.group_edge_sel(no_self=True))
        assert rc == capi.OK and nm0 == 0 and len(none) == 0
        by_root = {int(r["src_group"]): r for r in rows}
        with_rows = [c for c in comps if int(c["nrows"])]
        assert sorted(by_root) == sorted(int(c["root_slot"]) for c in with_rows) and len(with_rows) >= 3
        for c in with_rows:
            r = by_root[int(c["root_slot"])]
            for k in ("nrows", "nedges", "active_conns", "bytes_sent", "bytes_received"):
                assert int(r[k]) == int(c[k]), (int(c["root_slot"]), k, int(r[k]), int(c[k]))
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- the contention range
def test_a_tile_on_one_key_and_a_tile_past_its_lds_table(torch_mod):
    # every live entry of a 256-entry tile maps to ONE group pair: one cluster, a table of one tile
    w = World(4, 80, 128, cluster_of=lambda h: "only")
    try:
        assert w.eng.actconn_table_stats()["entries"] == 256  # (the whole table is one tile of k_gf_accum)
        T = {s: 0xA000 + w.slot_of[s] for s in w.svc}
        for s in w.svc[100:170]:
            T[s] = 0x7070  # the 70-listener task
        w.bind(list(T), list(T.values()))
        rng = np.random.default_rng(11)
        keys = sorted({(w.svc[int(rng.integers(320))], 0xA000 + int(rng.integers(320)), int(rng.random() < 0.3)) for _ in range(110)})
        w.report(keys)
        gm, st = _check(w, capi.GROUP_CLUSTER)
        assert len(gm) == 1 and gm[(0, 0)]["nedges"] == st["edges"] >= 50 and gm[(0, 0)]["nrows"] == gm[(0, 0)]["nedges"]
        _check(w, capi.GROUP_HOST)
        # the 70-listener task, each listener with its own label, called by 12 rows of the one tile: 840 distinct pairs
        for _ in range(4):
            w.window_close()
        w.set_labels(w.svc, list(range(len(w.svc))))
        w.report([(w.svc[i], 0x7070, i & 1) for i in range(12)])
        gm, st = w.flow(capi.GROUP_LABEL)
        pairs_in_the_tile = len(gm)  # (one tile holds every entry)
        assert w.eng.actconn_table_stats()["entries"] == 256 and pairs_in_the_tile > capi.GF_LDS_KEYS, \
            "scenario no longer reaches its edge: %d distinct pairs in the tile, the LDS table holds %d" % (pairs_in_the_tile, capi.GF_LDS_KEYS)
        gm, st = _check(w, capi.GROUP_LABEL)
        assert len(gm) == 840 and st["edges"] == 840 and all(r["nedges"] == 1 and r["nrows"] == 1 for r in gm.values())
        hm, _ = _check(w, capi.GROUP_HOST)  # the same entries by host: 70 edges and ONE flow per entry and calling host
        assert hm[(w.info[1][1], w.info[0][1])]["nedges"] == 12 * 60 and hm[(w.info[1][1], w.info[0][1])]["nrows"] == 12
        assert hm[(w.info[2][1], w.info[0][1])]["nedges"] == 12 * 10 and hm[(w.info[2][1], w.info[0][1])]["nrows"] == 12
    finally:
        w.close_engine()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_nothing_is_modified(torch_mod):
    off = World(3, 9, 0)
    on = _world_a(64)
    try:
        n1, n2, n3 = C.c_uint32(5), C.c_uint32(5), C.c_uint32(5)
        st = capi.GroupFlowStats()
        out = (capi.GroupEdge * 4)()
        d = torch_mod.zeros(1024, dtype=torch_mod.int32, device=off.eng.device)
        dp = C.c_void_p(d.data_ptr())
        roots = (C.c_uint32 * 2)(0, 1)
        gbuf, hbuf = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
        H = capi.GROUP_HOST
        L, h = off.eng.L, off.eng.h
        assert L.gys_group_edges_dev(h, H, None, None, 0, C.byref(n1), None) == capi.ERR_STATE
        assert L.gys_group_edges(h, H, None, out, 4, C.byref(n1), C.byref(n2), C.byref(st)) == capi.ERR_STATE
        assert L.gys_group_deps_dev(h, H, roots, 2, 1, 0, dp, C.byref(n1), C.byref(n2)) == capi.ERR_STATE
        assert L.gys_group_deps(h, H, roots, 2, 1, 0, gbuf, hbuf, 8, C.byref(n1), C.byref(n2)) == capi.ERR_STATE
        L, h = on.eng.L, on.eng.h
        on.report(_shapes(on))
        ts, edges = on.eng.actconn_table_stats(), on.eng.svc_edges()[1].tobytes()
        sel = on.eng.group_edge_sel(src=0)
        assert L.gys_group_edges_dev(h, capi.GROUP_NONE, None, None, 0, C.byref(n1), None) == capi.ERR_INVAL
        assert L.gys_group_edges_dev(h, 4, None, None, 0, C.byref(n1), None) == capi.ERR_INVAL
        assert L.gys_group_edges(h, capi.GROUP_NONE, None, out, 4, C.byref(n1), C.byref(n2), None) == capi.ERR_INVAL
        assert L.gys_group_deps_dev(h, capi.GROUP_NONE, roots, 2, 1, 0, dp, None, C.byref(n2)) == capi.ERR_INVAL
        assert L.gys_group_deps(h, capi.GROUP_NONE, roots, 2, 1, 0, gbuf, hbuf, 8, C.byref(n1), C.byref(n2)) == capi.ERR_INVAL
        sel.struct_size = 12
        assert L.gys_group_edges_dev(h, H, C.byref(sel), None, 0, C.byref(n1), None) == capi.ERR_INVAL
        assert L.gys_group_edges(h, H, C.byref(sel), out, 4, C.byref(n1), C.byref(n2), None) == capi.ERR_INVAL
        sel.struct_size, sel.flags = C.sizeof(capi.GroupEdgeSel), 8
        assert L.gys_group_edges_dev(h, H, C.byref(sel), None, 0, C.byref(n1), None) == capi.ERR_INVAL
        assert L.gys_group_edges_dev(h, H, None, None, 4, C.byref(n1), None) == capi.ERR_INVAL   # cap > 0 without a buffer
        assert L.gys_group_edges(h, H, None, None, 4, C.byref(n1), C.byref(n2), None) == capi.ERR_INVAL
        assert L.gys_group_edges_dev(h, H, None, None, 0, None, None) == capi.ERR_INVAL
        assert L.gys_group_edges(h, H, None, out, 4, None, C.byref(n2), None) == capi.ERR_INVAL
        for bad_dir in (0, 4):
            assert L.gys_group_deps_dev(h, H, roots, 2, bad_dir, 0, dp, None, C.byref(n2)) == capi.ERR_INVAL
            assert L.gys_group_deps(h, H, roots, 2, bad_dir, 0, gbuf, hbuf, 8, C.byref(n1), C.byref(n2)) == capi.ERR_INVAL
        assert L.gys_group_deps_dev(h, H, roots, 2, 1, 0, None, None, C.byref(n2)) == capi.ERR_INVAL
        assert L.gys_group_deps_dev(h, H, None, 2, 1, 0, dp, None, C.byref(n2)) == capi.ERR_INVAL
        assert L.gys_group_deps(h, H, roots, 2, 1, 0, None, hbuf, 8, C.byref(n1), C.byref(n2)) == capi.ERR_INVAL
        # the host form with cap below nmatch: GYS_ERR_NOMEM, out untouched
        C.memset(out, 0x5A, C.sizeof(out))
        n1 = C.c_uint32(9)
        assert L.gys_group_edges(h, H, None, out, 2, C.byref(n1), C.byref(n2), C.byref(st)) == capi.ERR_NOMEM
        assert n1.value == 0 and n2.value > 2 and st.group_edges == n2.value and bytes(out) == b"\x5a" * C.sizeof(out)
        assert L.gys_group_edges(h, H, None, None, 0, C.byref(n1), C.byref(n3), None) == capi.ERR_NOMEM and n3.value == n2.value  # (a count)
        # stats NULL, ndomain NULL: fine; no call modified anything
        assert L.gys_group_edges_dev(h, H, None, None, 0, C.byref(n1), None) == capi.OK and n1.value == n2.value
        assert L.gys_group_deps_dev(h, H, roots, 2, 3, 0, dp, None, C.byref(n2)) == capi.OK and n2.value == 3
        _check_all(on)
        assert on.eng.actconn_table_stats() == ts and on.eng.svc_edges()[1].tobytes() == edges and len(edges) > 0
    finally:
        off.close_engine()
        on.close_engine()
