"""One registry generation invalidates every cached member list: the fixed scopes (host, cluster, this rank) of the digest, distinct-count
and level-histogram roll-ups and the all-hosts top-N, walked through every kind of registry change.

World: 34 hosts in 2 clusters (33 + 1); host 0 has 1025 services (two chunks of the 1024-member service lists), every other host 2; the
cluster of 33 hosts takes two chunks of the 32-slab lists of the digest roll-up.  Steps, with every roll-up read after each:
  1. register;
  2. listeners of three hosts are deleted and others registered into the freed slots, the service count ending where it was (host 2 then holds
     a LOWER slot behind a higher one, slots of host 0 belong to hosts 1 and 2 and the other way round);
  3. one host moves to the other cluster;
  4. one new host without services is registered.
Expected values come from the per-service exports (export_hist_level, export_svc_hll, export_svc_hll_level, export_tdigest) over the members the
test itself keeps, exact equality as in tests/test_gpu_listener_delete.py::_check_fixed_rollups: histograms and register files in numpy; the
digests' weights and extremes in numpy, their bytes against the filtered roll-up (host scope: it selects its members afresh) and
against gys_tdigest_merge_slabs_dev over the member hosts' slabs picked here (cluster, rank); the top-N by metric, ties by lower slot."""
import json

import numpy as np
import pytest

from gyeeta_amd import capi, wire

pytestmark = pytest.mark.gpu

NH, NBIG, NSMALL = 34, 1025, 2
T0 = 1_700_000_000
I64MIN = np.iinfo(np.int64).min


def _listeners(h, svc):
    svc = np.asarray(svc)
    return wire.glob_id(np.full(len(svc), h), svc), wire.listener_netns(h, svc), wire.listener_port(svc)


def _events(rng, h, svc, per):
    svc = np.repeat(np.asarray(svc), per)
    n = len(svc)
    ev = np.zeros(n, dtype=wire.RESP_EVENT)
    _, ev["netns"], ev["sport_be"] = _listeners(h, svc)
    ev["saddr"] = np.full(n, 0x0A000000 | h, dtype=np.uint32).astype(">u4").view("<u4")
    ev["daddr"] = (0x0A000000 | rng.integers(1, 1 << 24, n)).astype(">u4").view("<u4")
    ev["dport_be"] = rng.integers(16000, 65536, n)
    lat = np.minimum(np.floor(rng.lognormal(3.0, 1.5, n)), 1e6).astype(np.uint32)
    lrcv = rng.integers(0, 1 << 31, n).astype(np.uint32)
    ev["lrcvtime"], ev["lsndtime"] = lrcv, lrcv + lat
    return ev


def _np_sum(recs):
    """GY_HISTOGRAM::add_histogram over [n][16][2] int64 records"""
    out = np.zeros((16, 2), dtype=np.int64)
    out[15, 1] = I64MIN
    if len(recs):
        out = recs.sum(axis=0, dtype=np.int64)
        out[15, 1] = recs[:, 15, 1].max()
    return out


class World:
    def __init__(self, eng):
        self.eng, self.rng, self.t = eng, np.random.default_rng(7), T0
        self.mids = {}
        self.cluster = {}  # host slot -> cluster index
        self.svcs = {}     # host slot -> {service index: slot}
        self.qps = {}      # slot -> (nqrys_5s, glob id) reported in the window closed last

    def add_host(self, h, cluster):
        self.mids[h] = wire.machine_id(h)
        assert self.eng.register_host(self.mids[h], "cl%d" % cluster) == h
        self.cluster[h] = cluster
        self.svcs.setdefault(h, {})

    def add_listeners(self, h, svc):
        slots = self.eng.register_listeners_slots(self.mids[h], *_listeners(h, svc))
        self.svcs[h].update(zip((int(s) for s in svc), (int(x) for x in slots)))
        return slots

    def delete(self, h, svc):
        assert self.eng.delete_listeners(_listeners(h, svc)[0]) == len(svc)
        for s in svc:
            self.qps.pop(self.svcs[h].pop(int(s)), None)

    def feed(self, per):
        """response events for every service (a few thousand in all); host 0's services get one event each"""
        for h in self.svcs:
            if self.svcs[h]:
                self.eng.handle_resp_events(self.mids[h], _events(self.rng, h, sorted(self.svcs[h]), 1 if h == 0 else per))

    def states_and_close(self):
        """every service reports a small query rate (many ties: the top-N order then hangs on the slot order of the member lists)"""
        for h in self.svcs:
            svc = np.array(sorted(self.svcs[h]), dtype=np.int64)
            if not len(svc):
                continue
            rec = wire.synth_listener_states(self.rng, h, svc)
            rec["nqrys_5s"] = self.rng.integers(5, 9, len(svc))
            for i in range(0, len(rec), 512):
                self.eng.partha_listener_state(self.mids[h], rec[i:i + 512].tobytes(), len(rec[i:i + 512]))
            for s, r in zip(svc, rec):
                self.qps[self.svcs[h][int(s)]] = (int(r["nqrys_5s"]), int(r["glob_id"]))
        self.eng.window_close(self.t * 1_000_000)
        self.t += 31

    def members(self, scope):
        """group -> service slots (sorted)"""
        host = {h: np.array(sorted(self.svcs[h].values()), dtype=np.int64) for h in sorted(self.svcs)}
        if scope == capi.ROLLUP_HOST:
            return host
        groups = {0: sorted(host)} if scope == capi.ROLLUP_GLOBAL else {c: [h for h in sorted(host) if self.cluster[h] == c] for c in (0, 1)}
        return {g: np.concatenate([host[h] for h in hs] + [np.zeros(0, dtype=np.int64)]) for g, hs in groups.items()}

    def check(self, what):
        eng, tusec, n = self.eng, self.t * 1_000_000, self.eng.num_services()
        scopes = (capi.ROLLUP_HOST, capi.ROLLUP_CLUSTER, capi.ROLLUP_GLOBAL)
        hosts = self.members(capi.ROLLUP_HOST)
        assert eng.L.gys_num_hosts(eng.h) == len(hosts) and sum(len(m) for m in hosts.values()) == n - eng.num_free_slots()
        # ---- digests: a service's weight is its clusters' plus its buffered values (host 0's services hold nothing but buffered values);
        # the exported extremes cover both
        _, cnts, mm = eng.export_tdigest(0, n)
        weight = cnts.sum(axis=1, dtype=np.int64) + eng.export_tdigest_pending(0, n)[0]
        hdev, hslabs = eng.tdigest_rollup(capi.ROLLUP_HOST)
        slab_bytes = hslabs.dtype.itemsize
        for scope in scopes:
            slabs = hslabs if scope == capi.ROLLUP_HOST else eng.tdigest_rollup(scope)[1]
            mem = self.members(scope)
            assert len(slabs) == len(mem)
            for g, m in mem.items():
                live = m[weight[m] > 0]
                assert int(slabs[g]["cnt"].sum()) == int(weight[m].sum()), (what, scope, g)
                if len(live):
                    assert (int(slabs[g]["vmin"]), int(slabs[g]["vmax"])) == (int(mm[live, 0].min()), int(mm[live, 1].max())), (what, scope, g)
                if scope != capi.ROLLUP_HOST:  # the same bytes as the merge of the member hosts' slabs, picked here
                    hs = [h for h in sorted(hosts) if scope == capi.ROLLUP_GLOBAL or self.cluster[h] == g]
                    picked = hdev.view(len(hosts), slab_bytes)[hs].contiguous().view(-1)
                    assert eng.tdigest_merge_slabs(picked, len(hs))[1].tobytes() == slabs[g].tobytes(), (what, scope, g)
        rows, _, o = eng.rollup_filtered(group_by=capi.GROUP_HOST, any_state=True)
        assert [tuple(r) for r in rows] == [(g, len(m)) for g, m in hosts.items() if len(m)]
        for r, (g, _) in enumerate(rows):
            assert o["slabs"][r].tobytes() == hslabs[g].tobytes(), "%s: digest of host %d differs from the one of its members selected afresh" % (what, g)
        # ---- level histograms
        for lv in (1, 3):
            recs = eng.export_hist_level(lv, tusec, 0, n)
            for scope in scopes:
                got = eng.hist_rollup_level(scope, lv, tusec)
                for g, m in self.members(scope).items():
                    assert (got[g] == _np_sum(recs[m])).all(), "%s: level %d histogram of group %d (scope %d) is not the sum of its %d members" % (what, lv, g, scope, len(m))
        # ---- distinct counts: the open registers and a level's files
        for files, roll in ((eng.export_svc_hll(0, n), eng.hll_rollup), (eng.export_svc_hll_level(1, tusec, 0, n), lambda s: eng.hll_rollup_level(s, 1, tusec))):
            assert files.any()
            for scope in scopes:
                regs = roll(scope)[0]
                for g, m in self.members(scope).items():
                    want = files[m].max(axis=0) if len(m) else np.zeros(files.shape[1], dtype=np.uint8)
                    assert (regs[g] == want).all(), "%s: register file of group %d (scope %d) is not the union of its %d members'" % (what, g, scope, len(m))
        # ---- top-N by query rate of the window closed last: per host 10, all hosts 50; metric descending, ties by lower slot
        best = {h: sorted((self.qps[s] + (s,) for s in m.tolist() if s in self.qps), key=lambda e: (-e[0], e[2]))[:10] for h, m in hosts.items()}
        for h in (0, 1, 2, NH - 1):
            d = json.loads(eng.json_toplisteners(self.mids[h], 2))
            assert [e["svcid"] for e in d["topqps"]] == ["%016x" % e[1] for e in best[h]], "%s: top-N of host %d" % (what, h)
        d = json.loads(eng.json_toplisteners(None, 2))
        union = sorted((e for h in best for e in best[h]), key=lambda e: (-e[0], e[2]))[:50]
        assert [e["svcid"] for e in d["topqps"]] == ["%016x" % e[1] for e in union], "%s: top-N of all hosts" % what


def test_every_registry_change_reaches_every_fixed_scope():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    from gyeeta_amd.engine import SketchEngine
    eng = SketchEngine(max_hosts=NH + 2, max_services=2048, max_batch_events=1 << 16, enable_levels=True, svc_hll_p=6, svc_hll_levels=1)
    w = World(eng)
    # 1. register
    for h in range(NH):
        w.add_host(h, 0 if h < NH - 1 else 1)
    for h in range(NH):
        w.add_listeners(h, np.arange(NBIG if h == 0 else NSMALL))
    assert eng.num_services() == NBIG + (NH - 1) * NSMALL and w.svcs[1] == {0: NBIG, 1: NBIG + 1}
    w.feed(40)
    w.states_and_close()
    w.feed(10)  # (the open window has registers and buffered values of its own)
    w.check("registered")
    # 2. delete and reuse: slots 3 and 7 (host 0), 1025 and 1026 (host 1: all it has), 1027 (host 2) become free; host 2 takes 3 -- behind its
    # slot 1028 --, host 1 takes 7 and 1025, host 0 takes 1026 and 1027: the service count is what it was
    nsvc = eng.num_services()
    w.delete(0, [3, 7])
    w.delete(1, [0, 1])
    w.delete(2, [0])
    assert eng.num_free_slots() == 5
    w.check("deleted")
    assert w.add_listeners(2, [100]).tolist() == [3]
    assert w.add_listeners(1, [100, 101]).tolist() == [7, NBIG]
    assert w.add_listeners(0, [2000, 2001]).tolist() == [NBIG + 1, NBIG + 2]
    assert eng.num_services() == nsvc and eng.num_free_slots() == 0 and len(w.svcs[0]) == NBIG
    w.check("reused, before any data")
    w.feed(40)
    w.states_and_close()
    w.feed(10)
    w.check("reused")
    # 3. one host moves to the other cluster (a repeated registration that changes nothing in between)
    w.add_host(4, 0)
    w.add_host(5, 1)
    w.check("host moved")
    # 4. one new host without services
    w.add_host(NH, 0)
    w.check("empty host")
    eng.close()
