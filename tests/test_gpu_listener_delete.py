"""gys_delete_listeners / gys_register_listeners_slots / gys_num_free_slots / gys_list_stale_listeners on the GPU.

World: 3 hosts.  Hosts 0 and 1 carry 40 listeners each -- on host 0 that includes one (netns, port) key with two listeners bound to different
addresses and an any-address listener behind them -- and host 2 carries 5200 listeners (cut into parts, as in
tests/test_gpu_round3.py::test_many_listener_hosts_stay_on_the_host_local_path).

Reuse equals fresh: engine A registers X, ingests response events, connection, active-connection and state records, closes windows,
deletes half of X and registers Y into the freed slots (under OTHER hosts where the counts allow); engine B never has the deleted services
while anything is ingested or closed, so every byte the delete has to clear, and every byte it must not touch, shows up as a difference in
an export.  A third engine never deletes and takes Y at the tail: a reused slot equals a tail slot, whatever closed while it was free."""
import threading

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

NSMALL, NBIG = 40, 5200
KEY_PORT, KEY_S = 9000, 37  # host 0: services 37, 38 (bound to 10.1.1.1 / 10.1.1.2) and 39 (any address) share (netns of s = 37, port 9000)
ADDR = {37: bytes([10, 1, 1, 1]), 38: bytes([10, 1, 1, 2]), 39: None}
T0 = 1_700_000_000


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine(**kw):
    from gyeeta_amd.engine import SketchEngine
    return SketchEngine(**kw)


def _listeners(h, svc):
    """(glob ids, netns, ports, addrs) of services `svc` of host h"""
    svc = np.asarray(svc)
    g, ns, pt = wire.glob_id(np.full(len(svc), h), svc), wire.listener_netns(h, svc).copy(), wire.listener_port(svc).copy()
    addrs = [None] * len(svc)
    if h == 0:
        for i, s in enumerate(svc):
            if int(s) in ADDR:
                ns[i], pt[i], addrs[i] = wire.listener_netns(0, KEY_S), KEY_PORT, ADDR[int(s)]
    return g, ns, pt, addrs


def _events(rng, h, svc, per_svc, v6=False):
    """response events of host h for the services `svc` (per_svc each): the server address picks the listener on the shared key"""
    svc = np.repeat(np.asarray(svc), per_svc)
    rng.shuffle(svc)
    n = len(svc)
    ev = np.zeros(n, dtype=wire.RESP_EVENT6 if v6 else wire.RESP_EVENT)
    _, ns, pt, addrs = _listeners(h, svc)
    sa = np.full(n, 0x0A000000 | h, dtype=np.uint32)
    if h == 0:
        sa = np.where(svc == 37, 0x0A010101, np.where(svc == 38, 0x0A010102, sa)).astype(np.uint32)
    if v6:
        a = np.zeros((n, 16), dtype=np.uint8)
        a[:, 10:12] = 0xFF  # ::ffff:a.b.c.d (equals the IPv4 address, GY_IP_ADDR::operator==)
        a[:, 12:16] = sa.astype(">u4").view(np.uint8).reshape(n, 4)
        ev["saddr"] = a
        d = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        d[:, 0] = 0x20
        d[:, 1] = 0x01
        ev["daddr"] = d
    else:
        ev["saddr"] = sa.astype(">u4").view("<u4")
        ev["daddr"] = (0x0A000000 | rng.integers(1, 1 << 24, n)).astype(">u4").view("<u4")
    ev["netns"], ev["sport_be"] = ns, pt
    ev["dport_be"] = rng.integers(16000, 65536, n)
    lat = np.minimum(np.floor(rng.lognormal(3.0, 1.5, n)), 1e6).astype(np.uint32)
    lrcv = rng.integers(0, 1 << 31, n).astype(np.uint32)
    ev["lrcvtime"], ev["lsndtime"] = lrcv, lrcv + lat
    return ev, svc


def _states(rng, h, svc, delete=False):
    rec = wire.synth_listener_states(rng, h, svc)
    if delete:
        rec["query_flags"] = wire.LISTEN_FLAG_DELETE
    return rec


def _send_states(eng, mid, rec):
    for i in range(0, len(rec), 512):
        part = rec[i:i + 512]
        eng.partha_listener_state(mid, part.tobytes(), len(part))


def _exports(eng, tusec):
    """every per-service export of every slot + the fixed and filtered roll-ups, as a dict of arrays"""
    n = eng.num_services()
    out = {}
    for w in (0, 1):
        out["hist%d" % w] = eng.export_hist(w, 0, n)
    for lv in range(4):
        out["hist_level%d" % lv] = eng.export_hist_level(lv, tusec, 0, n)
        out["hll_level%d" % lv] = eng.export_svc_hll_level(lv, tusec, 0, n)
        out["hist_host_level%d" % lv] = eng.hist_rollup_level(capi.ROLLUP_HOST, lv, tusec)
    out["period"] = eng.export_hist_period(T0 - 100, T0 + 10_000, tusec, 0, n)[0]
    s, c, m = eng.export_tdigest(0, n)
    out["td_sum"], out["td_cnt"], out["td_minmax"] = s, c, m
    out["td_npend"], out["td_pend"] = eng.export_tdigest_pending(0, n)
    out["bitmap"] = eng.export_conn_bitmap(0, n)
    out["counters"] = eng.export_svc_counters(0, n)
    out["act_counters"] = eng.export_active_conn_counters(0, n)
    out["svc_hll"] = eng.export_svc_hll(0, n)
    out["day_stats"] = np.frombuffer(bytes(eng.export_day_stats(tusec, 0, n)), dtype=np.uint8)
    for w in (0, 1):
        out["svc_hist%d" % w] = eng.export_svc_hist(w, 0, n)
    out["td_host"] = eng.tdigest_rollup(capi.ROLLUP_HOST)[1]
    regs, est = eng.hll_rollup(capi.ROLLUP_HOST)
    out["hll_host"], out["hll_host_est"] = regs, est
    rows, nr, o = eng.rollup_filtered(group_by=capi.GROUP_HOST, any_state=True)
    out["rf_rows"], out["rf_slabs"], out["rf_regs"] = np.array(rows), o["slabs"], o["regs"]
    for lv in range(4):
        rows, nr, recs = eng.hist_rollup_filtered(group_by=capi.GROUP_HOST, level=lv, tusec=tusec, any_state=True)[:3]
        out["rfh_rows%d" % lv], out["rfh_recs%d" % lv] = np.array(rows), recs
    _, notify, scan = eng.scan_listener_state(tusec)
    out["scan_notify"], out["scan"] = notify.view(np.uint8), scan.view(np.uint8)
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "export %s differs between the reused and the fresh engine" % k


def _world(eng):
    mids = {h: wire.machine_id(h) for h in range(3)}
    for h in range(3):
        eng.register_host(mids[h], "cluster%d" % (h % 2))
    return mids


def _register_x(eng, mids):
    slots = {}
    for h, n in ((0, NSMALL), (1, NSMALL), (2, NBIG)):
        g, ns, pt, addrs = _listeners(h, np.arange(n))
        slots[h] = eng.register_listeners_slots(mids[h], g, ns, pt, addrs=addrs)
    return slots


DEAD = {0: [s for s in range(NSMALL) if s % 2 == 1], 1: list(range(10, 30)), 2: list(range(0, NBIG, 2))}  # (host 0: 37 and 39 of the shared key go, 38 stays)
Y_BASE = {0: 100, 1: 100, 2: 6000}  # service indices of the Y listeners (fresh keys and ids)
FIRST = {0: 0, 1: NSMALL, 2: 2 * NSMALL}  # slot of service s of host h in X = FIRST[h] + s
# Y is registered host 1 first: its 20 listeners take the 20 lowest free slots, which host 0's deleted listeners left, and host 0's take
# the ones host 1 left -- a reused slot changes hosts, so a member list kept from before the delete would be wrong in BOTH hosts
Y_ORDER = (1, 0, 2)
I64MIN = np.iinfo(np.int64).min


def _remap(gids, h, svc):
    """ids of services 0 .. len(svc) - 1 of host h (what the wire.synth_* helpers draw) -> the ids of the services `svc`; other ids stay"""
    k = len(svc)
    old, new = wire.glob_id(np.full(k, h), np.arange(k)), wire.glob_id(np.full(k, h), np.asarray(svc))
    order = np.argsort(old)
    pos = np.minimum(np.searchsorted(old[order], gids), k - 1)
    return np.where(old[order][pos] == gids, new[order][pos], gids)


def _feed(eng, mids, rng, h, svc, per, dropped=()):
    """one round of everything a partha sends for the services `svc` of host h: response events (IPv4 and IPv6), TCP connection records,
    active-connection rows and state records.  Every record is generated (the random stream is the same whoever runs), the ones of the
    services `dropped` are then left out."""
    svc = np.asarray(svc)
    dropped = np.asarray(dropped, dtype=np.int64)
    dead_ids = wire.glob_id(np.full(len(dropped), h), dropped) if len(dropped) else np.zeros(0, dtype=np.uint64)
    for v6 in (False, True):
        ev, esvc = _events(rng, h, svc, per if not v6 else max(per // 4, 2), v6)
        (eng.handle_resp_events_v6 if v6 else eng.handle_resp_events)(mids[h], ev[~np.isin(esvc, dropped)])
    for msg in range(1 if len(svc) < 1000 else 3):  # (<= 2048 records per message)
        rec = wire.synth_tcp_conns(rng, 2048, [h], len(svc), dup_frac=0.2, v6_frac=0.1)
        rec["ser_glob_id"] = _remap(rec["ser_glob_id"], h, svc)
        rec = rec[~np.isin(rec["ser_glob_id"], dead_ids)]
        eng.partha_tcp_conn_info(mids[h], wire.pack_variable(rec, None), len(rec))
        act = wire.synth_active_conns(rng, 2048, h, len(svc))
        act["listener_glob_id"] = _remap(act["listener_glob_id"], h, svc)
        act = act[~np.isin(act["listener_glob_id"], dead_ids)]
        eng.handle_partha_active_conns(mids[h], act.tobytes(), len(act))
    st = _states(rng, h, svc)
    _send_states(eng, mids[h], st[~np.isin(svc, dropped)])


def _np_sum(recs):
    """GY_HISTOGRAM::add_histogram over [n][16][2] int64 records"""
    out = np.zeros((16, 2), dtype=np.int64)
    out[15, 1] = I64MIN
    if len(recs):
        out = recs.sum(axis=0, dtype=np.int64)
        out[15, 1] = recs[:, 15, 1].max()
    return out


def _check_fixed_rollups(eng, tusec, members):
    """the fixed host roll-ups (they walk the hosts' cached member lists) against numpy over the per-service exports of `members`
    ({host slot: service slots}) and against the filtered roll-up, which selects its members from svc_host afresh"""
    n = eng.num_services()
    for lv in (1, 3):
        recs, got = eng.export_hist_level(lv, tusec, 0, n), eng.hist_rollup_level(capi.ROLLUP_HOST, lv, tusec)
        for g, m in members.items():
            assert (got[g] == _np_sum(recs[m])).all(), "level %d histogram of host %d is not the sum of its %d members" % (lv, g, len(m))
    files = eng.export_svc_hll(0, n)
    regs, est = eng.hll_rollup(capi.ROLLUP_HOST)
    for g, m in members.items():
        assert (regs[g] == files[m].max(axis=0)).all(), "register file of host %d is not the union of its members'" % g
    rows, _, o = eng.rollup_filtered(group_by=capi.GROUP_HOST, any_state=True)
    assert [tuple(r) for r in rows] == [(g, len(members[g])) for g in sorted(members)]
    slabs = eng.tdigest_rollup(capi.ROLLUP_HOST)[1]
    for r, (g, _) in enumerate(rows):
        assert o["slabs"][r].tobytes() == slabs[g].tobytes(), "digest of host %d differs from the one of its members selected afresh" % g
        assert (o["regs"][r] == regs[g]).all() and o["est"][r].tobytes() == est[g].tobytes()


_RUNS = {}


def _run_reuse(mode, gap):
    """mode "reuse": X gets data, half of X is deleted, `gap` windows close, Y takes the freed slots, Y's stream.
    mode "fresh": the services that get deleted never exist while anything is ingested or closed -- they are deleted right after the
        registration (a placeholder that only puts the survivors at their slots: the delete finds nothing to clear), receive nothing,
        and Y is registered into the still untouched slots at the same point of the stream.
    mode "tail": nothing is ever deleted; the same stream without the dead services' records, Y takes tail slots.
    Returns (exports, slots of Y per host, number of slots); computed once per (mode, gap)."""
    if (mode, gap) in _RUNS:
        return _RUNS[(mode, gap)]
    eng = _engine(max_hosts=4, max_services=8192, max_batch_events=1 << 20, enable_levels=True, svc_hll_p=6, svc_hll_levels=1)
    mids = _world(eng)
    _register_x(eng, mids)
    dead_ids = np.concatenate([wire.glob_id(np.full(len(DEAD[h]), h), np.array(DEAD[h])) for h in range(3)])
    live = {h: np.setdiff1d(np.arange(n), DEAD[h]) for h, n in ((0, NSMALL), (1, NSMALL), (2, NBIG))}
    ysvc = {h: Y_BASE[h] + np.arange(len(DEAD[h])) for h in range(3)}
    if mode == "fresh":
        assert eng.delete_listeners(dead_ids) == len(dead_ids)
    rng = np.random.default_rng(11)
    t = T0
    plan = ((0, NSMALL, 700), (1, NSMALL, 500), (2, NBIG, 12))
    for rnd in range(3):  # 31 s apart: the 300-s ring advances
        for h, n, per in plan:
            _feed(eng, mids, rng, h, np.arange(n), per, () if mode == "reuse" else DEAD[h])
        eng.window_close(t * 1_000_000)
        t += 31
    # a half-open window at the delete: buffered values, an open-window count and connection counters go with the service
    _feed(eng, mids, rng, 0, np.arange(NSMALL), 50, () if mode == "reuse" else DEAD[0])
    # the hosts' member lists are built here, before the delete ...  (every mode reads at the same points of the stream: a read folds the
    # buffered values into the digests)
    allx = {h: FIRST[h] + np.arange(n) for h, n, _ in plan}
    livex = {h: FIRST[h] + live[h] for h in range(3)}
    _check_fixed_rollups(eng, t * 1_000_000, livex if mode == "fresh" else allx)
    if mode == "reuse":
        assert eng.delete_listeners(dead_ids) == len(dead_ids)
        assert eng.num_free_slots() == len(dead_ids)
    # ... and must not be used after it: the service count they were built for has not changed
    _check_fixed_rollups(eng, t * 1_000_000, allx if mode == "tail" else livex)
    nsvc = eng.num_services()
    for rnd in range(gap):  # windows close while the slots are free (a cleanup cycle deletes, new listeners come later)
        for h, n, per in plan:
            _feed(eng, mids, rng, h, live[h], per // 2)
        eng.window_close(t * 1_000_000)
        t += 31
    yslots = {h: eng.register_listeners_slots(mids[h], *_listeners(h, ysvc[h])[:3]) for h in Y_ORDER}
    if mode == "tail":
        assert eng.num_services() == nsvc + len(dead_ids)
    else:
        assert eng.num_free_slots() == 0 and eng.num_services() == nsvc
    for rnd in range(2):
        for h, n, per in plan:
            _feed(eng, mids, rng, h, np.concatenate([live[h], ysvc[h]]), per)
        eng.window_close(t * 1_000_000)
        t += 31
    eng.sync()
    _check_fixed_rollups(eng, t * 1_000_000, {h: np.concatenate([(allx if mode == "tail" else livex)[h], yslots[h]]) for h in range(3)})
    out = _exports(eng, t * 1_000_000)
    n = eng.num_services()
    eng.close()
    _RUNS[(mode, gap)] = (out, yslots, n)
    return _RUNS[(mode, gap)]


@pytest.mark.parametrize("gap", [0, 2])
def test_reused_slots_equal_fresh_slots(torch_mod, gap):
    a, ya, na = _run_reuse("reuse", gap)
    b, yb, nb = _run_reuse("fresh", gap)
    assert na == nb
    for h in ya:
        assert (ya[h] == yb[h]).all()
    # the Y listeners sit in exactly the slots the deleted ones had, lowest first in the order of the registrations
    want = sorted(FIRST[h] + s for h in DEAD for s in DEAD[h])
    assert np.concatenate([ya[h] for h in Y_ORDER]).tolist() == want
    assert set(ya[1].tolist()) == {FIRST[0] + s for s in DEAD[0]}  # (host 1's new listeners in slots that were host 0's)
    assert a["counters"].any() and a["act_counters"].any()  # (connection and active-connection records reached the services)
    _assert_same(a, b)


def test_reused_slots_equal_tail_slots(torch_mod):
    """windows close between the delete and the reuse: a listener registered into a freed slot starts like one registered at the tail
    (its since-start period begins at ITS first close, not at a close that went by while the slot was free)"""
    a, ya, na = _run_reuse("reuse", 2)
    c, yc, nc = _run_reuse("tail", 2)
    ndead = sum(len(DEAD[h]) for h in DEAD)
    assert nc == na + ndead and np.concatenate([yc[h] for h in Y_ORDER]).tolist() == list(range(na, nc))
    keep = np.concatenate([FIRST[h] + np.setdiff1d(np.arange(n), DEAD[h]) for h, n in ((0, NSMALL), (1, NSMALL), (2, NBIG))])
    rows_a = np.concatenate([keep] + [ya[h] for h in Y_ORDER])
    rows_c = np.concatenate([keep] + [yc[h] for h in Y_ORDER])
    per_slot = 0
    for k in a:
        if k.startswith(("scan", "rf", "td_host", "hll_host", "hist_host")):
            continue  # (roll-ups have the never-deleted services as members; scan records carry ids by slot)
        x, y = np.asarray(a[k]), np.asarray(c[k])
        if k == "day_stats":
            x, y = x.reshape(na, -1), y.reshape(nc, -1)
        assert x.shape[0] == na and y.shape[0] == nc, k
        assert x[rows_a].tobytes() == y[rows_c].tobytes(), "export %s: a reused slot differs from a tail slot" % k
        per_slot += 1
    assert per_slot >= 20
    assert a["period"][ya[0]].any()  # (the since-start period has something to say about the new listeners)


def test_deleted_means_gone(torch_mod):
    eng = _engine(max_hosts=4, max_services=8192, max_batch_events=1 << 20, svc_hll_p=6)
    mids = _world(eng)
    _register_x(eng, mids)
    rng = np.random.default_rng(5)
    gid = lambda h, s: int(wire.glob_id(h, s))
    for h, n in ((0, NSMALL), (1, NSMALL)):
        eng.handle_resp_events(mids[h], _events(rng, h, np.arange(n), 20)[0])
        _send_states(eng, mids[h], _states(rng, h, np.arange(n)))
    eng.window_close(T0 * 1_000_000)
    rows0 = dict(eng.rollup_filtered(group_by=capi.GROUP_HOST, any_state=True, want=("est",))[0])
    assert rows0 == {0: NSMALL, 1: NSMALL, 2: NBIG}
    # an unknown id and a repeat are not counted
    assert eng.delete_listeners([gid(1, 3), gid(1, 3), 0x1234, gid(0, 39)]) == 2
    assert eng.num_free_slots() == 2
    for h, s in ((1, 3), (0, 39)):
        with pytest.raises(capi.GysError) as e:
            eng.lookup(gid(h, s))
        assert e.value.code == capi.ERR_NOTFOUND
    c0 = eng.counters()
    cnt = lambda s: int(eng.export_hist(1, 0, eng.num_services())[s][15][0])
    s37, s38 = eng.lookup(gid(0, 37)), eng.lookup(gid(0, 38))
    before = (cnt(s37), cnt(s38))
    # host 1, service 3: its port has no listener any more
    eng.handle_resp_events(mids[1], _events(rng, 1, [3], 77)[0])
    # host 0: the any-address listener of the shared key is gone -- an address nobody is bound to reaches nobody; the bound ones still get theirs
    ev, _ = _events(rng, 0, [39], 55)
    eng.handle_resp_events(mids[0], ev)
    eng.handle_resp_events(mids[0], _events(rng, 0, [37, 38], 10)[0])
    eng.sync()
    c1 = eng.counters()
    assert c1["resp_dropped_nolistener"] - c0["resp_dropped_nolistener"] == 77 + 55
    assert (cnt(s37), cnt(s38)) == (before[0] + 10, before[1] + 10)
    # one bound listener deleted: the other's counts are untouched, the deleted one's address drops
    assert eng.delete_listeners([gid(0, 37)]) == 1
    eng.handle_resp_events(mids[0], _events(rng, 0, [37], 31)[0])
    eng.sync()
    c2 = eng.counters()
    assert c2["resp_dropped_nolistener"] - c1["resp_dropped_nolistener"] == 31 and cnt(s38) == before[1] + 10
    eng.handle_resp_events(mids[0], _events(rng, 0, [38], 9)[0])
    eng.sync()
    assert cnt(s38) == before[1] + 19 and eng.counters()["resp_dropped_nolistener"] == c2["resp_dropped_nolistener"]
    # state records for a deleted id are missed
    _send_states(eng, mids[1], _states(rng, 1, [3, 4]))
    eng.sync()
    c3 = eng.counters()
    assert c3["lstate_missed"] - c2["lstate_missed"] == 1
    # the hosts' roll-ups lose the members; ANY_STATE selections have nobody from a free slot
    rows = dict(eng.rollup_filtered(group_by=capi.GROUP_HOST, any_state=True, want=("est",))[0])
    assert rows == {0: NSMALL - 2, 1: NSMALL - 1, 2: NBIG}
    rows = dict(eng.rollup_filtered(group_by=capi.GROUP_CLUSTER, any_state=True, want=("est",))[0])
    assert rows == {0: NSMALL - 2 + NBIG, 1: NSMALL - 1}
    eng.close()


def test_register_delete_cycles_keep_the_tables_clean(torch_mod, oracle):
    eng = _engine(max_hosts=2, max_services=64, max_batch_events=1 << 16)
    mid = wire.machine_id(0)
    hslot = eng.register_host(mid, "c")
    rng = np.random.default_rng(3)
    ids = None
    for rnd in range(2000):
        svc = 1000 + 32 * rnd + np.arange(32)
        g, ns, pt = wire.glob_id(np.zeros(32, dtype=np.int64), svc), wire.listener_netns(0, svc), wire.listener_port(svc)
        slots = eng.register_listeners_slots(mid, g, ns, pt)  # (GYS_ERR_NOMEM would raise)
        assert eng.num_services() <= 64 and eng.num_free_slots() == eng.num_services() - 32
        assert sorted(slots.tolist()) == list(range(32)) or rnd == 0
        if rnd == 1999:
            ids = (svc, g, ns, pt, slots)
            break
        assert eng.delete_listeners(g) == 32
        assert eng.num_free_slots() == eng.num_services()
    svc, g, ns, pt, slots = ids
    orc = oracle.OracleEngine(64)
    order = np.argsort(slots)
    for i in order:
        orc.register(hslot, int(g[i]), int(ns[i]), int(pt[i]))
    assert [int(slots[i]) for i in order] == list(range(32))
    for k in range(3):
        ev = helpers.make_resp_events(rng, 0, 20000, 32, unknown_frac=0.0)
        sidx = rng.integers(0, 32, len(ev))
        ev["netns"], ev["sport_be"] = ns[sidx], pt[sidx]
        eng.handle_resp_events(mid, ev)
        orc.resp_batch(ev.tobytes(), [hslot], [0])
    eng.sync()
    helpers.assert_hist_equal(eng.export_hist(0, 0, 32), orc.hist(), 32)
    gs, gc, gm = eng.export_tdigest(0, 32)
    os_, oc, om = orc.td_arrays()
    assert (gc == oc[:32]).all() and (gs == os_[:32]).all() and (gm == om[:32]).all()
    c, oc_ = eng.counters(), orc.counters()
    assert c["resp_events"] == oc_["events"] and c["resp_dropped_nolistener"] == oc_["dropped_nolistener"] == 0
    for i in range(32):
        assert eng.lookup(int(g[i])) == int(slots[i])
    eng.close()


def test_stale_list(torch_mod):
    eng = _engine(max_hosts=4, max_services=8192, max_batch_events=1 << 16)
    mids = _world(eng)
    _register_x(eng, mids)
    rng = np.random.default_rng(9)
    gid = lambda h, s: int(wire.glob_id(h, s))
    t = T0
    # window 1: services 0..19 of host 1 and 0..2999 of host 2 report; 5..9 of host 1 never again; host 0 never reports at all
    _send_states(eng, mids[1], _states(rng, 1, np.arange(20)))
    _send_states(eng, mids[2], _states(rng, 2, np.arange(3000)))
    K = 4
    for w in range(K):
        eng.window_close(t * 1_000_000)
        t += 5
        keep1 = np.setdiff1d(np.arange(20), np.arange(5, 10))
        _send_states(eng, mids[1], _states(rng, 1, keep1))
        _send_states(eng, mids[2], _states(rng, 2, np.arange(0, 3000, 3)))  # every third service of host 2 stays live
    # delete records: services 12, 13 of host 1 (reported before) and 30 of host 1 (never reported: cannot be listed)
    _send_states(eng, mids[1], _states(rng, 1, [12, 13, 30], delete=True))
    eng.sync()
    ids, nf = eng.list_stale_listeners(eng.STALE_DELETED, 0)
    assert nf == 2 and ids.tolist() == [gid(1, 12), gid(1, 13)]
    silent2 = [s for s in range(3000) if s % 3]
    want_aged = [gid(1, s) for s in range(5, 10)] + [gid(2, s) for s in silent2]  # slot order: host 1 before host 2
    ids, nf = eng.list_stale_listeners(eng.STALE_AGED, K - 1)
    assert nf == len(want_aged) and ids.tolist() == want_aged
    ids, nf = eng.list_stale_listeners(eng.STALE_AGED, K)  # kept in window 1, K windows closed since: not OLDER than K
    assert nf == 0 and len(ids) == 0
    ids, nf = eng.list_stale_listeners(eng.STALE_AGED, 0)  # everybody who did not report in the open window ... which is nobody live
    assert nf == len(want_aged)
    both = [gid(1, s) for s in (5, 6, 7, 8, 9, 12, 13)] + [gid(2, s) for s in silent2]
    ids, nf = eng.list_stale_listeners(eng.STALE_AGED | eng.STALE_DELETED, K - 1, cap=100)
    assert nf == len(both) and ids.tolist() == both[:100]
    ids, nf = eng.list_stale_listeners(3, K - 1)
    assert eng.delete_listeners(ids) == len(both) and eng.num_free_slots() == len(both)
    ids, nf = eng.list_stale_listeners(3, K - 1)
    assert nf == 0 and len(ids) == 0
    eng.close()


def test_the_old_call_takes_tail_slots_only(torch_mod):
    eng = _engine(max_hosts=2, max_services=64, max_batch_events=1 << 16)
    mid = wire.machine_id(0)
    eng.register_host(mid, "c")
    reg = lambda call, svc: call(mid, wire.glob_id(np.zeros(len(svc), dtype=np.int64), svc), wire.listener_netns(0, svc), wire.listener_port(svc))
    assert reg(eng.register_listeners, np.arange(40)) == 0
    assert eng.delete_listeners(wire.glob_id(np.zeros(10, dtype=np.int64), np.arange(10, 20))) == 10
    assert reg(eng.register_listeners, np.arange(100, 120)) == 40  # consecutive tail slots, the ten free ones stay free
    assert eng.num_services() == 60 and eng.num_free_slots() == 10
    with pytest.raises(capi.GysError) as e:
        reg(eng.register_listeners, np.arange(200, 205))  # 4 tail slots left
    assert e.value.code == capi.ERR_NOMEM and eng.num_services() == 60
    s = reg(eng.register_listeners_slots, np.arange(200, 212))  # 10 free + 2 tail
    assert s.tolist() == list(range(10, 20)) + [60, 61] and eng.num_free_slots() == 0 and eng.num_services() == 62
    with pytest.raises(capi.GysError) as e:
        reg(eng.register_listeners_slots, np.arange(300, 303))  # 2 left: nothing is registered
    assert e.value.code == capi.ERR_NOMEM and eng.num_services() == 62
    s = reg(eng.register_listeners_slots, np.array([300, 205, 300, 301]))  # known and repeated ids report their slot
    assert s.tolist() == [62, 15, 62, 63]
    eng.close()


def test_both_registration_calls_build_the_same_registry(torch_mod, oracle):
    """No deletion ever: one engine registers the world through register_listeners, one through register_listeners_slots -- hosts of 40 and
    40 listeners (host 0 with the shared bound-address key) and one of 2 049, the smallest that is cut into parts.  The slot numbers are
    equal, and after an IPv4 and an IPv6 response batch per host both engines equal the oracle and, behind a window close, each other in
    every export."""
    ncut = 2049
    world = ((0, NSMALL, 30), (1, NSMALL, 30), (2, ncut, 1))
    rng = np.random.default_rng(17)
    batches = [(h, v6, _events(rng, h, np.arange(n), max(per // (4 if v6 else 1), 1), v6)[0]) for h, n, per in world for v6 in (False, True)]
    orc = oracle.OracleEngine(2 * NSMALL + ncut)
    outs, slots = {}, {}
    for call in ("tail", "slots"):
        eng = _engine(max_hosts=4, max_services=8192, max_batch_events=1 << 20, enable_levels=True, svc_hll_p=6, svc_hll_levels=1)
        mids = {h: wire.machine_id(h) for h in range(3)}
        hslot = {h: eng.register_host(mids[h], "cluster%d" % (h % 2)) for h in range(3)}
        slots[call] = []
        for h, n, _ in world:
            g, ns, pt, addrs = _listeners(h, np.arange(n))
            if call == "tail":
                slots[call].append(eng.register_listeners(mids[h], g, ns, pt, addrs=addrs) + np.arange(n))
                for i in range(n):
                    assert orc.register_addr(hslot[h], int(g[i]), int(ns[i]), int(pt[i]), addrs[i]) == slots[call][-1][i]
            else:
                slots[call].append(eng.register_listeners_slots(mids[h], g, ns, pt, addrs=addrs))
        for h, v6, ev in batches:
            (eng.handle_resp_events_v6 if v6 else eng.handle_resp_events)(mids[h], ev)
            if call == "tail":
                (orc.resp_batch_v6 if v6 else orc.resp_batch)(ev.tobytes(), [hslot[h]], [0])
        eng.sync()
        n = eng.num_services()
        assert n == orc.nsvc == 2 * NSMALL + ncut
        helpers.assert_hist_equal(eng.export_hist(0, 0, n), orc.hist(), n)
        gs, gc, gm = eng.export_tdigest(0, n)
        os_, oc, om = orc.td_arrays()
        assert (gc == oc).all() and (gs == os_).all() and (gm == om).all()
        c, oc_ = eng.counters(), orc.counters()
        assert c["resp_events"] == oc_["events"] == sum(len(ev) for _, _, ev in batches) and c["resp_dropped_nolistener"] == oc_["dropped_nolistener"] == 0
        eng.window_close(T0 * 1_000_000)
        outs[call] = _exports(eng, (T0 + 31) * 1_000_000)
        eng.close()
    assert np.concatenate(slots["tail"]).tolist() == np.concatenate(slots["slots"]).tolist() == list(range(2 * NSMALL + ncut))
    assert outs["tail"]["hist1"][:, 15, 0].sum() == sum(len(ev) for _, _, ev in batches)  # (every event reached a service)
    _assert_same(outs["tail"], outs["slots"])


def test_mid_window_delete(torch_mod):
    """A: everything ingested (one batch from two threads through the submission queue), then host 1's services 0..9 deleted mid-window.
    B: never got their events.  C: got everything, deleted nothing."""
    rng = np.random.default_rng(21)
    ev0, _ = _events(rng, 0, np.arange(NSMALL), 300)
    ev1, svc1 = _events(rng, 1, np.arange(NSMALL), 300)
    dead = np.arange(10)
    outs = {}
    for name in "ABC":
        eng = _engine(max_hosts=4, max_services=8192, max_batch_events=1 << 20)
        mids = _world(eng)
        _register_x(eng, mids)
        e1 = ev1[~np.isin(svc1, dead)] if name == "B" else ev1
        if name == "A":
            th = [threading.Thread(target=eng.handle_resp_events, args=(mids[h], e)) for h, e in ((0, ev0), (1, e1))]
            [x.start() for x in th]
            [x.join() for x in th]
            assert eng.delete_listeners(wire.glob_id(np.ones(10, dtype=np.int64), dead)) == 10  # drains the queues first
        else:
            eng.handle_resp_events(mids[0], ev0)
            eng.handle_resp_events(mids[1], e1)
        eng.window_close(T0 * 1_000_000)
        n = eng.num_services()
        gh = eng.export_global_hist()
        outs[name] = dict(cms=eng.export_cms(0), hist=eng.export_hist(1, 0, n), hll=eng.export_hll(), td=eng.export_tdigest(0, n)[1],
                          ghist=[gh.stats[i].count for i in range(15)] + [gh.total_count, gh.max_val_seen])
        eng.close()
    a, b, c = outs["A"], outs["B"], outs["C"]
    assert (a["cms"] == b["cms"]).all() and (a["hist"] == b["hist"]).all() and (a["td"] == b["td"]).all()
    assert not (a["cms"] == c["cms"]).all()
    assert (a["hll"] == c["hll"]).all() and a["ghist"] == c["ghist"]
    assert a["ghist"] != b["ghist"]
