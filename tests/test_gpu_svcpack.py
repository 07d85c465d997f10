"""Service records on the GPU: gys_pack_services* / gys_unpack_services* / gys_list_service_ids ("service records" in include/gysketch.h).

World: 3 hosts x 8 services, t-digest on with td_pend_cap 64 and td_buf_values 193 (an odd buffer stride: the services' buffers sit at all
four residues from a 16-byte boundary), svc_hll_p 4 with svc_hll_levels, enable_levels 1.  A window's stream is a function of the window
number alone (its own seeded generator), so every engine that takes window w takes the same bytes: a few thousand response events (service
0 of host 0 only ever buffers, service 1 merges every window, service 2 gets 5 000 values in one call in window 2, service 3 only IPv6
events, service 4 nothing), listener-state, connection and active-connection records, one gys_scan_listener_state_dev +
gys_decide_listener_state_dev per window.  Service 7 of host 1 is registered after window 1 into the slot a deleted listener left.

Everything is compared per glob_id: the destination registers hosts and listeners in another order, so slots and host slots differ."""
import numpy as np
import pytest

from gyeeta_amd import capi, wire

pytestmark = pytest.mark.gpu

H, S = 3, 8
T0 = 1_700_000_000  # T0 % 30 == 20: the 300-s level's ring (30-s buckets) turns at T0 + 10, T0 + 40, ...
assert T0 % 30 == 20
CLOSES = [T0, T0 + 5, T0 + 10, T0 + 15, T0 + 20, T0 + 40, T0 + 45]  # windows 0 .. 3 before the pack (one ring boundary), 4 .. 6 after (another)
NPRE = 4
DOOMED = 99  # host 1's listener that is deleted after window 1; service 7 of host 1 takes its slot
CFG = dict(max_hosts=4, max_services=64, max_batch_events=1 << 16, enable_levels=True, svc_hll_p=4, svc_hll_levels=1, td_pend_cap=64, td_buf_values=193)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine(**kw):
    from gyeeta_amd.engine import SketchEngine
    return SketchEngine(**dict(CFG, **kw))


def _gid(h, s):
    return int(wire.glob_id(h, s))


def _reg(eng, h, svc):
    svc = np.asarray(svc)
    return eng.register_listeners_slots(wire.machine_id(h), wire.glob_id(np.full(len(svc), h), svc), wire.listener_netns(h, svc), wire.listener_port(svc))


def _events(rng, h, svc_counts, v6=False, slow=()):
    """response events of host h: svc_counts = {service: events}; the services `slow` answer e^3 times slower than they use to"""
    svc = np.concatenate([np.full(c, s) for s, c in svc_counts.items()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    rng.shuffle(svc)
    n = len(svc)
    ev = np.zeros(n, dtype=wire.RESP_EVENT6 if v6 else wire.RESP_EVENT)
    sa = np.full(n, 0x0A000000 | h, dtype=np.uint32)
    if v6:
        a = np.zeros((n, 16), dtype=np.uint8)
        a[:, 10:12] = 0xFF
        a[:, 12:16] = sa.astype(">u4").view(np.uint8).reshape(n, 4)
        ev["saddr"] = a
        d = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        d[:, 0], d[:, 1] = 0x20, 0x01
        ev["daddr"] = d
    else:
        ev["saddr"] = sa.astype(">u4").view("<u4")
        ev["daddr"] = (0x0A000000 | rng.integers(1, 1 << 24, n)).astype(">u4").view("<u4")
    ev["netns"], ev["sport_be"] = wire.listener_netns(h, svc), wire.listener_port(svc)
    ev["dport_be"] = rng.integers(16000, 65536, n)
    lat = np.minimum(np.floor(rng.lognormal(3.0 + 0.2 * (svc % 5) + 3.0 * np.isin(svc, list(slow)), 1.5, n)), 1e6).astype(np.uint32)
    lrcv = rng.integers(0, 1 << 31, n).astype(np.uint32)
    ev["lrcvtime"], ev["lsndtime"] = lrcv, lrcv + lat
    return ev


def _counts(h, w):
    if h == 0:
        return {0: 5, 1: 300, 2: 5000 if w == 2 else 20, 5: 100, 6: 70, 7: 130}, {3: 40}
    return {s: 40 + 15 * ((s + h + w) % 7) for s in range(S)}, {s: 10 for s in range(0, S, 3)}


def _present(h, w, s):
    """is service s of host h registered while window w is open"""
    return not (h == 1 and s == 7 and w < 2)


def _feed(eng, w, hosts, part=None, known_only=False):
    """window w's stream of `hosts` (the same bytes for every engine); part 0 / 1: only the first / second half of the response events;
    known_only: without the connection records that name no registered service (the connecting halves with an unresolved ser_glob_id_):
    those go straight into the RANK's Count-Min rows at ingest, which are no per-service state and stay with the source"""
    for h in hosts:
        rng = np.random.default_rng(7000 + 10 * w + h)
        mid = wire.machine_id(h)
        v4, v6 = _counts(h, w)
        for cnts, is6 in ((v4, False), (v6, True)):
            ev = _events(rng, h, {s: c for s, c in cnts.items() if _present(h, w, s)}, is6, slow=(5, 6) if w in (2, 5) else ())  # (slow windows: the decision's high-response history, seen by the next window's scan)
            half = len(ev) // 2
            ev = ev if part is None else (ev[:half] if part == 0 else ev[half:])
            (eng.handle_resp_events_v6 if is6 else eng.handle_resp_events)(mid, ev)
        if part == 1:
            continue
        rec = wire.synth_tcp_conns(rng, 256, [h], S, dup_frac=0.2, v6_frac=0.1)
        if known_only:
            rec = rec[np.isin(rec["ser_glob_id"], wire.glob_id(np.full(S, h), np.arange(S)))]
        eng.partha_tcp_conn_info(mid, wire.pack_variable(rec, None), len(rec))
        act = wire.synth_active_conns(rng, 128, h, S)
        eng.handle_partha_active_conns(mid, act.tobytes(), len(act))
        svc = [s for s in range(S) if _present(h, w, s) and not (h == 0 and s == 4)]  # (service 4 of host 0 never reports anything)
        st = wire.synth_listener_states(rng, h, svc)
        eng.partha_listener_state(mid, st.tobytes(), len(st))


GID2HS = {int(wire.glob_id(h, s)): (h, s) for h in (0, 1, 2, 5) for s in range(S)}


def _decide(eng, w):
    """the 5-s scan and the state decision of window w: (scan records, notify records, decisions).  The task inputs are a function of
    (host, service, window): every fourth service has more server errors than queries (a severe state: the issue history)."""
    t = CLOSES[w] - 1  # (a second before the close: the 5-s level still holds the window closed last where the closes are 5 s apart)
    notify_dev, notify, scan = eng.scan_listener_state(t * 1_000_000)
    issue = np.zeros(len(scan), dtype=eng.ISSUE_IN_DT)
    for i, g in enumerate(scan["glob_id"]):
        h, s = GID2HS.get(int(g), (0, 1))
        if int(g) in GID2HS and (h + s + w) % 4 == 0:
            issue["ser_errors"][i] = 1 << 20
    dec = eng.decide_listener_state(scan, issue_in=issue, notify_dev=notify_dev)
    return scan, np.frombuffer(notify_dev.cpu().numpy().tobytes(), dtype=np.uint8).reshape(-1, 88)[:len(scan)], dec


def _window(eng, w, hosts, decisions=None):
    _feed(eng, w, hosts)
    d = _decide(eng, w)
    if decisions is not None:
        decisions.append(d)
    eng.window_close(CLOSES[w] * 1_000_000)


def _world(eng, hosts=(0, 1, 2), order=None):
    for h in hosts:
        eng.register_host(wire.machine_id(h), "cluster%d" % (h % 2))
    for h in hosts:
        svc = list(range(S)) if h != 1 else list(range(S - 1)) + [DOOMED]
        _reg(eng, h, svc if order is None else order(svc))


def _source(hosts=(0, 1, 2), nwin=NPRE):
    """engine A after `nwin` windows: the doomed listener of host 1 is deleted after window 1 and service 7 takes its slot"""
    eng = _engine()
    _world(eng, hosts)
    for w in range(nwin):
        _window(eng, w, hosts)
        if w == 1 and 1 in hosts:
            slot = eng.lookup(_gid(1, DOOMED))
            assert eng.delete_listeners([_gid(1, DOOMED)]) == 1
            assert _reg(eng, 1, [7]).tolist() == [slot]  # (a reused slot)
    return eng


def _dest(**kw):
    """engine B: fresh, hosts and listeners registered in another order (no listener was ever deleted here), more room"""
    eng = _engine(**dict(dict(max_hosts=6, max_services=40), **kw))
    for h in (2, 0, 1):
        eng.register_host(wire.machine_id(h), "cluster%d" % (h % 2))
    for h in (1, 2, 0):
        _reg(eng, h, list(range(S))[::-1])
    return eng


ALL = [(h, s) for h in range(H) for s in range(S)]


def _exports(eng, t, who=ALL, decide=False):
    """every per-service export, one row per (host, service) of `who` in that order -- per glob_id, whatever the slots are"""
    tusec = t * 1_000_000
    n = eng.num_services()
    slot = np.array([eng.lookup(_gid(h, s)) for h, s in who])
    out = {}
    for wh in (0, 1):
        out["hist%d" % wh] = eng.export_hist(wh, 0, n)
        out["svc_hist%d" % wh] = eng.export_svc_hist(wh, 0, n)
    out["bitmap"] = eng.export_conn_bitmap(0, n)
    out["td_sum"], out["td_cnt"], out["td_minmax"] = eng.export_tdigest(0, n)
    out["td_npend"], out["td_pend"] = eng.export_tdigest_pending(0, n)
    out["counters"] = eng.export_svc_counters(0, n)
    out["act_counters"] = eng.export_active_conn_counters(0, n)
    out["svc_hll"] = eng.export_svc_hll(0, n)
    for lv in range(4):
        out["hll_level%d" % lv] = eng.export_svc_hll_level(lv, tusec, 0, n)
        out["hist_level%d" % lv] = eng.export_hist_level(lv, tusec, 0, n)
    out["period_a"] = eng.export_hist_period(T0 - 100, T0 + 10_000, tusec, 0, n)[0]
    out["period_b"] = eng.export_hist_period(T0 + 8, T0 + 31, tusec, 0, n)[0]
    out["day_stats"] = np.frombuffer(bytes(eng.export_day_stats(tusec, 0, n)), dtype=np.uint8).reshape(n, -1)
    out["quantiles"] = eng.scan_quantiles([0.25, 0.5, 0.95, 0.99]).view(np.uint64)
    below, total = eng.scan_ranks([1, 10, 100, 1000])
    out["ranks_below"], out["ranks_total"] = below.view(np.uint64), total
    _, notify, scan = eng.scan_listener_state(tusec)
    out["scan"] = np.frombuffer(scan.tobytes(), dtype=np.uint8).reshape(n, -1)
    out["scan_notify"] = np.frombuffer(notify.tobytes(), dtype=np.uint8).reshape(n, -1)
    out = {k: np.asarray(v)[slot] for k, v in out.items()}
    # the kept state of all services: rows by glob id; the row's host slot is the host's slot HERE
    _, hosts, recs, nm = eng.svcstate_scan(maxrecs=1000)
    by_id = {int(r["glob_id"]): (int(hs), r.tobytes()) for hs, r in zip(hosts, recs)}
    rows = []
    for h, s in who:
        hs, raw = by_id.get(_gid(h, s), (None, b""))
        if hs is not None:
            assert hs == eng.register_host(wire.machine_id(h), "cluster%d" % (h % 2)), "kept state of (%d, %d) names host slot %d" % (h, s, hs)
        rows.append(raw)
    out["svcstate"] = np.array(rows, dtype=object)
    return out


def _assert_same(a, b, what, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        if a[k].dtype == object:
            assert list(a[k]) == list(b[k]), "%s: %s differs" % (what, k)
            continue
        assert a[k].shape == b[k].shape, (what, k)
        bad = [i for i in range(len(a[k])) if a[k][i].tobytes() != b[k][i].tobytes()]
        assert not bad, "%s: export %s differs for rows %s" % (what, k, bad[:8])


def _assert_decisions_same(da, db, ea, eb, what):
    """scan / notify / decision records of two engines' _decide, per glob_id"""
    for (sa, na, ca), (sb, nb, cb) in zip(da, db):
        ia = {int(g): i for i, g in enumerate(sa["glob_id"]) if g}
        ib = {int(g): i for i, g in enumerate(sb["glob_id"]) if g}
        assert ia.keys() == ib.keys() and len(ia) == H * S, what
        for g in ia:
            i, j = ia[g], ib[g]
            assert sa[i].tobytes() == sb[j].tobytes() and na[i].tobytes() == nb[j].tobytes() and ca[i].tobytes() == cb[j].tobytes(), "%s: decision of %x" % (what, g)


def _pack_source():
    """an engine A after four windows, its blob of every service (host bytes) and A's exports right after the pack, which changed nothing"""
    a = _source()
    ids = a.list_service_ids()
    assert sorted(ids.tolist()) == sorted(_gid(h, s) for h, s in ALL) and a.num_free_slots() == 0
    before = _exports(a, CLOSES[NPRE])
    blob = a.pack_services(ids)
    assert blob.nbytes == a.service_blob_bytes(len(ids))
    _assert_same(before, _exports(a, CLOSES[NPRE]), "the pack modified its source")
    return dict(a=a, blob=blob, exports=before)


@pytest.fixture(scope="module")
def packed(torch_mod):
    """A as _pack_source leaves it, shared by the tests that only read it: no test feeds it or closes a window on it"""
    p = _pack_source()
    yield p
    p["a"].close()


def test_restore_continues_bit_for_bit(torch_mod):
    p = _pack_source()  # (its own A: this test takes it through three more windows)
    a, b = p["a"], _dest()
    assert b.unpack_services(p["blob"]) == (H * S, 0)
    _assert_same(p["exports"], _exports(b, CLOSES[NPRE]), "right after the unpack")
    assert p["exports"]["hist1"][:, 15, 0].sum() > 10000 and p["exports"]["td_npend"].any() and p["exports"]["td_cnt"].any()
    # (service 0 of host 0 only buffers, 2 merged its 5 000 values, 3 has IPv6 rows only, 4 nothing)
    row = {hs: i for i, hs in enumerate(ALL)}
    e = p["exports"]
    assert e["td_cnt"][row[(0, 0)]].sum() == 0 and e["td_npend"][row[(0, 0)]] == 5 * NPRE
    assert e["td_cnt"][row[(0, 2)]].sum() >= 5000 and e["hist1"][row[(0, 4)], 15, 0] == 0
    assert e["counters"].any() and e["act_counters"].any() and e["hll_level2"].any() and e["hist_level1"][:, 15, 0].any()
    da, db = [], []
    for w in range(NPRE, len(CLOSES)):
        for eng, d in ((a, da), (b, db)):
            if w == 5:  # a query in the middle of the open window
                _feed(eng, w, range(H), part=0)
                mid = _exports(eng, CLOSES[w] - 2)
                _feed(eng, w, range(H), part=1)
                d.append(mid)
            else:
                _feed(eng, w, range(H))
            d.append(_decide(eng, w))
            eng.window_close(CLOSES[w] * 1_000_000)
        if w == 5:
            _assert_same(da.pop(-2), db.pop(-2), "in the middle of window %d" % w)
        _assert_same(_exports(a, CLOSES[w] + 1), _exports(b, CLOSES[w] + 1), "after window %d" % w)
    _assert_decisions_same(da, db, a, b, "restore")
    # the history bytes carry something over the restore: window 4's decisions hold bits that windows before the pack shifted in
    first = da[0][2]
    assert (first["issue_bit_hist"] & 0xFE).any() and (first["high_resp_bit_hist"] & 0xFE).any()
    a.close()
    b.close()


def _rank_level(eng):
    """what the close builds from the services' window accumulators: the Count-Min rows of the window closed last"""
    return {"cms0": eng.export_cms(0), "cms1": eng.export_cms(1)}


def test_restore_of_an_open_window(torch_mod):
    """The pack falls into the MIDDLE of window 4: buffered values of the open window, its histogram records and bitmap rows, the connection
    path's window accumulators and the window's response event counts travel.  Both engines then close with nothing further ingested: the
    per-service exports are equal, and so are the window's Count-Min rows, which the close folds from the carried accumulators (in a
    restored engine nothing was ingested, so only the unpack can have told the close that there is something to fold)."""
    a = _source()
    _feed(a, NPRE, range(H), known_only=True)
    dec_a = _decide(a, NPRE)
    # No export in front of the pack: gys_export_svc_counters folds the connection path's window accumulators into the counters AND into
    # the rank's Count-Min rows (k_conn_fold), after which that share is a rank-level register and stays with the source.  Here the
    # accumulators are still per-service state when they are packed; both engines read (and fold) them after the unpack.
    blob = a.pack_services(dev=True)
    b = _dest()
    assert b.unpack_services(blob) == (H * S, 0)
    before = _exports(a, CLOSES[NPRE] - 1)
    _assert_same(before, _exports(b, CLOSES[NPRE] - 1), "open window, right after the unpack")
    assert before["counters"].any()
    assert before["hist0"][:, 15, 0].sum() > 1000 and before["bitmap"].any()  # (the open window holds something)
    for eng in (a, b):
        eng.window_close(CLOSES[NPRE] * 1_000_000)
    _assert_same(_exports(a, CLOSES[NPRE] + 1), _exports(b, CLOSES[NPRE] + 1), "open window, after the close")
    ra, rb = _rank_level(a), _rank_level(b)
    assert ra["cms0"].any() and ra["cms1"].any()
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), "the window's %s rows differ: the carried accumulators were not folded alike" % k
    # ... and the next window starts from zero in both
    for eng in (a, b):
        _feed(eng, NPRE + 1, range(H))
        eng.window_close(CLOSES[NPRE + 1] * 1_000_000)
    _assert_same(_exports(a, CLOSES[NPRE + 1] + 1), _exports(b, CLOSES[NPRE + 1] + 1), "open window, a window later")
    ra, rb = _rank_level(a), _rank_level(b)
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert dec_a[2]["state"].any()
    a.close()
    b.close()


def test_restore_after_a_pause(torch_mod, packed):
    """B's first close is 400 s after A's last: every 30-s bucket of the 300-s ring has turned.  C = A's twin that ran through."""
    p = packed
    c, b = _source(), _dest()
    assert b.unpack_services(p["blob"]) == (H * S, 0)
    t = CLOSES[NPRE - 1] + 400
    for k in range(3):
        for eng in (c, b):
            if k:
                _feed(eng, NPRE + k, range(H))
            eng.window_close((t + 5 * k) * 1_000_000)
        ec, eb = _exports(c, t + 5 * k + 1), _exports(b, t + 5 * k + 1)
        if k == 0:
            assert not eb["hist_level1"][:, :15].any() and not eb["hll_level1"].any(), "the 5-min level is not empty after a 400-s pause"
            assert eb["hist_level2"][:, 15, 0].sum() > 10000 and eb["hll_level2"].any()
        _assert_same(ec, eb, "pause, close %d" % k)
    c.close()
    b.close()


def test_move_between_live_contexts(torch_mod):
    """A (hosts 0, 1, 2) and B (host 3... here: its own host 2' = index 5) close in lockstep; host 1 moves from A to B after window 3.
    W has every host all along."""
    hosts_b = (5,)
    a, w_ = _source(), _engine()
    _world(w_, (0, 1, 2))
    b = _engine(max_hosts=3, max_services=24)
    for eng in (b, w_):
        eng.register_host(wire.machine_id(5), "cluster1")
        _reg(eng, 5, list(range(S)))

    def present5(eng, w):
        rng = np.random.default_rng(9000 + w)
        eng.handle_resp_events(wire.machine_id(5), _events(rng, 5, {s: 30 + 10 * s for s in range(S)}))

    for w in range(NPRE):
        present5(b, w)
        b.window_close(CLOSES[w] * 1_000_000)
        present5(w_, w)
        _window(w_, w, (0, 1, 2))
        if w == 1:
            assert w_.delete_listeners([_gid(1, DOOMED)]) == 1
            _reg(w_, 1, [7])
    ids1 = np.array([_gid(1, s) for s in range(S)], dtype=np.uint64)
    keep = [(h, s) for h in (0, 2) for s in range(S)]
    keep_before = _exports(a, CLOSES[NPRE], keep)
    blob = a.pack_services(ids1, dev=True)
    b.register_host(wire.machine_id(1), "cluster1")
    _reg(b, 1, list(range(S))[::-1])
    assert b.unpack_services(blob) == (S, 0)
    assert a.delete_listeners(ids1) == S
    _assert_same(keep_before, _exports(a, CLOSES[NPRE], keep), "the services that stayed")
    for w in range(NPRE, NPRE + 2):
        _feed(a, w, (0, 2))
        _decide(a, w)
        a.window_close(CLOSES[w] * 1_000_000)
        present5(b, w)
        _feed(b, w, (1,))
        _decide(b, w)
        b.window_close(CLOSES[w] * 1_000_000)
        present5(w_, w)
        _window(w_, w, (0, 1, 2))
    t = CLOSES[NPRE + 1] + 1
    moved = [(1, s) for s in range(S)]
    # (scan records: the scan's curr / last qps columns come from the kept state and the levels of the service alone)
    _assert_same(_exports(w_, t, moved), _exports(b, t, moved), "the moved host on B")
    _assert_same(_exports(w_, t, keep), _exports(a, t, keep), "A's remaining services")
    torch = torch_mod
    ga, gb, gw = a.tdigest_rollup(capi.ROLLUP_GLOBAL), b.tdigest_rollup(capi.ROLLUP_GLOBAL), w_.tdigest_rollup(capi.ROLLUP_GLOBAL)
    both = torch.cat([ga[0], gb[0]])
    merged = a.tdigest_merge_slabs(both, 2)[1]
    assert int(merged["cnt"].sum()) == int(gw[1][0]["cnt"].sum()) > 10000
    assert int(merged["vmin"]) == int(gw[1][0]["vmin"]) and int(merged["vmax"]) == int(gw[1][0]["vmax"])
    for eng in (a, b, w_):
        eng.close()


def test_refusals_leave_the_destination_unchanged(torch_mod, packed):
    p = packed
    blob = p["blob"]
    t = CLOSES[NPRE]

    def lite(eng, t_, who=ALL):
        """the exports every configuration of this test has"""
        n = eng.num_services()
        slot = np.array([eng.lookup(_gid(h, s)) for h, s in who])
        out = {"hist0": eng.export_hist(0, 0, n), "hist1": eng.export_hist(1, 0, n), "bitmap": eng.export_conn_bitmap(0, n), "counters": eng.export_svc_counters(0, n),
               "act_counters": eng.export_active_conn_counters(0, n), "svc_hll": eng.export_svc_hll(0, n), "hist_level3": eng.export_hist_level(3, t_ * 1_000_000, 0, n),
               "hll_level3": eng.export_svc_hll_level(3, t_ * 1_000_000, 0, n)}
        out["td_sum"], out["td_cnt"], out["td_minmax"] = eng.export_tdigest(0, n)
        out["td_npend"], out["td_pend"] = eng.export_tdigest_pending(0, n)
        return {k: np.asarray(v)[slot] for k, v in out.items()}

    def refused(eng, data, code, word=None, exports=_exports):
        before = exports(eng, t)
        with pytest.raises(capi.GysError) as e:
            eng.unpack_services(data)
        assert e.value.code == code, str(e.value)
        if word:
            assert word in str(e.value), str(e.value)
        _assert_same(before, exports(eng, t), "a refused unpack (%s)" % (word or code))

    for kw, word in ((dict(td_pend_cap=128), "td_pend_cap"), (dict(svc_hll_p=6), "svc_hll_p"), (dict(enable_levels=2), "enable_levels")):
        b = _dest(**kw)
        refused(b, blob, capi.ERR_STATE, word=word, exports=lite)
        b.close()
    b = _dest()
    b.window_close((T0 + 1000) * 1_000_000)  # a destination with a clock of its own
    refused(b, blob, capi.ERR_STATE, word="window")
    b.close()
    b = _dest()
    bad = blob.copy()
    bad[0] ^= 0xFF
    refused(b, bad, capi.ERR_INVAL, word="magic")
    refused(b, blob[:-16], capi.ERR_INVAL)
    refused(b, blob[:40], capi.ERR_INVAL)
    twice = blob.copy()
    twice[64 + 8:64 + 16] = twice[64:64 + 8]  # the second id = the first
    refused(b, twice, capi.ERR_INVAL, word="twice")
    a = p["a"]
    for ids in ([_gid(0, 1), 0x1234], [_gid(0, 1), _gid(0, 1)]):
        with pytest.raises(capi.GysError) as e:
            a.pack_services(ids)
        assert e.value.code == capi.ERR_INVAL
    # an id the destination does not know is skipped and counted; labels set at the destination survive
    assert b.delete_listeners([_gid(2, 3)]) == 1
    ids = np.array([_gid(h, s) for h, s in ALL], dtype=np.uint64)
    b.set_service_groups(ids[ids != _gid(2, 3)], np.arange(len(ids) - 1, dtype=np.uint32) % 3)
    who = [hs for hs in ALL if hs != (2, 3)]
    assert b.unpack_services(blob) == (H * S - 1, 1)
    rows = dict(b.rollup_filtered(group_by=capi.GROUP_LABEL, any_state=True, want=("est",))[0])
    assert rows == {g: sum(1 for i in range(H * S - 1) if i % 3 == g) for g in range(3)}
    keep = [i for i, hs in enumerate(ALL) if hs != (2, 3)]
    _assert_same({k: v[keep] for k, v in p["exports"].items()}, _exports(b, t, who), "the applied services beside a skipped one")
    # the empty blob is valid
    empty = b.pack_services([])
    assert empty.nbytes == 64 == b.service_blob_bytes(0) and b.unpack_services(empty) == (0, 0)
    b.close()


def test_forms_agree(torch_mod, packed, tmp_path, monkeypatch):
    import os
    p = packed
    a = p["a"]
    ids = a.list_service_ids()
    host = a.pack_services(ids)
    dev = a.pack_services(ids, dev=True)
    assert host.tobytes() == dev.cpu().numpy().tobytes(), "the host-pointer form gives another blob than the device form"
    assert a.list_service_ids(3, 5).tolist() == ids[3:8].tolist() and len(a.list_service_ids(1000, 5)) == 0
    b = _dest()
    assert b.unpack_services(dev) == (H * S, 0)
    _assert_same(p["exports"], _exports(b, CLOSES[NPRE]), "device-form unpack")
    b.close()
    # save_state / load_state through a file, in pieces smaller than the context (STATE_FILE_PIECE shrunk: several blobs in the file)
    path = str(tmp_path / "state.gys")
    monkeypatch.setattr(a, "STATE_FILE_PIECE", 64 + 5 * (a.service_blob_bytes(1) - 64), raising=False)
    assert a.save_state(path) == H * S and not os.path.exists(path + ".tmp")
    saved = open(path, "rb").read()
    assert len(saved) > 4 * (a.service_blob_bytes(5) + 8)
    b = _dest()
    assert b.load_state(path) == (H * S, 0)
    _assert_same(p["exports"], _exports(b, CLOSES[NPRE]), "save_state / load_state")
    b.close()
    # a save that fails half way leaves the previous file as it was
    real, calls = a.pack_services, []

    def failing(ids_):
        calls.append(len(ids_))
        if len(calls) == 3:
            raise RuntimeError("the disk is full")
        return real(ids_)

    monkeypatch.setattr(a, "pack_services", failing)
    with pytest.raises(RuntimeError):
        a.save_state(path)
    assert open(path, "rb").read() == saved and not os.path.exists(path + ".tmp")


def test_restore_without_levels_closes_through_the_captured_graph(torch_mod):
    """no levels: gys_window_close replays a captured graph that reads the window number from device memory.  A restored engine's graph
    must see the ADOPTED number: a host state ingested in window e counts at the close only when the graph's window is e too."""
    cfg = dict(enable_levels=False, svc_hll_levels=0)
    a = _engine(**cfg)
    _world(a)
    for w in range(3):
        _feed(a, w, range(H))
        a.window_close(CLOSES[w] * 1_000_000)
    blob = a.pack_services(dev=True)
    b = _engine(**dict(cfg, max_hosts=6, max_services=40))  # (host 1 keeps its doomed listener here and never gets service 7, on both sides)
    for h in (2, 0, 1):
        b.register_host(wire.machine_id(h), "cluster%d" % (h % 2))
    for h in (1, 2, 0):
        _reg(b, h, (list(range(S)) if h != 1 else list(range(S - 1)) + [DOOMED])[::-1])
    assert b.unpack_services(blob) == (H * S, 0)
    who = [(h, s) for h in range(H) for s in range(S) if (h, s) != (1, 7)]
    outs = []
    for eng in (a, b):
        for w in (3, 4):
            _feed(eng, w, range(H))
            for h in range(H):
                eng.handle_host_state(wire.machine_id(h), ntasks=10 + h, nlisten=S, curr_state=1)
            eng.window_close(CLOSES[w] * 1_000_000)
        eng.sync()
        n = eng.num_services()
        slot = np.array([eng.lookup(_gid(h, s)) for h, s in who])
        td = eng.export_tdigest(0, n)
        out = {"hist0": eng.export_hist(0, 0, n)[slot], "hist1": eng.export_hist(1, 0, n)[slot], "bitmap": eng.export_conn_bitmap(0, n)[slot],
               "td_sum": td[0][slot], "td_cnt": td[1][slot], "counters": eng.export_svc_counters(0, n)[slot], "svc_hll": eng.export_svc_hll(0, n)[slot],
               "cluster": np.array([eng.clusterstate("cluster%d" % k).as_tuple() for k in (0, 1)]), "cms": eng.export_cms(0)}
        assert eng.counters()["window_graph_launches"] >= 2
        outs.append(out)
    assert outs[0]["cluster"][:, 0].tolist() == [2, 1] and outs[0]["hist1"][:, 15, 0].sum() > 5000  # hosts with a current state per cluster
    _assert_same(outs[0], outs[1], "restore without levels")
    a.close()
    b.close()
