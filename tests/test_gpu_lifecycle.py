"""The context's memory over its life on the GPU: every buffer that is allocated on first use or grows is driven once at a small size and
once at a size that forces a re-allocation, the context is destroyed, and all of that three times in one process.  What the large call
of each pair leaves behind must equal, byte for byte, what a FRESH context holds after the large call alone -- a buffer that grew under
the engine (gyeeta_amd/csrc/gys_devmem.hpp) is as good as one that was allocated at its final size.

How "equal" is made exact: the small calls only ever touch host 3 (its eight services, slots 24..31), the large calls hosts 0..2; every
comparison is over the per-service state of slots 0..23 (or ids of hosts 0..2), which the small calls cannot reach.

Shapes: 4 hosts x 8 services, max_batch_events 4096, t-digests, levels, per-service HLL (p = 6) with levels, the connection pair CMS.
A response payload above 1 MiB (43 700 events) cannot be INGESTED under max_batch_events = 4096; the call still takes a staging slot of
that size before it is refused, so it is made and must be refused alike (GYS_ERR_NOMEM) by the grown and the fresh context; the largest
valid response calls (4096 events) carry the state.  Listener-state records above 2 MiB take the staging ring for real."""
import ctypes as C
import functools

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

NH, SP, NCMP = 4, 8, 24  # hosts, services per host, slots compared (hosts 0..2)
T0 = 1_700_000_000
BOUND = (1030, 1030, 17)  # bound-address listeners of hosts 4, 5, 6: 2048 + 2048 + 32 candidate records > the pool's first 4096


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine():
    from gyeeta_amd.engine import SketchEngine
    return SketchEngine(max_hosts=8, max_services=2304, max_batch_events=4096, enable_tdigest=True, enable_levels=1, svc_hll_p=6, svc_hll_levels=1,
                        conn_pair_cms=True)


def _frames(rng, conn_hosts, nconn, lst_host):
    rec = wire.synth_tcp_conns(rng, nconn, conn_hosts, SP, dup_frac=0.1)
    ls = wire.synth_listener_states(rng, lst_host, np.arange(SP))
    return wire.frame_event_notify(wire.NOTIFY_TCP_CONN, nconn, rec.tobytes()) + wire.frame_event_notify(wire.NOTIFY_LISTENER_STATE, SP, ls.tobytes())


@functools.lru_cache(maxsize=None)
def _payloads():
    """every input of a drive, made once (seeded) and shared by the four contexts"""
    rng = np.random.default_rng(0x11FE)
    p = {}
    p["resp_small"] = helpers.make_resp_events(rng, 3, 40, SP).tobytes()  # ~1 KB
    p["resp_large"] = [helpers.make_resp_events(rng, h, 4096, SP).tobytes() for h in range(3)]
    p["resp_too_large"] = helpers.make_resp_events(rng, 0, 43700, SP).tobytes()  # > 1 MiB
    p["resp6_small"] = np.zeros(21, dtype=wire.RESP_EVENT6).tobytes()  # ~1 KB of events nobody listens for
    p["conn_small"] = wire.synth_tcp_conns(rng, 3, [3], SP).tobytes()  # 840 B
    p["conn_large"] = wire.synth_tcp_conns(rng, 4000, [0, 1, 2], SP, dup_frac=0.1).tobytes()  # 1.12 MB
    p["lst_small"] = wire.synth_listener_states(rng, 3, rng.integers(0, SP, 11)).tobytes()  # 968 B
    p["lst_large0"] = wire.synth_listener_states(rng, 0, rng.integers(0, SP, 12000)).tobytes()  # 1.06 MB: the record queue
    p["lst_large1"] = wire.synth_listener_states(rng, 1, rng.integers(0, SP, 24000)).tobytes()  # 2.1 MB: a staging slot
    p["wire_small"] = _frames(rng, [3], 3, 3)  # ~250 slots of 8 bytes
    p["wire_large"] = _frames(rng, [0, 1, 2], 2048, 2)  # 573 KB: more than 65536 slots
    assert len(p["resp_too_large"]) > 1 << 20 and len(p["conn_large"]) > 1 << 20 and len(p["lst_large0"]) > 1 << 20 and len(p["wire_large"]) // 8 > 65536
    ev = helpers.make_resp_events(rng, 4, 4096, BOUND[0], unknown_frac=0.0)
    ev["saddr"] = np.where(rng.random(4096) < 0.3, int.from_bytes(bytes([10, 0, 0, 99]), "little"), ev["saddr"])  # (not the listeners' address: no match)
    p["resp_bound"] = ev.tobytes()
    return p


def _per_service(eng):
    s, c, m = eng.export_tdigest(0, NCMP)
    npend, pend = eng.export_tdigest_pending(0, NCMP)
    return {"hist0": eng.export_hist(0, 0, NCMP), "hist1": eng.export_hist(1, 0, NCMP), "td_sum": s, "td_cnt": c, "td_minmax": m, "td_npend": npend,
            "td_pend": pend, "counters": eng.export_svc_counters(0, NCMP), "bitmap": eng.export_conn_bitmap(0, NCMP), "svc_hll": eng.export_svc_hll(0, NCMP),
            "svcstate": np.frombuffer("\n".join(eng.json_svcstate(wire.machine_id(h)) for h in range(3)).encode(), dtype=np.uint8)}


def _drive(torch, grow):
    """one context from create to destroy; grow: every large call is preceded by its small twin (and the candidate pool is made to grow)"""
    p = _payloads()
    eng = _engine()
    res = {}
    info, gids = helpers.register_world(eng, None, range(NH), SP)
    mid = [info[h][0] for h in range(NH)]
    ids012 = set(int(g) for h in range(3) for g in gids[h])
    # host-pointer response calls: the response queue's batches; the staging ring (16 slots, oldest first: after 16 small calls every slot
    # holds its first megabyte, and the next larger call re-allocates one)
    if grow:
        eng.handle_resp_events(mid[3], p["resp_small"])
        for _ in range(16):
            eng.handle_resp_events_v6(mid[3], p["resp6_small"])
    for h in range(3):
        eng.handle_resp_events(mid[h], p["resp_large"][h])
    with pytest.raises(capi.GysError) as ei:
        eng.handle_resp_events(mid[0], p["resp_too_large"])
    res["too_large_code"] = np.array([ei.value.code])
    assert ei.value.code == capi.ERR_NOMEM  # (gysketch.h: capacity -- hosts, services, batch staging -- exhausted)
    # connection and listener-state records
    if grow:
        eng.partha_tcp_conn_info(mid[3], p["conn_small"], 3)
        eng.partha_listener_state(mid[3], p["lst_small"], 11)
    eng.partha_tcp_conn_info(mid[0], p["conn_large"], 4000)
    eng.partha_listener_state(mid[0], p["lst_large0"], 12000)
    eng.partha_listener_state(mid[1], p["lst_large1"], 24000)
    # the wire front end
    if grow:
        st = eng.handle_comm_stream(mid[3], p["wire_small"])
        assert st.nrecords == 3 + SP and st.nmsgs_invalid == 0
    st = eng.handle_comm_stream(mid[2], p["wire_large"])
    assert st.nrecords == 2048 + SP and st.nmsgs_invalid == 0 and st.bytes_consumed == len(p["wire_large"])
    eng.sync()
    for k, v in _per_service(eng).items():
        res["open_" + k] = v
    assert res["open_hist1"][:, 15, 0].all() and res["open_counters"].any() and res["open_svcstate"].size > 1000  # (the records did arrive)
    eng.window_close(T0 * 1_000_000)
    # the synthetic generator: its Zipf table at two sizes
    d_ev = torch.empty(4096 * 24, dtype=torch.uint8, device="cuda")
    if grow:
        eng.gen_resp_events(d_ev.data_ptr(), 4096, 7, 3, 1, 4, zipf_milli=1100)
    segs = eng.gen_resp_events(d_ev.data_ptr(), 4096, 8, 0, 3, SP, zipf_milli=1100)
    eng.sync()
    res["gen"] = d_ev.cpu().numpy()
    eng.handle_resp_events_dev(segs, d_ev.data_ptr(), 4096)
    eng.window_close((T0 + 5) * 1_000_000)
    tusec = (T0 + 6) * 1_000_000
    # stale listeners: the id buffer at two sizes (everybody who reported two windows ago is "aged" at max_age 0)
    if grow:
        few, nf = eng.list_stale_listeners(eng.STALE_AGED, 0, cap=4)
        assert len(few) == 4 and nf > 4
    ids, nf = eng.list_stale_listeners(eng.STALE_AGED, 0, cap=64)
    assert nf == len(ids)
    res["stale"] = np.array([i for i in ids.tolist() if i in ids012], dtype=np.uint64)
    assert len(res["stale"]) == NCMP
    # labels (first use), and a roll-up by label
    all_ids = np.concatenate([gids[h] for h in range(3)])
    labels = (np.arange(NCMP) % 5).astype(np.uint32)
    if grow:
        eng.set_service_groups(all_ids[:1], labels[:1])
    eng.set_service_groups(all_ids, labels)
    rows, nr, out = eng.rollup_filtered(group_by=capi.GROUP_LABEL, any_state=True)
    assert nr == 5
    res["rf_rows"], res["rf_slabs"], res["rf_regs"] = np.array(rows), out["slabs"].view(np.uint8), out["regs"]
    # the listener scan and the decision (its history bytes: first use)
    notify_dev, _, scan = eng.scan_listener_state(tusec)
    res["decision"] = eng.decide_listener_state(scan, None, notify_dev)[:NCMP].view(np.uint8)
    res["scan"] = scan[:NCMP].view(np.uint8)
    # per-call temporaries
    res["scan_quantiles"] = np.asarray(eng.scan_quantiles([0.25, 0.5, 0.95, 0.99]))[:NCMP]
    res["day_stats"] = np.frombuffer(bytes(eng.export_day_stats(tusec, 0, NCMP)), dtype=np.uint8)
    for k, v in _per_service(eng).items():
        res["closed_" + k] = v
    # bound-address listeners: the candidate pool.  Grown: three registration calls (2048 + 2048 + 32 records: the third moves the pool,
    # host 4's records with it); fresh: host 4 alone, in a pool that never moves.  Host 4's events must find the same listeners.
    first = None
    for k, n in enumerate(BOUND if grow else BOUND[:1]):
        h = 4 + k
        eng.register_host(wire.machine_id(h), "cluster9")
        s = np.arange(n)
        f = eng.register_listeners(wire.machine_id(h), wire.glob_id(np.full(n, h), s), wire.listener_netns(h, s), wire.listener_port(s),
                                   addrs=[bytes([10, 0, 0, h])] * n)
        first = f if first is None else first
    assert first == NH * SP
    eng.handle_resp_events(wire.machine_id(4), p["resp_bound"])
    eng.sync()
    res["bound_hist"] = eng.export_hist(1, first, BOUND[0])
    hits = int(res["bound_hist"][:, 15, 0].sum())
    assert 2000 < hits < 3400  # ~70 % of 4096 events carry the listeners' address (less the events the generator marks bad)
    eng.close()
    return res


@pytest.fixture(scope="module")
def fresh(torch_mod):
    return _drive(torch_mod, grow=False)


def test_grown_buffers_equal_fresh_ones_three_contexts(torch_mod, fresh):
    for rnd in range(3):
        got = _drive(torch_mod, grow=True)
        assert got.keys() == fresh.keys()
        for k in fresh:
            a, b = np.asarray(got[k]), np.asarray(fresh[k])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (rnd, k)


def test_create_on_an_invalid_device_fails_cleanly(torch_mod):
    """gys_create returns through its guard on every HIPCHK: an invalid ordinal is GYS_ERR_HIP (an API error, no fault), nothing is left
    behind -- no context, no pending HIP error for the process's other users of the runtime -- and the next create works"""
    L = capi.load()
    cfg = capi.Config()
    cfg.struct_size = C.sizeof(capi.Config)
    cfg.device = torch_mod.cuda.device_count()
    cfg.rank, cfg.nranks = 0, 1
    cfg.max_hosts, cfg.max_services, cfg.max_clusters, cfg.max_batch_events = NH, NH * SP, 4, 4096
    cfg.enable_tdigest = 1
    h = C.c_void_p()
    assert L.gys_create(C.byref(cfg), C.byref(h)) == capi.ERR_HIP
    assert not h.value and b"hipSetDevice" in L.gys_last_error()
    # ... and no stale "last error" in the runtime either: the thread's next launch check (torch's reads hipGetLastError) finds nothing
    assert int(torch_mod.ones(8, dtype=torch_mod.int32, device="cuda").sum().item()) == 8
    cfg.device = 0
    assert L.gys_create(C.byref(cfg), C.byref(h)) == capi.OK and h.value
    assert L.gys_sync(h) == capi.OK
    L.gys_destroy(h)
