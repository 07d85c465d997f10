"""The live (listener, client task group) rows of ACTIVE_CONN_STATS on the GPU (gys_config.actconn_pair_cap; gyeeta_amd/csrc/gys_actpairs.hpp):
gys_actconn_list / _list_dev / _svc_stats_dev / _table_stats and gys_json_activeconn against a Python dict written here from the definition
("Live active-connection rows" in include/gysketch.h).  World: 3 hosts x 9 services."""
import ctypes as C
import json
import threading

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers
from tests.test_kernel_logic_actpairs_cpu import ACTIVECONN_FIELDS

pytestmark = pytest.mark.gpu

NH, SP = 3, 9
RING = 3  # GYS_ACT_RING


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine(cap, **kw):
    from gyeeta_amd.engine import SketchEngine
    eng = SketchEngine(max_hosts=NH, max_services=NH * SP + 8, enable_tdigest=False, actconn_pair_cap=cap, **kw)
    info, gids = helpers.register_world(eng, None, range(NH), SP)
    return eng, info, gids


class Model:
    """key (listener id, client id, kind) -> the report of the latest window that named it"""

    def __init__(self):
        self.ent = {}
        self.epoch = 1  # the engine's first open window

    def ingest(self, rec):
        for r in rec:  # in index order: the last row of the last call stays
            lid, cid = int(r["listener_glob_id"]), int(r["cli_aggr_task_id"])
            if lid == 2 ** 64 - 1 or cid == 2 ** 64 - 1:
                continue
            k = (lid, cid, (int(r["flags"]) >> 1) & 1)
            e = self.ent.get(k)
            if e is None or e["window"] != self.epoch:
                e = self.ent[k] = dict(window=self.epoch, active_conns=0, bytes_sent=0, bytes_received=0, nrows=0, cli_delay_msec=0, ser_delay_msec=0,
                                       max_rtt_msec=np.float32(0), flags=0)
            e["active_conns"] += int(r["active_conns"])
            e["bytes_sent"] += int(r["bytes_sent"])
            e["bytes_received"] += int(r["bytes_received"])
            e["nrows"] += 1
            e["cli_delay_msec"] = max(e["cli_delay_msec"], int(r["cli_delay_msec"]))
            e["ser_delay_msec"] = max(e["ser_delay_msec"], int(r["ser_delay_msec"]))
            rtt = r["max_rtt_msec"]
            e["max_rtt_msec"] = max(e["max_rtt_msec"], rtt if rtt >= 0 else np.float32(0))  # (a NaN compares false)
            e["flags"] |= int(r["flags"])
            e["desc"] = (bytes(r["ser_comm"]), bytes(r["cli_comm"]), tuple(int(x) for x in r["remote_machine_id"]), int(r["remote_madhava_id"]))

    def close(self):
        self.epoch += 1

    def live(self):
        return {k: e for k, e in self.ent.items() if self.epoch - e["window"] <= RING}


def _check_rows(rows, want, slot_of):
    """rows (numpy, in the order of gys_actconn_list) == the model's entries `want`, field for field"""
    keys = [(int(r["listener_glob_id"]), int(r["cli_aggr_task_id"]), int(r["kind"])) for r in rows]
    assert keys == sorted(want), (len(keys), len(want))
    for r, k in zip(rows, keys):
        e = want[k]
        for f in ("window", "active_conns", "bytes_sent", "bytes_received", "nrows", "cli_delay_msec", "ser_delay_msec", "flags"):
            assert int(r[f]) == e[f], (k, f, int(r[f]), e[f])
        assert np.float32(r["max_rtt_msec"]).tobytes() == np.float32(e["max_rtt_msec"]).tobytes(), k
        assert (bytes(r["ser_comm"]), bytes(r["cli_comm"]), tuple(int(x) for x in r["remote_machine_id"]), int(r["remote_madhava_id"])) == e["desc"], k
        assert int(r["slot"]) == (slot_of.get(k[0], capi.NOSLOT) if k[2] == 0 else capi.NOSLOT), k
        assert int(r["reserved"]) == 0 and not r["pad"].any()


def _compare(eng, model, slot_of, host_of_slot, torch):
    live = model.live()
    rc, rows, nmatch = eng.actconn_list()
    assert rc == capi.OK and nmatch == len(live)
    _check_rows(rows, live, slot_of)
    if not live:
        return
    keys = sorted(live)
    some = keys[len(keys) // 2]
    totals = sorted(e["bytes_sent"] + e["bytes_received"] for e in live.values())
    acts = sorted(e["active_conns"] for e in live.values())
    local_known = [k for k in keys if k[2] == 0 and k[0] in slot_of]
    sels = [
        (dict(listener=some[0]), lambda k, e: k[0] == some[0]),
        (dict(client=some[1]), lambda k, e: k[1] == some[1]),
        (dict(listener=some[0], client=some[1]), lambda k, e: k[0] == some[0] and k[1] == some[1]),
        (dict(kind=0), lambda k, e: k[2] == 0),
        (dict(kind=1), lambda k, e: k[2] == 1),
        (dict(min_bytes=totals[len(totals) // 2]), lambda k, e: e["bytes_sent"] + e["bytes_received"] >= totals[len(totals) // 2]),
        (dict(min_active_conns=acts[(2 * len(acts)) // 3]), lambda k, e: e["active_conns"] >= acts[(2 * len(acts)) // 3]),
        (dict(listener=12345), lambda k, e: False),
    ]
    for hs in range(NH):
        sels.append((dict(host_slot=hs), lambda k, e, hs=hs: k[2] == 0 and k[0] in slot_of and host_of_slot[slot_of[k[0]]] == hs))
    if local_known:
        lk = local_known[0]
        hs = host_of_slot[slot_of[lk[0]]]
        sels.append((dict(host_slot=hs, client=lk[1], kind=0, min_active_conns=1),
                     lambda k, e: k[2] == 0 and k[0] in slot_of and host_of_slot[slot_of[k[0]]] == hs and k[1] == lk[1] and e["active_conns"] >= 1))
    for kw, pred in sels:
        want = {k: e for k, e in live.items() if pred(k, e)}
        sel = eng.actconn_sel(**kw)
        rc, rows, nmatch = eng.actconn_list(sel)
        assert rc == capi.OK and nmatch == len(want), (kw, nmatch, len(want))
        _check_rows(rows, want, slot_of)
        if len(want) >= 1:  # the cap too small: the count, and nothing else
            rc, rows, nmatch = eng.actconn_list(sel, cap=len(want) - 1)
            assert rc == capi.ERR_NOMEM and nmatch == len(want) and len(rows) == 0, kw
        # the device form: any order, min(matches, cap) rows
        for cap in (len(want) + 3, len(want) // 2):
            t, nm = eng.actconn_list_dev(sel, cap)
            eng.sync()
            assert nm == len(want)
            got = np.frombuffer(t.cpu().numpy().tobytes(), dtype=eng.ACTCONN_ROW_DT)
            nw = min(cap, len(want))
            gk = {(int(r["listener_glob_id"]), int(r["cli_aggr_task_id"]), int(r["kind"])) for r in got[:nw]}
            assert len(gk) == nw and gk <= set(want), kw
            assert not t[nw:].any().item(), "rows beyond min(matches, cap) were written"
            if cap >= len(want):
                _check_rows(np.sort(got[:nw], order=["listener_glob_id", "cli_aggr_task_id", "kind"]), want, slot_of)
    # per-service sums, and a ranking on them
    nsvc = eng.num_services()
    want = np.zeros((nsvc, 4), dtype=np.float64)
    for k, e in live.items():
        if k[2] == 0 and k[0] in slot_of:
            want[slot_of[k[0]]] += [1, e["active_conns"], e["bytes_sent"] + e["bytes_received"], e["nrows"]]
    st = eng.actconn_svc_stats_dev()
    assert np.array_equal(st.cpu().numpy()[:nsvc], want)
    for col in (0, 2):
        ent, nel = eng.topk(st.view(-1)[col:], 5, stride=4, nrows=nsvc)
        order = sorted(range(nsvc), key=lambda s: (-want[s, col], s))[:5]
        assert nel == nsvc and [int(x) for x in ent["row"]] == order and [float(x) for x in ent["value"]] == [want[s, col] for s in order]
    ts = eng.actconn_table_stats()
    assert ts["live_keys"] == len(live) and ts["rows_dropped"] == 0 and ts["occupied"] >= len(live) and ts["entries"] >= 2 * eng.cfg.actconn_pair_cap


def _slots(eng, gids):
    slot_of = {int(g): eng.lookup(int(g)) for h in gids for g in gids[h]}
    host_of_slot = {}
    for h in gids:
        for g in gids[h]:
            host_of_slot[slot_of[int(g)]] = h  # (register_world: host h has host slot h)
    return slot_of, host_of_slot


def test_six_windows_of_reports_equal_the_dict_model(torch_mod):
    eng, info, gids = _engine(4096)
    try:
        assert all(info[h][1] == h for h in info)
        slot_of, host_of_slot = _slots(eng, gids)
        rng = np.random.default_rng(11)
        model = Model()
        for w in range(6):
            # staggered phases: host h reports every third window; in window 0 host 0 reports twice (the calls add), in window 4 host 1
            # brings a row with the free marker as an id
            for h in range(NH):
                if w % 3 != h:
                    continue
                for rep in range(2 if (w == 0 and h == 0) else 1):
                    rec = wire.synth_active_conns(rng, 150 + 40 * h, h, SP, ntasks=12, remote_listen_frac=0.25, unknown_frac=0.05)
                    rec["max_rtt_msec"][::17] = -3.0
                    rec["max_rtt_msec"][5::19] = np.nan
                    rec["ser_comm"] = [b"svc%d" % i for i in range(len(rec))]
                    rec["remote_madhava_id"] = rng.integers(1, 1 << 62, len(rec), dtype=np.uint64)
                    if w == 4:
                        rec["cli_aggr_task_id"][3] = 2 ** 64 - 1
                    eng.handle_partha_active_conns(info[h][0], rec.tobytes(), len(rec))
                    model.ingest(rec)
                    _compare(eng, model, slot_of, host_of_slot, torch_mod)
            eng.window_close(1_700_000_000_000_000 + w * 5_000_000)
            model.close()
            _compare(eng, model, slot_of, host_of_slot, torch_mod)
            # the Count-Min gauge never reads below the table: live keys whose report lies in a closed window
            nchecked = 0
            for k, e in model.live().items():
                if e["window"] >= model.epoch:
                    continue
                base = 6 if k[2] else 0
                assert eng.pair_cms(k[0], k[1], base) >= e["active_conns"], k
                assert eng.pair_cms(k[0], k[1], base + 1) >= e["bytes_sent"] + e["bytes_received"], k
                nchecked += 1
            assert nchecked > 100
        assert eng.actconn_table_stats()["rows_bad_key"] == 1
        assert any(e["window"] < model.epoch - RING for e in model.ent.values()), "no entry aged out: the case is trivial"
        assert any(k[2] == 1 for k in model.ent) and any(k[2] == 0 and k[0] not in slot_of for k in model.ent)
    finally:
        eng.close()


def _one_key_rows(n, lid, cid, seed):
    rng = np.random.default_rng(seed)
    rec = wire.synth_active_conns(rng, n, 0, SP, remote_listen_frac=0.0, unknown_frac=0.0)
    rec["listener_glob_id"], rec["cli_aggr_task_id"] = lid, cid
    rec["cli_comm"] = [b"c%d" % i for i in range(n)]
    return rec


@pytest.mark.parametrize("n", [1000, 2048])  # the one-launch form and the three-pass form
def test_many_rows_of_one_key(torch_mod, n):
    eng, info, gids = _engine(2048)
    try:
        slot_of, _ = _slots(eng, gids)
        model = Model()
        rec = _one_key_rows(n, int(gids[0][2]), 0xC11E, n)
        eng.handle_partha_active_conns(info[0][0], rec.tobytes(), n)
        model.ingest(rec)
        rc, rows, nmatch = eng.actconn_list()
        assert rc == capi.OK and nmatch == 1 and int(rows[0]["nrows"]) == n and bytes(rows[0]["cli_comm"]) == b"c%d" % (n - 1)
        _check_rows(rows, model.live(), slot_of)
        ts = eng.actconn_table_stats()
        assert ts["occupied"] == 1 and ts["rows_dropped"] == 0
    finally:
        eng.close()


def test_2048_distinct_keys_at_cap_2048_and_the_rebuild(torch_mod):
    eng, info, gids = _engine(2048)
    try:
        slot_of, _ = _slots(eng, gids)
        rng = np.random.default_rng(5)
        model = Model()

        def fresh(n, first):
            rec = wire.synth_active_conns(rng, n, 1, SP, remote_listen_frac=0.3, unknown_frac=0.0)
            rec["cli_aggr_task_id"] = wire.splitmix64(np.arange(first, first + n, dtype=np.uint64))
            return rec

        rec = fresh(2048, 0)
        eng.handle_partha_active_conns(info[1][0], rec.tobytes(), len(rec))
        model.ingest(rec)
        rc, rows, nmatch = eng.actconn_list()
        assert rc == capi.OK and nmatch == 2048
        _check_rows(rows, model.live(), slot_of)
        ts = eng.actconn_table_stats()
        assert ts["entries"] == 4096 and ts["occupied"] == 2048 and ts["rows_dropped"] == 0 and ts["rebuilds"] == 0
        for w in range(3):  # (the first 2 048 keys stay live through three closes and are gone with the fourth, below)
            eng.window_close(1_700_000_000_000_000 + w * 5_000_000)
            model.close()
        assert eng.actconn_list()[2] == 2048
        # 512 fresh keys per window: at most 2 048 live keys (four windows' worth), the table never drops a row
        first = 2048
        for w in range(3, 13):
            eng.window_close(1_700_000_000_000_000 + w * 5_000_000)
            model.close()
            rec = fresh(512, first)
            first += 512
            eng.handle_partha_active_conns(info[1][0], rec.tobytes(), len(rec))
            model.ingest(rec)
            rc, rows, nmatch = eng.actconn_list()
            assert len(model.live()) <= 2048
            assert rc == capi.OK and nmatch == len(model.live())
            _check_rows(rows, model.live(), slot_of)
        ts = eng.actconn_table_stats()
        assert ts["rows_dropped"] == 0 and ts["rebuilds"] >= 2 and ts["occupied"] <= 2048 + 512, ts
    finally:
        eng.close()


def test_16_threads_give_the_sums_of_the_sequential_model(torch_mod):
    eng, info, gids = _engine(4096)
    try:
        slot_of, _ = _slots(eng, gids)
        rng = np.random.default_rng(23)
        pool = wire.synth_active_conns(rng, 600, 2, SP, ntasks=10, remote_listen_frac=0.2, unknown_frac=0.05)
        # every row of a key carries the same descriptive fields, so that the payload rule is not in question
        pool["ser_comm"], pool["cli_comm"], pool["remote_madhava_id"] = b"svc", b"cli", 7
        batches = [pool[rng.integers(0, len(pool), 100 + 100 * t)].copy() for t in range(16)]  # 100 .. 1 600 rows: both forms
        errs = []

        def run(t):
            try:
                for _ in range(3):
                    eng.handle_partha_active_conns(info[2][0], batches[t].tobytes(), len(batches[t]))
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)

        th = [threading.Thread(target=run, args=(t,)) for t in range(16)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        model = Model()
        for t in range(16):
            for _ in range(3):
                model.ingest(batches[t])
        rc, rows, nmatch = eng.actconn_list()
        assert rc == capi.OK and nmatch == len(model.live())
        _check_rows(rows, model.live(), slot_of)
    finally:
        eng.close()


def test_deleted_listener_reads_noslot_until_it_is_registered_again(torch_mod):
    eng, info, gids = _engine(512)
    try:
        slot_of, host_of_slot = _slots(eng, gids)
        lid = int(gids[1][4])
        rec = _one_key_rows(3, lid, 0xABCD, 1)
        eng.handle_partha_active_conns(info[1][0], rec.tobytes(), len(rec))
        sel = eng.actconn_sel(listener=lid)
        by_host = eng.actconn_sel(host_slot=1)
        rc, rows, _ = eng.actconn_list(sel)
        assert rc == capi.OK and len(rows) == 1 and int(rows[0]["slot"]) == slot_of[lid]
        assert eng.actconn_list(by_host)[2] == 1
        assert eng.delete_listeners([lid]) == 1
        rc, rows, _ = eng.actconn_list(sel)
        assert rc == capi.OK and len(rows) == 1 and int(rows[0]["slot"]) == capi.NOSLOT and int(rows[0]["nrows"]) == 3
        assert eng.actconn_list(by_host)[2] == 0
        assert eng.actconn_svc_stats_dev().cpu().numpy().sum() == 0
        # registered again, under another host: the free slot, and that host's rows
        new = eng.register_listeners_slots(info[2][0], [lid], wire.listener_netns(2, np.array([40])), wire.listener_port(np.array([40])))
        rc, rows, _ = eng.actconn_list(sel)
        assert rc == capi.OK and len(rows) == 1 and int(rows[0]["slot"]) == int(new[0]) == eng.lookup(lid)
        assert eng.actconn_list(by_host)[2] == 0 and eng.actconn_list(eng.actconn_sel(host_slot=2))[2] == 1
        assert eng.actconn_svc_stats_dev().cpu().numpy()[int(new[0])].tolist() == [1.0, float(rec["active_conns"].sum()), float(rec["bytes_sent"].sum() + rec["bytes_received"].sum()), 3.0]
    finally:
        eng.close()


def test_json_activeconn_against_a_literal(torch_mod):
    eng, info, gids = _engine(64)
    try:
        rec = np.zeros(4, dtype=wire.ACTIVE_CONN_STATS)
        rec["listener_glob_id"] = [0x1122334455667788, 0x1122334455667788, 0x0A, 0x0B]
        rec["cli_aggr_task_id"] = [0xFEDCBA9876543210, 0xFEDCBA9876543210, 0x01, 0x02]
        rec["ser_comm"] = [b"nginx", b"nginx", b'q"uote', b"remote"]
        rec["cli_comm"] = [b"curl", b"curl", b"cli\\ent", b"x"]
        rec["remote_machine_id"] = [[0x0102030405060708, 0x1112131415161718]] * 2 + [[1, 2], [3, 4]]
        rec["remote_madhava_id"] = [0xAABBCCDD00112233, 0xAABBCCDD00112233, 5, 6]
        rec["bytes_sent"] = [1000, 234, 7, 1]
        rec["bytes_received"] = [5000, 1, 0, 1]
        rec["cli_delay_msec"] = [3, 9, 0, 1]
        rec["ser_delay_msec"] = [8, 2, 0, 1]
        rec["max_rtt_msec"] = [1.25, 0.5, 12.3456, 1]
        rec["active_conns"] = [4, 6, 1, 1]
        rec["flags"] = [0, wire.ACTIVE_FLAG_CLI_LISTENER_PROC, 0, wire.ACTIVE_FLAG_REMOTE_LISTEN]
        eng.handle_partha_active_conns(info[0][0], rec.tobytes(), len(rec))
        got = eng.json_activeconn(madid="00000000000000aa", timestr="2026-01-02T03:04:05Z")
        want = ('{"madid":"00000000000000aa","activeconn":['
                '{"time":"2026-01-02T03:04:05Z","svcid":"000000000000000a","svcname":"q\\"uote","cprocid":"0000000000000001","cname":"cli\\\\ent",'
                '"cparid":"00000000000000010000000000000002","cmadid":"0000000000000005","cnetout":7,"cnetin":0,"cdelms":0,"sdelms":0,"rttms":12.346,"nconns":1,"csvc":false},'
                '{"time":"2026-01-02T03:04:05Z","svcid":"1122334455667788","svcname":"nginx","cprocid":"fedcba9876543210","cname":"curl",'
                '"cparid":"01020304050607081112131415161718","cmadid":"aabbccdd00112233","cnetout":1234,"cnetin":5001,"cdelms":9,"sdelms":8,"rttms":1.250,"nconns":10,"csvc":true}'
                ']}')
        assert got == want
        obj = json.loads(got)
        assert all(list(o) == ACTIVECONN_FIELDS for o in obj["activeconn"])
        assert json.loads(eng.json_activeconn(eng.actconn_sel(kind=1)))["activeconn"] == []
        assert len(json.loads(eng.json_activeconn(eng.actconn_sel(listener=0x0A)))["activeconn"]) == 1
        # the buffer convention of the other gys_json_* calls: too small -> GYS_ERR_NOMEM and the length
        need = C.c_size_t()
        buf = C.create_string_buffer(8)
        assert eng.L.gys_json_activeconn(eng.h, None, b"00000000000000aa", b"2026-01-02T03:04:05Z", buf, 8, C.byref(need)) == capi.ERR_NOMEM and need.value == len(want)
    finally:
        eng.close()


def test_table_off_every_call_answers_state_and_the_rollups_are_unchanged(torch_mod):
    off, info, gids = _engine(0)
    on, info2, _ = _engine(1024)
    try:
        n32, n64, row = C.c_uint32(), C.c_size_t(), (capi.ActconnRow * 4)()
        d = torch_mod.zeros(1024, dtype=torch_mod.uint8, device=off.device)
        st = capi.ActconnTblStats()
        L, h = off.L, off.h
        assert L.gys_actconn_list(h, None, row, 4, C.byref(n32), C.byref(n32)) == capi.ERR_STATE
        assert L.gys_actconn_list_dev(h, None, C.c_void_p(d.data_ptr()), 4, C.byref(n32)) == capi.ERR_STATE
        assert L.gys_actconn_svc_stats_dev(h, C.c_void_p(d.data_ptr())) == capi.ERR_STATE
        assert L.gys_actconn_table_stats(h, C.byref(st)) == capi.ERR_STATE
        assert L.gys_json_activeconn(h, None, b"0" * 16, b"", None, 0, C.byref(n64)) == capi.ERR_STATE
        rng = np.random.default_rng(3)
        for w in range(2):
            for hh in range(NH):
                rec = wire.synth_active_conns(rng, 1500 if hh == 1 else 300, hh, SP)
                for eng, inf in ((off, info), (on, info2)):
                    eng.handle_partha_active_conns(inf[hh][0], rec.tobytes(), len(rec))
            for eng in (off, on):
                eng.window_close(1_700_000_000_000_000 + w * 5_000_000)
            for which in (0, 1, 6, 7):
                assert np.array_equal(off.export_pair_cms(which), on.export_pair_cms(which)), which
            assert np.array_equal(off.export_active_conn_counters(), on.export_active_conn_counters())
            assert off.export_pair_cms(0).any() and off.export_active_conn_counters().any()
        co, cn = off.counters(), on.counters()
        assert all(co[k] == cn[k] for k in ("actconn_records", "actconn_remote_listen", "actconn_unknown_listener"))
        assert on.actconn_table_stats()["live_keys"] > 0
    finally:
        off.close()
        on.close()
