"""GPU parity of the event kernel k_resp_host at the segment lengths its event loads treat differently: a partly filled last group packs
its events into the four slots of the lowest threads (slot stride = a quarter of them, rounded up to whole waves) and the waves that
hold no event leave the group loop.  Every length around a slot (T threads), a group (G = 4 T events) and a tile (TILE = TPT x T events)
of each tile form -- the lengths any change of where and when the event words are loaded has to get right -- runs against the oracle on the same bytes: HLL
registers, both Count-Min tables, the all-service histogram, per-service records and bitmaps, digest state, buffered values as multisets.

The tile form follows from the batch's largest listener table (gys_resp_plan.hpp, resp_tile_events): 400 listeners leave room for two
512-thread workgroups per CU (512 x 12), 1000 listeners take the 1024 x 16 form, and the 48 KB of per-key areas of 2000 listeners leave
only an 8192-event tile image (1024 x 8).  Batches are handed over as device buffers of exactly n events, so the last segment ends at
the buffer's last byte."""
import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_resp import _compare_all, _compare_window, _engine
from tests.test_gpu_round5 import World

pytestmark = pytest.mark.gpu

# tile form -> (listeners per host, threads T, events per thread TPT)
FORMS = {"1024x16": (1000, 1024, 16), "512x12": (400, 512, 12), "1024x8": (2000, 1024, 8)}


def edge_lengths(T, TPT):
    G, TILE = 4 * T, TPT * T
    return [1, 63, 64, 65, T - 1, T, T + 1, G - 1, G, G + 1, G + 439, TILE - 1, TILE, TILE + 1, TILE + G + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 4535]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _run_dev(torch, eng, orc, parts, slots):
    """one device batch of len(parts) adjacent segments; the buffer holds the events and nothing behind them"""
    from gyeeta_amd import capi
    buf = helpers.concat_events(parts)
    firsts = np.cumsum([0] + [len(x) for x in parts[:-1]])
    segs = (capi.RespSeg * len(parts))()
    for i, s in enumerate(slots):
        segs[i].host_slot, segs[i].first_event = s, int(firsts[i])
    d = torch.from_numpy(buf.view(np.uint8).copy()).cuda()
    assert d.numel() == 24 * len(buf)
    eng.handle_resp_events_dev(segs, d.data_ptr(), len(buf))
    eng.sync()
    orc.resp_batch(buf.tobytes(), list(slots), [int(f) for f in firsts])
    return len(buf)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_host_every_edge_length(torch_mod, oracle, form):
    """one host per tile form, one batch per length: the segment IS the batch"""
    L, T, TPT = FORMS[form]
    rng = np.random.default_rng(700 + TPT)
    eng = _engine(max_hosts=2, max_services=2048, max_batch_events=1 << 16, resp_path=2)
    orc = oracle.OracleEngine(2048)
    info, _ = helpers.register_world(eng, orc, [0], L)
    total = 0
    for n in edge_lengths(T, TPT):
        total += _run_dev(torch_mod, eng, orc, [helpers.make_resp_events(rng, 0, n, L)], [info[0][1]])
        _compare_all(eng, orc, oracle)
    c, oc = eng.counters(), orc.counters()
    assert c["resp_batches_general"] == 0 and c["resp_batches_host_split"] == 0
    assert c["resp_events"] == total == oc["events"]
    assert c["resp_dropped_range"] == oc["dropped_range"] and c["resp_dropped_nolistener"] == oc["dropped_nolistener"] > 0
    eng.window_close()
    _compare_window(eng, orc)
    eng.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_adjacent_hosts_end_at_the_batch_end(torch_mod, oracle, form):
    """three such hosts next to each other in one batch: every length of the table as a first, middle and last segment's; the last
    segment ends exactly at the batch's last event, and some batches hold an odd number of events"""
    L, T, TPT = FORMS[form]
    rng = np.random.default_rng(800 + TPT)
    nh = 3
    eng = _engine(max_hosts=4, max_services=nh * 2048, max_batch_events=1 << 17, resp_path=2)
    orc = oracle.OracleEngine(nh * 2048)
    info, _ = helpers.register_world(eng, orc, range(nh), L)
    lens = edge_lengths(T, TPT)
    odd = 0
    for b in range(6):
        hosts = [(b + i) % nh for i in range(nh)]
        n = _run_dev(torch_mod, eng, orc, [helpers.make_resp_events(rng, h, lens[b + 6 * i], L) for i, h in enumerate(hosts)], [info[h][1] for h in hosts])
        odd += n & 1
        _compare_all(eng, orc, oracle)
    assert odd >= 1
    c = eng.counters()
    assert c["resp_batches_general"] == 0 and c["resp_batches_host_local"] == 6
    eng.window_close()
    _compare_window(eng, orc)
    eng.close()


def test_bound_address_host_and_ipv6_batches(torch_mod, oracle):
    """a host whose keys have candidates (the event's server address picks the listener: the MODE 1 instance) and batches of 48-byte IPv6
    events (the MODE 2 instance: the packed slots address 48-byte events), at lengths around a group and a tile of the 1024 x 16 form"""
    from tests.test_gpu_round5 import _compare
    rng = np.random.default_rng(900)
    T, G, TILE = 1024, 4096, 16384
    eng = _engine(max_hosts=2, max_services=256, max_batch_events=1 << 16, resp_path=2)
    orc = oracle.OracleEngine(256)
    w = World(eng, orc, [0], 40)
    mid, slot, _ = w.info[0]
    for n in (T + 1, G + 439, TILE + G + 1, 3 * TILE + 4535):
        _run_dev(torch_mod, eng, orc, [w.events4(rng, 0, n)], [slot])
        _compare(eng, orc)
    for n in (65, G + 439, TILE + 1):
        ev = w.events6(rng, 0, n)
        eng.handle_resp_events_v6(mid, ev)
        orc.resp_batch_v6(ev.tobytes(), [slot], [0])
        eng.sync()
        _compare(eng, orc)
    assert eng.counters()["resp_batches_general"] == 0
    eng.window_close()
    _compare_window(eng, orc)
    eng.close()


def test_split_form_150000_events(torch_mod, oracle):
    """one host with 150 000 events: the split form (parts of 65 536 events = four full tiles; the last part one tile and 2 544 events),
    then the same with one event more (an odd batch)"""
    rng = np.random.default_rng(1000)
    L = 1000
    eng = _engine(max_hosts=2, max_services=2048, max_batch_events=1 << 18, resp_path=3)
    orc = oracle.OracleEngine(2048)
    info, _ = helpers.register_world(eng, orc, [0], L)
    for n in (150_000, 150_001):
        _run_dev(torch_mod, eng, orc, [helpers.make_resp_events(rng, 0, n, L)], [info[0][1]])
        _compare_all(eng, orc, oracle)
    c = eng.counters()
    assert (c["resp_batches_host_split"], c["resp_batches_general"]) == (2, 0)
    eng.window_close()
    _compare_window(eng, orc)
    eng.close()
