"""GPU parity of the event kernel's listener lookup (k_resp_host: two entries of the host's LDS sub-table at once, the copy of entry 0 behind
the last entry, the third-and-later probe walk) on the key sets of tests/lstkeys.py: runs that wrap around the end of 16-, 64- and
4096-entry tables, long runs and the misses that walk them, keys that agree with a stored entry in one 32-bit half of the packed compare,
the all-ones key (the key bits of a free entry) registered and not, full-size tables of both tile forms, a host in two parts, a run
rebuilt after a delete.  Each scenario checks its own witnesses when it is built, so a changed hash or capacity rule fails here with
"scenario no longer reaches its edge".

Every world is one device batch over hosts of different table sizes -- a small table's copy of entry 0 then lies inside a larger LDS area --
through the host-local path (resp_path=2); scenarios A to E again through the general path's global table (resp_path=1) and scenario C's
wrapped run through the split form (resp_path=3); scenario H's keys with candidates under IPv4 and IPv6 events (MODE 1 / 2).  After every batch, against the oracle on the same bytes and exactly: per-service
histograms, bitmaps, digest state, buffered values, the three response counters and the batch-path counters; after window_close the HLL
registers, both Count-Min tables and the all-service histogram."""
import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers, lstkeys
from tests.test_gpu_resp import _compare_all, _compare_window, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _last(*names):
    return [(h, len(h.steps) - 1) for n in names for h in lstkeys.scenario(n).hosts]


# world -> (hosts and the step whose tables and events are used, table sizes that must meet in the launch)
WORLDS = {
    "ABCD": (lambda: _last("A", "C", "B", "D"), {16, 64}),
    "E+C": (lambda: _last("E") + _last("C")[:1], {16, 32, 64}),
    "F.quarter+A": (lambda: [(lstkeys.scenario("F").hosts[0], 0)] + _last("A"), {4096, 16}),
    "F.half+B": (lambda: [(lstkeys.scenario("F").hosts[1], 0)] + _last("B"), {4096, 16}),
    "G+A": (lambda: _last("G") + _last("A"), {4096, 16}),
}


class Net:
    """an engine and the oracle with the same hosts and listeners; host i of the net is synthetic host i"""

    def __init__(self, oracle, resp_path, max_services=8192, max_batch_events=1 << 17):
        self.eng = _engine(max_hosts=8, max_services=max_services, max_batch_events=max_batch_events, resp_path=resp_path)
        self.orc = oracle.OracleEngine(max_services)
        self.oracle = oracle
        self.mids, self.slots, self.batches = [], [], 0

    def host(self):
        self.mids.append(wire.machine_id(len(self.mids)))
        self.slots.append(self.eng.register_host(self.mids[-1], "cluster%d" % (len(self.mids) % 3)))
        return len(self.mids) - 1

    def register(self, i, keys, svcs, bound=None):
        """plain listeners `keys` (service numbers svcs of host i) in the engine and, at the same slots, in the oracle"""
        g = wire.glob_id(np.full(len(svcs), i), np.asarray(svcs))
        ns, pt = np.array([k[0] for k in keys], dtype=np.uint32), np.array([k[1] for k in keys], dtype=np.uint16)
        if bound:  # (listeners bound to an address: one call each, as tests/test_gpu_round5.py registers them)
            for j, k in enumerate(keys):
                a = lstkeys.ADDR[bound[k]] if k in bound else None
                s = self.eng.register_listeners(self.mids[i], [int(g[j])], [k[0]], [k[1]], addrs=[a])
                assert self.orc.register_addr(self.slots[i], int(g[j]), k[0], k[1], a) == s
            return None
        first = self.eng.register_listeners_np(self.mids[i], g, ns, pt)
        for j, k in enumerate(keys):
            assert self.orc.register(self.slots[i], int(g[j]), k[0], k[1]) == first + j
        return first

    def batch(self, torch, hosts_events, v6=False):
        """one device batch, one segment per (host, events); the buffer holds the events and nothing behind them"""
        parts = [lstkeys.to_v6(ev) if v6 else ev for _, ev in hosts_events]
        buf = np.frombuffer(b"".join(p.tobytes() for p in parts), dtype=wire.RESP_EVENT6) if v6 else helpers.concat_events(parts)
        firsts = np.cumsum([0] + [len(x) for x in parts[:-1]])
        segs = (capi.RespSeg * len(parts))()
        for j, (i, _) in enumerate(hosts_events):
            segs[j].host_slot, segs[j].first_event = self.slots[i], int(firsts[j])
        d = torch.from_numpy(buf.view(np.uint8).copy()).cuda()
        (self.eng.handle_resp_events_v6_dev if v6 else self.eng.handle_resp_events_dev)(segs, d.data_ptr(), len(buf))
        self.eng.sync()
        (self.orc.resp_batch_v6 if v6 else self.orc.resp_batch)(buf.tobytes(), [self.slots[i] for i, _ in hosts_events], [int(f) for f in firsts])
        self.batches += 1
        self.check()

    def check(self):
        _compare_all(self.eng, self.orc, self.oracle)
        c, oc = self.eng.counters(), self.orc.counters()
        assert [c["resp_events"], c["resp_dropped_range"], c["resp_dropped_nolistener"]] == [oc["events"], oc["dropped_range"], oc["dropped_nolistener"]]
        assert oc["dropped_nolistener"] > 0 and oc["dropped_range"] > 0
        return c

    def paths(self):
        c = self.eng.counters()
        return c["resp_batches_host_local"], c["resp_batches_general"], c["resp_batches_host_split"]

    def finish(self):
        self.eng.window_close()
        _compare_window(self.eng, self.orc)
        helpers.assert_hist_equal(self.eng.export_hist(1, 0, self.orc.nsvc), self.orc.hist(), self.orc.nsvc)
        self.eng.close()


def _run_world(torch, oracle, name, resp_path):
    hosts, sizes = WORLDS[name][0](), WORLDS[name][1]
    assert sizes <= {len(t[0]) for h, s in hosts for t in h.steps[s].tables}
    net = Net(oracle, resp_path)
    batch = []
    for h, s in hosts:
        i = net.host()
        st = h.steps[s]
        assert s == 0 and st.kind == "reg"
        net.register(i, st.keys, st.svcs)
        batch.append((i, st.events))
    # every listener gets events: a hit booked to a colliding listener would change two services' records
    net.batch(torch, batch)
    assert (net.eng.export_hist(0, 0, net.orc.nsvc)[:, 15, 0] >= 3).all()
    return net


@pytest.mark.parametrize("name", list(WORLDS))
def test_lookup_scenarios_host_local(torch_mod, oracle, name):
    """each world as one device batch through k_resp_host"""
    net = _run_world(torch_mod, oracle, name, 2)
    assert net.paths() == (1, 0, 0)
    net.finish()


@pytest.mark.parametrize("name", ["ABCD", "E+C"])
def test_lookup_scenarios_general_path(torch_mod, oracle, name):
    """scenarios A to E through the general path: the global table gives the same answers"""
    net = _run_world(torch_mod, oracle, name, 1)
    assert net.paths() == (0, 1, 0)
    net.finish()


def test_all_ones_key_registers(torch_mod, oracle):
    """(0xFFFFFFFF, 0xFFFF) is a key like any other to gys_register_listeners: E.own's listener on it gets its events (host-local and
    general), and on the hosts that do not have it the event is dropped as "no listener", as the oracle counts it"""
    e = lstkeys.scenario("E")
    own, bare = e.hosts[2], e.hosts[0]
    assert lstkeys.ALL_ONES in own.steps[0].keys and lstkeys.ALL_ONES in bare.steps[0].misses
    for resp_path in (2, 1):
        net = _run_world(torch_mod, oracle, "E+C", resp_path)
        svc = own.steps[0].svcs[own.steps[0].keys.index(lstkeys.ALL_ONES)]
        slot = net.eng.lookup(int(wire.glob_id(2, svc)))
        want = 4 if svc % 4 == 0 else 3
        assert net.eng.export_hist(0, 0, net.orc.nsvc)[slot, 15, 0] == want == net.orc.hist()[slot, 15, 0]
        net.finish()


@pytest.mark.parametrize("resp_path", [2, 1], ids=["hostlocal", "general"])
def test_keys_with_candidates_among_the_displaced(torch_mod, oracle, resp_path):
    """scenario H next to scenario C's 64-entry hosts: entries that name candidate records in entry 0 behind home mask and where only the
    walk reaches them; the event's server address picks the listener or nobody.  IPv4 events (the MODE 1 instance), then the same traffic
    as 48-byte IPv6 events with ::ffff: addresses (MODE 2) against the same tables"""
    hosts = _last("H", "C")
    net = Net(oracle, resp_path, max_services=256)
    batch = []
    for h, s in hosts:
        st = h.steps[s]
        i = net.host()
        net.register(i, st.keys, st.svcs, st.bound)
        batch.append((i, st.events))
    assert hosts[0][0].steps[0].cands and net.orc.nsvc == sum(len(h.steps[s].keys) for h, s in hosts)
    net.batch(torch_mod, batch)
    n4 = net.eng.export_hist(0, 0, net.orc.nsvc)[:, 15, 0].copy()
    assert (n4 >= 3).all()
    net.batch(torch_mod, batch[::-1], v6=True)
    assert (net.eng.export_hist(0, 0, net.orc.nsvc)[:, 15, 0] == 2 * n4).all()
    assert net.paths() == ((2, 0, 0) if resp_path == 2 else (0, 2, 0))
    net.finish()


def test_wrapped_run_through_the_split_form(torch_mod, oracle):
    """scenario C's run through the table's end under resp_path=3: one segment of 65 537 events cycling over the same keys is cut in two"""
    net = Net(oracle, 3, max_services=64, max_batch_events=1 << 17)
    h = lstkeys.scenario("C").hosts[1]
    st = h.steps[0]
    i = net.host()
    net.register(i, st.keys, st.svcs)
    net.batch(torch_mod, [(i, lstkeys.cycle_events(st.events, 65537))])
    assert net.paths() == (0, 0, 1)
    net.finish()


def test_run_after_a_delete(torch_mod, oracle):
    """scenario I: three listeners leave the head, the middle and the tail of a run through the table's end (gys_delete_listeners rebuilds the
    table without holes): their events are misses, the survivors still hit; then two new listeners of the same home take the lowest free
    slots and the check repeats.  The oracle has no delete: it never has the three keys on this host -- the slots the engine will reuse
    hold the two later listeners from the start (their events come only after the engine has them too), the third a key of a host that
    gets no events -- and nothing is ingested before the delete, so every export still has to agree slot for slot."""
    torch = torch_mod
    sc = lstkeys.scenario("I")
    h = sc.hosts[0]
    reg, dele, add = h.steps
    b = lstkeys.scenario("B").hosts[0]
    net = Net(oracle, 2, max_services=64, max_batch_events=1 << 16)
    x, y, idle = net.host(), net.host(), net.host()
    g = wire.glob_id(np.full(len(reg.svcs), x), np.asarray(reg.svcs))
    first = net.eng.register_listeners_np(net.mids[x], g, np.array([k[0] for k in reg.keys], dtype=np.uint32), np.array([k[1] for k in reg.keys], dtype=np.uint16))
    assert first == 0
    reuse = dict(zip(sorted(dele.svcs), add.keys))  # deleted service number == its slot -> the listener that takes the slot later
    g_add = wire.glob_id(np.full(len(add.svcs), x), np.asarray(add.svcs))
    for s, k in zip(reg.svcs, reg.keys):
        if s not in dele.svcs:
            assert net.orc.register(net.slots[x], int(g[s]), k[0], k[1]) == s
        elif s in reuse:
            assert net.orc.register(net.slots[x], int(g_add[add.keys.index(reuse[s])]), reuse[s][0], reuse[s][1]) == s
        else:
            assert net.orc.register(net.slots[idle], int(g[s]), k[0], k[1]) == s
    net.register(y, b.steps[0].keys, b.steps[0].svcs)
    assert net.eng.delete_listeners(g[dele.svcs]) == 3
    assert not set(add.keys) & {(int(n), int(p)) for n, p in zip(dele.events["netns"], dele.events["sport_be"])}
    net.batch(torch, [(x, dele.events), (y, b.steps[0].events)])
    hist = net.eng.export_hist(0, 0, net.orc.nsvc)
    assert (hist[dele.svcs, 15, 0] == 0).all() and (hist[dele.live, 15, 0] >= 3).all()
    slots = net.eng.register_listeners_slots(net.mids[x], g_add, [k[0] for k in add.keys], [k[1] for k in add.keys])
    assert slots.tolist() == sorted(dele.svcs)[:2]
    net.batch(torch, [(y, b.steps[0].events), (x, add.events)])
    hist = net.eng.export_hist(0, 0, net.orc.nsvc)
    assert (hist[slots, 15, 0] >= 3).all() and hist[sorted(dele.svcs)[2], 15, 0] == 0
    assert net.paths() == (2, 0, 0)
    net.finish()
