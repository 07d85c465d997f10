"""Listener key sets that drive the event kernel's lookup (k_resp_host, gys_kernels.hpp) to the edges of a host's open-addressing sub-table.

A Python restatement of host_tbl_hash / host_tbl_slot / host_tbl_part (gys_device.hpp), host_tbl_capacity and the insertion order of
host_tbl_insert / host_lst_repartition / host_lst_remove + host_rebuild (gys_hostlst.hpp) for plain listeners (one any-address listener per
(netns, port) key), a search over ports x a few name spaces for keys with a wanted home entry, and on top of both the scenarios A .. G and
I of the lookup tests: small tables whose runs wrap, long runs, near-miss keys, the all-ones key, full-size tables, a host in two parts, a
run after a delete.  Every scenario is built from a fixed seed, carries its listeners in registration order, its events, the predicted
tables and a list of WITNESSES -- statements about what the kernel's lookup meets on these keys ("hit through the copy of entry 0", "the
walk crosses the table's end") -- which the builder checks itself: a change of the hash or of the capacity rule fails with "scenario no
longer reaches its edge" instead of quietly testing less.

The restatement is pinned entry for entry to the C++ mirror by tests/test_hostlst_cpu.py; tests/test_kernel_logic_resp_lookup_cpu.py runs
the kernel on the scenarios under the CPU stand-in and tests/test_gpu_resp_lookup.py on the GPU."""
import numpy as np

from gyeeta_amd import wire

M32 = 0xFFFFFFFF
EMPTY = (1 << 64) - 1
MAX_LOCAL = 2048  # GYS_HOST_MAX_LOCAL
SPARSE = 4096     # GYS_HOST_TBL_SPARSE
ALL_ONES = (0xFFFFFFFF, 0xFFFF)  # (key48 << 16) >> 16 of a free entry
LOCAL_GROUP = 0x8000             # GYS_LOCAL_GROUP: the entry's low 15 bits index the host's candidate records
ADDR = {1: bytes([10, 0, 0, 1]), 2: bytes([10, 0, 0, 2]), 3: bytes([10, 0, 0, 3])}  # address kinds of tests/cpp/test_hostlst.cc; 0: any address
NOBODY = bytes([10, 9, 9, 9])


class ScenarioError(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------- the mirror, restated
def tbl_hash(netns, port):
    """host_tbl_hash; python ints or uint64 arrays"""
    x = (netns ^ ((port & 0xFFFF) * 0x9E3779)) & M32
    x = x ^ (x >> 16)
    return (x * 0x85EBCA6B) & M32


def tbl_slot(hk, mask):
    return (hk ^ (hk >> 13)) & mask


def tbl_part(hk, pmask):
    return (hk >> 21) & pmask


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def capacity(n):
    """host_tbl_capacity"""
    c4 = next_pow2(max(16, 4 * n))
    return c4 if c4 <= SPARSE else max(SPARSE, next_pow2(max(16, 2 * n)))


def key48(netns, port):
    return (netns << 16) | port


def home(key, cap):
    return int(tbl_slot(tbl_hash(key[0], key[1]), cap - 1))


class SubTable:
    def __init__(self, entries=0):
        self.tbl = [EMPTY] * entries
        self.keys = []   # local index -> (netns, port)
        self.slots = []  # local index -> service number

    def put(self, key, local):
        mask = len(self.tbl) - 1
        h = home(key, len(self.tbl))
        while self.tbl[h] != EMPTY:
            h = (h + 1) & mask
        self.tbl[h] = (key48(*key) << 16) | local

    def insert(self, key, slot):
        """host_tbl_insert: the table grows to the capacity of its locals and is rehashed in local-index order"""
        self.keys.append(key)
        self.slots.append(slot)
        if capacity(len(self.slots)) > len(self.tbl):
            self.tbl = [EMPTY] * capacity(len(self.slots))
            for l, k in enumerate(self.keys):
                self.put(k, l)
        else:
            self.put(key, len(self.slots) - 1)


class HostMirror:
    """HostListeners for plain listeners: one table (16 free entries at first), or 2, 4, .. parts once a table would pass MAX_LOCAL locals"""

    def __init__(self):
        self.one = SubTable(16)
        self.sub = []
        self.group = {}  # key -> address kind of its one bound listener (a key with candidates)
        self.cands = []  # candidate records (ip32, flags, local, service number)

    def parts(self):
        return self.sub if self.sub else [self.one]

    def table_of(self, key):
        return self.sub[int(tbl_part(tbl_hash(*key), len(self.sub) - 1))] if self.sub else self.one

    def register(self, keys, slots, bound=None):
        for key, slot in zip(keys, slots):
            assert all(key not in t.keys for t in self.parts()), "one listener per key"
            if bound and key in bound:
                self.group[key] = bound[key]
            while len(self.table_of(key).slots) >= MAX_LOCAL:  # host_new_local -> host_lst_repartition
                every = [(k, s) for t in self.parts() for k, s in zip(t.keys, t.slots)]
                self.sub = [SubTable() for _ in range(2 * len(self.sub) if self.sub else 2)]
                assert len(self.sub) <= 16
                for k, s in every:
                    self.table_of(k).insert(k, s)
                for t in self.sub:
                    if not t.tbl:
                        t.tbl = [EMPTY] * 16
            self.table_of(key).insert(key, slot)
        if self.group:
            self.rebuild()

    def rebuild(self):
        """host_rebuild: the entry of a key with candidates names the first record of its chain, made when its first local comes by"""
        assert not self.sub or not self.group
        self.cands = []
        for t in self.parts():
            t.tbl = [EMPTY] * max(len(t.tbl), capacity(len(t.slots)))
            for l, k in enumerate(t.keys):
                if k in self.group:
                    t.put(k, LOCAL_GROUP | len(self.cands))
                    self.cands.append((int.from_bytes(ADDR[self.group[k]], "little"), 2, l, t.slots[l]))  # (flags: not any-address, last of its key)
                else:
                    t.put(k, l)

    def remove(self, dead):
        """host_lst_remove + the rebuild of the next flush: the survivors close up, hole-free tables"""
        dead = set(dead)
        for t in self.parts():
            keep = [i for i, s in enumerate(t.slots) if s not in dead]
            t.keys, t.slots = [t.keys[i] for i in keep], [t.slots[i] for i in keep]
        self.rebuild()

    def snapshot(self):
        return [(list(t.tbl), list(t.slots)) for t in self.parts()]


def probe(tbl, key):
    """k_resp_host's lookup of `key` in one sub-table, step by step: entries h and h + 1 at once (entry mask + 1 is the copy of entry 0), each
    compared in two 32-bit halves, then the walk from (h + 2) & mask that an empty entry ends."""
    netns, port = key
    mask = len(tbl) - 1
    h = home(key, len(tbl))
    a, b = tbl[h], tbl[h + 1] if h < mask else tbl[0]
    half = lambda e: ((e >> 32) == netns, (((e & M32) ^ (port << 16)) & M32) < 0xFFFF)
    r = dict(home=h, a=half(a), b=half(b), a_empty=a == EMPTY, where=None, entry=None, local=None, via_copy=False, walk_start=None, walk=0,
             crossed=False, wrap_in_step=False)
    if all(r["a"]):
        r.update(where="a", entry=h, local=a & 0xFFFF)
    elif all(r["b"]):
        r.update(where="b", entry=(h + 1) & mask, local=b & 0xFFFF, via_copy=h == mask)
    else:
        i = (h + 2) & mask
        r.update(walk_start=i, wrap_in_step=h + 2 > mask)
        for _ in range(2, mask + 1):
            e = tbl[i]
            if e == EMPTY:
                break
            r["walk"] += 1  # used entries the walk reads
            if (e >> 16) == key48(netns, port):
                r.update(where="walk", entry=i, local=e & 0xFFFF)
                break
            if i == mask:
                r["crossed"] = True
            i = (i + 1) & mask
    return r


def used(tbl):
    return {i for i, e in enumerate(tbl) if e != EMPTY}


def run_through_end(tbl):
    """length of the run of used entries that holds both the last entry and entry 0 (0: there is none)"""
    n = len(tbl)
    if tbl[n - 1] == EMPTY or tbl[0] == EMPTY:
        return 0
    back = next(d for d in range(n) if tbl[n - 1 - d] == EMPTY)
    fwd = next(d for d in range(n) if tbl[d] == EMPTY)
    return back + fwd


# ---------------------------------------------------------------------------------------------- search
class Search:
    """keys by home entry: ports 1 .. 65535 of a few name spaces, picked in an order drawn from the scenario's seed"""

    def __init__(self, rng, netns):
        self.rng, self.netns, self.taken = rng, list(netns), set()
        self.ports = np.arange(1, 65536, dtype=np.uint64)

    def find(self, cap, want_home, count=1, pmask=0, part=0, why=""):
        out = []
        for ns in self.netns:
            hk = tbl_hash(np.uint64(ns), self.ports)
            ok = (tbl_slot(hk, np.uint64(cap - 1)) == np.uint64(want_home)) & (tbl_part(hk, np.uint64(pmask)) == np.uint64(part))
            out += [(ns, int(p)) for p in self.ports[ok]]
        out = [k for k in out if k not in self.taken]
        if len(out) < count:
            raise ScenarioError("scenario no longer reaches its edge: %d keys of home %d in %d entries wanted (%s), %d found" % (count, want_home, cap, why, len(out)))
        pick = [out[i] for i in self.rng.permutation(len(out))[:count]]
        self.taken.update(pick)
        return pick


# ---------------------------------------------------------------------------------------------- events
def latency(s):
    """response time (ms) of the events of a host's service number s: a hit booked to the wrong listener changes two services' records"""
    return 999999 if s % 13 == 5 else 7 + 3 * s


def make_events(rng, hidx, hits, misses, bound=None):
    """RESP_EVENT records: `hits` = [((netns, port), service number)] get 3 or 4 events each at the service's latency, `misses` =
    [(netns, port)] 3 each; two events outside the latency range (one on a listener's key, one on a miss key); a few 0.0.0.0 clients; shuffled"""
    rows = []
    for key, s in hits:
        rows += [(key, latency(s))] * (4 if s % 4 == 0 else 3)
    for i, key in enumerate(misses):
        rows += [(key, 50 + i)] * 3
    own = bytes([10, 7, hidx & 255, 1])
    addr = [ADDR[bound[k]] if bound and k in bound else own for k, _ in rows]
    for i, key in enumerate(bound or ()):  # a bound listener's key with a server address that matches no candidate: nobody's event
        rows += [(key, 70 + i)] * 3
        addr += [NOBODY, own, NOBODY]
    for key in ([hits[0][0]] if hits else []) + ([misses[0]] if misses else []):
        rows.append((key, 1000001 + len(rows)))
        addr.append(ADDR[bound[key]] if bound and key in bound else own)
    n = len(rows)
    order = rng.permutation(n)
    ev = np.zeros(n, dtype=wire.RESP_EVENT)
    ev["netns"] = np.array([rows[i][0][0] for i in order], dtype=np.uint32)
    ev["sport_be"] = np.array([rows[i][0][1] for i in order], dtype=np.uint16)
    lat = np.array([rows[i][1] for i in order], dtype=np.uint32)
    ev["saddr"] = np.array([int.from_bytes(addr[i], "little") for i in order], dtype=np.uint32)
    ev["daddr"] = np.where(rng.random(n) < 0.01, 0, (0x0B000000 | rng.integers(1, 1 << 20, n)).astype(">u4").view("<u4"))
    ev["dport_be"] = rng.integers(16000, 65536, n)
    lrcv = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore"):
        ev["lsndtime"] = lrcv + lat
    ev["lrcvtime"] = lrcv
    return ev


def cycle_events(ev, n):
    """n events cycling over the records of `ev` (the split form needs one long segment over the same keys)"""
    return np.frombuffer((ev.tobytes() * (n // len(ev) + 1))[:n * ev.itemsize], dtype=ev.dtype)


# ---------------------------------------------------------------------------------------------- scenarios
class Step:
    """one registry call of a host and what follows it: kind "reg" (keys = the new listeners, service numbers `svcs`) or "del" (svcs = the
    deleted services); `events` are sent afterwards (None: nothing); `tables` = the predicted [(entries, local -> service number)] per part
    and `live` = the services registered then, in registration order; `bound` = {key: address kind} of the keys with candidates and
    `cands` their predicted records (ip32, flags, local, service number)"""

    def __init__(self, kind, keys, svcs):
        self.kind, self.keys, self.svcs = kind, keys, svcs
        self.events, self.misses, self.tables, self.live = None, [], None, None


class Host:
    def __init__(self, name):
        self.name, self.steps, self.mirror, self.key_of, self.nsvc = name, [], HostMirror(), {}, 0

    def reg(self, keys, bound=None):
        """bound: {key: address kind (ADDR)} of the listeners bound to an address; the others are any-address listeners"""
        svcs = list(range(self.nsvc, self.nsvc + len(keys)))
        self.nsvc += len(keys)
        self.mirror.register(keys, svcs, bound)
        self.key_of.update(zip(svcs, keys))
        return self._step(Step("reg", list(keys), svcs))

    def delete(self, svcs):
        self.mirror.remove(svcs)
        st = Step("del", [self.key_of.pop(s) for s in svcs], list(svcs))
        return self._step(st)

    def _step(self, st):
        st.tables = self.mirror.snapshot()
        st.bound, st.cands = dict(self.mirror.group), list(self.mirror.cands)
        st.live = sorted(self.key_of)
        st.live_keys = [self.key_of[s] for s in st.live]
        self.steps.append(st)
        return st

    def send(self, rng, hidx, misses):
        """events for every live key and for `misses` behind the latest step"""
        st = self.steps[-1]
        st.misses = list(misses)
        st.events = make_events(rng, hidx, [(self.key_of[s], s) for s in st.live], misses, st.bound)
        return st

    def table_of(self, key, step=-1):
        t = self.steps[step].tables
        return t[int(tbl_part(tbl_hash(*key), len(t) - 1))][0]

    def probe(self, key, step=-1):
        return probe(self.table_of(key, step), key)


class Scenario:
    def __init__(self, name, seed):
        self.name, self.hosts, self.witnesses = name, [], []
        self.rng = np.random.default_rng([seed, sum(name.encode())])
        self.search = Search(self.rng, [0xC0DE0000 + 0x100 * sum(name.encode()) + j for j in range(3)])

    def host(self, suffix=""):
        self.hosts.append(Host(self.name + suffix))
        return self.hosts[-1]

    def witness(self, text, cond):
        self.witnesses.append((text, bool(cond)))

    def check(self):
        bad = [t for t, ok in self.witnesses if not ok]
        if bad:
            raise ScenarioError("scenario %s no longer reaches its edge: %s" % (self.name, "; ".join(bad)))
        for h in self.hosts:  # what every scenario promises: the prediction resolves every event as the registry says
            for i, st in enumerate(h.steps):
                if st.events is None:
                    continue
                for s, k in zip(st.live, st.live_keys):
                    r = h.probe(k, i)
                    t = st.tables[int(tbl_part(tbl_hash(*k), len(st.tables) - 1))]
                    if r["where"] is not None and r["local"] & LOCAL_GROUP:
                        if k not in st.bound or st.cands[r["local"] & (LOCAL_GROUP - 1)][2:] != (t[1].index(s), s):
                            raise ScenarioError("scenario %s: the candidate record of %r in %s" % (self.name, k, h.name))
                    elif r["where"] is None or k in st.bound or t[1][r["local"]] != s:
                        raise ScenarioError("scenario %s: the predicted table of %s does not resolve %r" % (self.name, h.name, k))
                for k in st.misses:
                    if h.probe(k, i)["where"] is not None:
                        raise ScenarioError("scenario %s: miss key %r of %s is registered" % (self.name, k, h.name))
        return self


def _small_wrap(name, seed, first_home, entries):
    """A / B: four listeners of one home at the end of a 16-entry table"""
    sc = Scenario(name, seed)
    h = sc.host()
    keys = sc.search.find(16, first_home, 4, why="the run")
    h.reg(keys)
    miss = sc.search.find(16, first_home, 1, why="miss of the run's home") + sc.search.find(16, entries[-1] + 1, 1, why="miss behind the run") + sc.search.find(16, 8, 1, why="miss far from the run")
    h.send(sc.rng, len(name), miss)
    tbl = h.steps[-1].tables[0][0]
    sc.witness("16 entries, the run fills %s" % entries, len(tbl) == 16 and used(tbl) == set(entries))
    p = [h.probe(k) for k in keys]
    sc.witness("the first key sits in its home entry", p[0]["where"] == "a" and p[0]["entry"] == first_home)
    if first_home == 15:
        sc.witness("a hit in the home entry at mask", p[0]["entry"] == 15)
        sc.witness("a hit through the copy of entry 0", p[1]["where"] == "b" and p[1]["via_copy"] and p[1]["entry"] == 0)
        sc.witness("walks that begin at entry 1", all(q["where"] == "walk" and q["walk_start"] == 1 for q in p[2:]))
    else:
        sc.witness("a hit in entry mask as the second entry", p[1]["where"] == "b" and p[1]["entry"] == 15 and not p[1]["via_copy"])
        sc.witness("walks that begin at entry 0 (the wrap is in + 2)", all(q["where"] == "walk" and q["walk_start"] == 0 and q["wrap_in_step"] for q in p[2:]))
    m = h.probe(miss[0])
    sc.witness("a miss walks the wrapped run to its end", m["where"] is None and m["walk"] == 2 and m["walk_start"] == (first_home + 2) & 15)
    sc.witness("a miss whose home is the first free entry", h.probe(miss[1])["a_empty"])
    return sc.check()


def scenario_a(seed=20260):
    return _small_wrap("A", seed, 15, [15, 0, 1, 2])


def scenario_b(seed=20260):
    return _small_wrap("B", seed, 14, [14, 15, 0, 1])


def scenario_c(seed=20260):
    """64 entries: sixteen listeners of one home in mid-table (C.mid), twelve of home 60 (C.end: entries 60 .. 63 and 0 .. 7)"""
    sc = Scenario("C", seed)
    mid = sc.host(".mid")
    keys = sc.search.find(64, 20, 16, why="mid-table run")
    mid.reg(keys)
    miss = [sc.search.find(64, x, 1, why="miss of home %d" % x)[0] for x in (20, 27, 35, 36)]
    mid.send(sc.rng, 1, miss)
    tbl = mid.steps[-1].tables[0][0]
    sc.witness("C.mid: displacements 0 to 15", len(tbl) == 64 and [mid.probe(k)["entry"] for k in keys] == list(range(20, 36)))
    sc.witness("C.mid: the last key's walk reads 14 entries", mid.probe(keys[15])["walk"] == 14)
    sc.witness("C.mid: a miss of the run's home walks all of it", mid.probe(miss[0])["walk"] == 14 and mid.probe(miss[0])["where"] is None)
    sc.witness("C.mid: a miss that starts inside the run", mid.probe(miss[1])["walk"] == 7)
    sc.witness("C.mid: a miss whose home is the first free entry behind the run", mid.probe(miss[3])["a_empty"] and mid.probe(miss[2])["walk"] == 0)
    end = sc.host(".end")
    keys = sc.search.find(64, 60, 12, why="run through the end")
    end.reg(keys)
    miss = [sc.search.find(64, x, 1, why="miss of home %d" % x)[0] for x in (60, 62, 63, 0, 3, 8)]
    end.send(sc.rng, 2, miss)
    tbl = end.steps[-1].tables[0][0]
    m = [end.probe(k) for k in miss]
    sc.witness("C.end: entries 60 to 63 and 0 to 7", len(tbl) == 64 and used(tbl) == {60, 61, 62, 63, 0, 1, 2, 3, 4, 5, 6, 7})
    sc.witness("C.end: hits behind the end are found by walks that cross it", all(end.probe(k)["crossed"] for k in keys[5:]))
    sc.witness("C.end: the miss of the run's home walks 10 entries and crosses the end", m[0]["walk"] == 10 and m[0]["crossed"] and m[0]["where"] is None)
    sc.witness("C.end: the miss of home 62 walks 8 entries from entry 0 (the wrap is in + 2)", m[1]["walk"] == 8 and m[1]["wrap_in_step"] and m[1]["walk_start"] == 0)
    sc.witness("C.end: the miss of home 63 reads the copy of entry 0 and walks from entry 1", m[2]["home"] == 63 and m[2]["walk_start"] == 1 and m[2]["walk"] == 7)
    sc.witness("C.end: misses of homes 0 and 3 start inside the run", m[3]["walk"] == 6 and m[4]["walk"] == 3 and not m[3]["crossed"])
    sc.witness("C.end: a miss whose home is the first free entry behind the run", m[5]["a_empty"] and m[5]["walk"] == 0)
    return sc.check()


NEAR = (lambda n, p: (n, p ^ 1), lambda n, p: (n, p ^ 0x8000), lambda n, p: (n ^ 1, p), lambda n, p: (n ^ 0x80000000, p), lambda n, p: (n ^ 0x00010000, p))
NEAR_NAMES = ("port ^ 1", "port ^ 0x8000", "netns ^ 1", "netns ^ 0x80000000", "netns ^ 0x00010000")


def scenario_d(seed=20260):
    """near-miss keys in 64 entries: for every variant v of NEAR a registered key K whose variant's home is K's entry (the variant meets K as
    entry a) and one whose variant's home is the entry before (as entry b); five of the variants are listeners themselves"""
    sc = Scenario("D", seed)
    h = sc.host()
    ports = np.arange(1, 65535, dtype=np.uint64)
    chosen, homes = [], []
    for v, near in enumerate(NEAR):
        for pos in (0, 1):
            found = None
            for ns in sc.search.netns:
                vn, vp = near(ns, ports)
                hk, hv = tbl_slot(tbl_hash(np.uint64(ns), ports), np.uint64(63)), tbl_slot(tbl_hash(np.uint64(vn) if np.isscalar(vn) else vn, vp), np.uint64(63))
                for i in sc.rng.permutation(np.nonzero(hv + np.uint64(pos) == hk)[0]):
                    hm = int(hk[i])
                    if 2 <= hm < 60 and all(abs(hm - x) >= 3 for x in homes):
                        found = (ns, int(ports[i]))
                        break
                if found:
                    break
            if not found:  # (no key does that under this hash -- netns ^ 0x80000000 always moves the home by 4 or more: any key then, no place promised)
                free = next(x for x in range(2, 60) if all(abs(x - y) >= 3 for y in homes))
                found, pos = sc.search.find(64, free, 1, why="near-miss key")[0], None
            chosen.append((found, v, pos))
            homes.append(home(found, 64))
    keys = [c[0] for c in chosen]
    regd = [NEAR[(v + 1) % 5](*k) for k, v, pos in chosen[::2]]  # listeners among the variants: another variant of five of the keys
    h.reg(keys + regd)
    live = set(keys + regd)
    miss = sorted({near(*k) for k in keys for near in NEAR} - live)
    h.send(sc.rng, 4, miss)
    tbl = h.steps[-1].tables[0][0]
    sc.witness("D: 15 listeners in 64 entries", len(tbl) == 64 and len(live) == 15)
    seen = set()
    for (k, v, pos) in chosen:
        if pos is None:
            continue
        r = h.probe(NEAR[v](*k))
        if r["ab"[pos]] == ((True, False) if v < 2 else (False, True)) and r["where"] is None and h.probe(k)["where"] == "a":
            seen.add(("netns" if v < 2 else "port", "ab"[pos]))
            sc.witness("D: the %s variant of %r meets it as entry %s with only the %s half equal" % (NEAR_NAMES[v], k, "ab"[pos], "netns" if v < 2 else "port"), True)
    for half in ("netns", "port"):
        for pos in "ab":
            sc.witness("D: only the %s half of the packed compare agrees in entry %s, at least once" % (half, pos), (half, pos) in seen)
    sc.witness("D: at least six variants meet their key in entry a or b", len([t for t, ok in sc.witnesses if "variant of" in t]) >= 6)
    return sc.check()


def scenario_e(seed=20260):
    """the all-ones key (0xFFFFFFFF, 0xFFFF) = what a free entry holds in its key bits: unregistered on a host without (E.bare) and with
    (E.run) a run at its home; its neighbours registered on E.run and unregistered on E.bare; the key itself registered on E.own, displaced
    into the walk"""
    sc = Scenario("E", seed)
    n1, n2 = (0xFFFFFFFF, 0xFFFE), (0xFFFFFFFE, 0xFFFF)
    bare = sc.host(".bare")
    keys = sc.search.find(16, (home(ALL_ONES, 16) + 5) & 15, 2, why="listeners away from the all-ones home") + sc.search.find(16, (home(ALL_ONES, 16) + 9) & 15, 2, why="listeners")
    bare.reg(keys)
    bare.send(sc.rng, 5, [ALL_ONES, n1, n2])
    r = bare.probe(ALL_ONES)
    sc.witness("E.bare: the all-ones key's home and the two entries behind it are free", r["a_empty"] and r["walk"] == 0 and bare.table_of(ALL_ONES)[r["walk_start"]] == EMPTY)
    run = sc.host(".run")
    keys = sc.search.find(32, home(ALL_ONES, 32), 4, why="run at the all-ones home")
    run.reg(keys + [n1, n2])
    run.send(sc.rng, 6, [ALL_ONES])
    r = run.probe(ALL_ONES)
    sc.witness("E.run: 32 entries; the all-ones key walks a run to a free entry", len(run.table_of(ALL_ONES)) == 32 and r["walk"] >= 2 and r["where"] is None)
    own = sc.host(".own")
    keys = sc.search.find(16, home(ALL_ONES, 16), 2, why="run at the all-ones home")
    own.reg(keys + [ALL_ONES])
    own.send(sc.rng, 7, [n1, n2])
    sc.witness("E.own: the registered all-ones key is found by the walk", own.probe(ALL_ONES)["where"] == "walk")
    return sc.check()


def _usual(hidx, n):
    s = np.arange(n)
    return list(zip(wire.listener_netns(hidx, s).tolist(), wire.listener_port(s).tolist()))


def _end_run(sc, h, cap, pmask=0, part=0):
    """searched keys that make a run through the end of a `cap`-entry table: 5 of home cap - 5, 2 of the last entry, 4 of home cap - 3"""
    f = lambda hm, n: sc.search.find(cap, hm, n, pmask, part, why="run through the end of %d entries" % cap)
    return f(cap - 5, 5) + f(cap - 1, 2) + f(cap - 3, 4)


def _end_run_witnesses(sc, h, tag, special, miss, tbl):
    sc.witness("%s: a run of at least 8 crosses the end" % tag, run_through_end(tbl) >= 8)
    q, q1 = h.probe(special[5]), h.probe(special[6])
    sc.witness("%s: a key of the last home lies in entry 0, found through the copy" % tag, q["home"] == len(tbl) - 1 and q["entry"] == 0 and q["via_copy"])
    sc.witness("%s: another one is found by a walk that begins at entry 1" % tag, q1["home"] == len(tbl) - 1 and q1["where"] == "walk" and q1["walk_start"] == 1)
    m = [h.probe(k) for k in miss]
    sc.witness("%s: a miss of the run's home walks at least 8 entries across the end" % tag, m[0]["where"] is None and m[0]["walk"] >= 8 and m[0]["crossed"])
    sc.witness("%s: misses that start inside the run on either side of the end" % tag, m[1]["walk"] >= 4 and m[1]["wrap_in_step"] and m[2]["walk"] >= 2 and m[2]["home"] == 0)


def scenario_f(seed=20260):
    """full-size tables: 1000 listeners (4096 entries a quarter full, the 1024 x 16 tile form) and 2048 (half full, 1024 x 8): the usual
    consecutive ports behind eleven searched keys that put a run through the table's end"""
    sc = Scenario("F", seed)
    for suffix, n, hidx in ((".quarter", 1000, 0), (".half", 2048, 1)):
        h = sc.host(suffix)
        special = _end_run(sc, h, 4096)
        h.reg(special + _usual(hidx, n - len(special)))
        miss = [sc.search.find(4096, x, 1, why="miss of home %d" % x)[0] for x in (4091, 4094, 0)] + [(0xF0000000 + 4 * hidx, 999)]
        h.send(sc.rng, 8 + hidx, miss)
        tbl = h.steps[-1].tables[0][0]
        sc.witness("F%s: %d listeners in one table of 4096 entries" % (suffix, n), len(h.steps[-1].tables) == 1 and len(tbl) == 4096 and len(used(tbl)) == n)
        _end_run_witnesses(sc, h, "F" + suffix, special, miss, tbl)
    return sc.check()


def scenario_g(seed=20260):
    """a host in two parts (2100 listeners): searched keys of part 1 make a wrapped run in its table; misses hash to either part"""
    sc = Scenario("G", seed)
    h = sc.host()
    special = _end_run(sc, h, 4096, 1, 1)
    h.reg(special + _usual(3, 2100 - len(special)))
    miss = [sc.search.find(4096, x, 1, 1, 1, why="part 1 miss of home %d" % x)[0] for x in (4091, 4094, 0)] + sc.search.find(4096, 100, 2, 1, 0, why="part 0 miss") + sc.search.find(4096, 200, 1, 1, 1, why="part 1 miss")
    h.send(sc.rng, 10, miss)
    t = h.steps[-1].tables
    sc.witness("G: two parts of 4096 entries, 2100 listeners", len(t) == 2 and [len(x[0]) for x in t] == [4096, 4096] and sum(len(x[1]) for x in t) == 2100)
    sc.witness("G: the searched keys and three misses belong to part 1, two misses to part 0",
               all(tbl_part(tbl_hash(*k), 1) == 1 for k in special + miss[:3] + miss[5:]) and all(tbl_part(tbl_hash(*k), 1) == 0 for k in miss[3:5]))
    if len(t) == 2:
        _end_run_witnesses(sc, h, "G part 1", special, miss, t[1][0])
    return sc.check()


def scenario_i(seed=20260):
    """after a delete: scenario C's run through the end loses its head, a middle key and its tail (the table is rebuilt without holes), then
    two new listeners of the same home go in"""
    sc = Scenario("I", seed)
    h = sc.host()
    keys = sc.search.find(64, 60, 12, why="run through the end")
    h.reg(keys)
    gone = [0, 5, 11]
    h.delete(gone)
    miss = [keys[s] for s in gone] + sc.search.find(64, 60, 1, why="miss of the run's home")
    h.send(sc.rng, 11, miss)
    tbl = h.steps[-1].tables[0][0]
    sc.witness("I: the nine survivors close up in 64 entries: 60 to 63 and 0 to 4", len(tbl) == 64 and used(tbl) == {60, 61, 62, 63, 0, 1, 2, 3, 4})
    sc.witness("I: the deleted keys walk the rebuilt run across the end and miss", all(h.probe(keys[s])["where"] is None and h.probe(keys[s])["crossed"] for s in gone))
    sc.witness("I: survivors behind the end still hit", all(h.probe(k)["where"] is not None for k in keys if k not in miss) and h.probe(keys[10])["crossed"])
    new = sc.search.find(64, 60, 2, why="new listeners of the run's home")
    h.reg(new)
    h.send(sc.rng, 12, miss)
    tbl = h.steps[-1].tables[0][0]
    sc.witness("I: the new listeners extend the run to entry 6", used(tbl) == {60, 61, 62, 63, 0, 1, 2, 3, 4, 5, 6} and h.probe(new[1])["entry"] == 6 and h.probe(new[1])["walk"] == 9)
    return sc.check()


def scenario_h(seed=20260):
    """keys with candidates (a listener bound to an address: the entry names a candidate record, GYS_LOCAL_GROUP, and the event's server
    address decides) among the displaced entries of a 16-entry table: home 15 holds a plain key, entry 0 a key with candidates (read
    through the copy), entry 1 a plain key, entry 2 a key with candidates that only the walk reaches; events with a server address that
    matches no candidate are nobody's"""
    sc = Scenario("H", seed)
    h = sc.host()
    keys = sc.search.find(16, 15, 4, why="the run")
    h.reg(keys, {keys[1]: 1, keys[3]: 2})
    miss = sc.search.find(16, 15, 1, why="miss of the run's home")
    st = h.send(sc.rng, 13, miss)
    tbl = st.tables[0][0]
    p = [h.probe(k) for k in keys]
    sc.witness("H: 16 entries, the run fills 15, 0, 1, 2", len(tbl) == 16 and used(tbl) == {15, 0, 1, 2})
    sc.witness("H: a key with candidates in entry 0 behind home mask, read through the copy", p[1]["via_copy"] and p[1]["local"] == LOCAL_GROUP | 0)
    sc.witness("H: a key with candidates that only the walk reaches", p[3]["where"] == "walk" and p[3]["entry"] == 2 and p[3]["local"] == LOCAL_GROUP | 1)
    sc.witness("H: plain keys before and between them", p[0]["local"] == 0 and p[2]["local"] == 2 and p[2]["where"] == "walk")
    nobody = int.from_bytes(NOBODY, "little")
    sc.witness("H: events whose key has candidates and whose server address matches none",
               all(((st.events["netns"] == k[0]) & (st.events["sport_be"] == k[1]) & (st.events["saddr"] == nobody)).sum() == 2 for k in (keys[1], keys[3])))
    return sc.check()


def to_v6(ev):
    """the same traffic as 48-byte IPv6 events: every address as ::ffff:a.b.c.d (equals the IPv4 address, GY_IP_ADDR::operator==)"""
    out = np.zeros(len(ev), dtype=wire.RESP_EVENT6)
    for f in ("saddr", "daddr"):
        a = np.zeros((len(ev), 16), dtype=np.uint8)
        a[:, 10:12] = 0xFF
        a[:, 12:16] = np.ascontiguousarray(ev[f]).astype("<u4").view(np.uint8).reshape(len(ev), 4)
        a[ev[f] == 0] = 0
        out[f] = a
    for f in ("netns", "sport_be", "dport_be", "lsndtime", "lrcvtime"):
        out[f] = ev[f]
    return out


BUILDERS = {"H": scenario_h, "A": scenario_a, "B": scenario_b, "C": scenario_c, "D": scenario_d, "E": scenario_e, "F": scenario_f, "G": scenario_g, "I": scenario_i}
_cache = {}


def scenario(name):
    """the checked scenario `name` (built once per process; treat it as read-only)"""
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


# ---------------------------------------------------------------------------------------------- hand-over to the C++ programs
def write_registry_ops(path, names):
    """the registry calls of every host of the scenarios `names` for tests/cpp/test_hostlst.cc --tables; returns the hosts in file order"""
    hosts = [h for n in names for h in scenario(n).hosts]
    with open(path, "w") as f:
        for h in hosts:
            f.write("host\n")
            for st in h.steps:
                if st.kind == "reg":
                    f.write("reg %d\n" % len(st.keys) + "".join("%x %d %d %d\n" % (k[0], k[1], s, st.bound.get(k, 0)) for k, s in zip(st.keys, st.svcs)))
                else:
                    f.write("del %d\n" % len(st.svcs) + "".join("%d\n" % s for s in st.svcs))
                f.write("dump\n")
        f.write("end\n")
    return hosts


def parse_registry_dump(text):
    """what test_hostlst.cc --tables printed -> per host, per dump: ([(entries, slots)] per part, [candidate records (ip32, flags, local, slot)])"""
    hosts = []
    lines = iter(text.split("\n"))
    for ln in lines:
        w = ln.split()
        if not w:
            continue
        if w == ["host"]:
            hosts.append([])
        elif w[0] == "tables":
            parts = []
            for _ in range(int(w[1])):
                next(lines)  # "part p cap nlst"
                parts.append(([int(x, 16) for x in next(lines).split()], [int(x) for x in next(lines).split()]))
            hosts[-1].append((parts, []))
        elif w[0] == "cands":
            hosts[-1][-1][1].extend(tuple(int(x) for x in next(lines).split()) for _ in range(int(w[1])))
    return hosts


class World:
    """hosts of several scenarios side by side, one step each: what one launch of the kernel (or one engine) sees"""

    def __init__(self, name, hosts_steps, tpt=16):
        self.name, self.tpt = name, tpt
        self.hosts = [(h, h.steps[i]) for h, i in hosts_steps]


def standin_worlds():
    """the launches of tests/cpp/kemu/test_resp_lookup.cc: hosts of different table sizes side by side, so that a small table's copy of
    entry 0 lies inside a larger LDS area"""
    S = scenario
    last = lambda n: [(h, len(h.steps) - 1) for h in S(n).hosts]
    i = S("I").hosts[0]
    return [World("ABCD", last("A") + last("C") + last("B") + last("D")), World("E", last("E") + last("C")[:1]),
            World("F.quarter+A", [(S("F").hosts[0], 0)] + last("A")), World("F.half+B", [(S("F").hosts[1], 0)] + last("B"), tpt=8),
            World("G+A", last("G") + last("A")), World("H+C", last("H") + last("C")), World("I.deleted+B", [(i, 1)] + last("B")), World("I.added+A", [(i, 2)] + last("A"))]


def write_standin(path, worlds):
    """listeners (in the order of their oracle slots: the live services in registration order; with their address kind), candidate records,
    tables, local -> slot lists and events"""
    with open(path, "w") as f:
        for w in worlds:
            f.write("world %s %d %d %d\n" % (w.name, w.tpt, int(any(st.bound for _, st in w.hosts)), len(w.hosts)))
            base = 0
            for h, st in w.hosts:
                f.write("host %s %d %d %d %d\n" % (h.name, len(st.live), len(st.tables), len(st.events), len(st.cands)))
                f.write("".join("%x %d %d\n" % (k[0], k[1], st.bound.get(k, 0)) for k in st.live_keys))
                pos = {s: base + i for i, s in enumerate(st.live)}
                f.write("".join("%d %d %d %d\n" % (c[0], c[1], c[2], pos[c[3]]) for c in st.cands))
                for tbl, slots in st.tables:
                    f.write("part %d %d\n" % (len(tbl), len(slots)))
                    f.write(" ".join("%x" % e for e in tbl) + "\n")
                    f.write(" ".join("%d" % pos[s] for s in slots) + "\n")
                f.write(" ".join("%x" % x for x in np.frombuffer(st.events.tobytes(), dtype="<u4")) + "\n")
                base += len(st.live)
        f.write("end\n")
