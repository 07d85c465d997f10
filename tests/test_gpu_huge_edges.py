"""GPU parity of the several-workgroup t-digest path for large keys (gys_huge.hpp: k_huge_plan / k_huge_clear / k_huge_count, the two
tiers of k_huge_merge, the one-workgroup fallback k_digest_huge) at the inputs that steer it.  A key that brings more than 16 384
values in one call takes this path; with L its values below GYS_HB_BINS (16 384 ms) and T those at or above ("tail values"):
  * T <= GYS_HB_TAIL_A (512): tier A (unsorted tail list, ranks by a linear count, ties by list position); T <= GYS_HB_TAIL_LDS
    (16 384): tier B (bitonic sort in LDS); more: the fallback.  Tail values come from the run (the global tail list, filtered by
    entry) and from the key's buffered words, and both count;
  * a run of up to GYS_HB_CHUNK (131 072) values is one chunk whose bins are written with plain stores, a longer one is added to
    cleared bins with device atomics by several workgroups;
  * k_huge_count takes a chunk as 0 .. 3 head words up to the first 16-byte boundary, sweeps of 2 x 1024 16-byte pieces, and 0 .. 3
    words behind the last piece;
  * the global tail list has GYS_HB_TAIL_CAP (2^20) places; one value more and every entry of the round takes the fallback.
Every case is a response batch with chosen per-service counts and latencies, shuffled, and is compared with the oracle's sequential
engine on the same bytes, bit for bit: both histogram records, CONN_BITMAP rows, digest sums / counts / min / max, buffered values as
multisets, quantiles.  The route is not inferred from the test's arithmetic alone: SketchEngine.huge_counts() reads the path's own
list lengths (large entries, entries handed to tier B, entries handed to the fallback) after every batch.

Buffers: td_buf_values = 1024 at the default td_pend_cap (896); at td_pend_cap 1920 the library accepts no buffer below
td_pend_cap + 64, so 1984 there.  A call of 300 events stays buffered at both.

Where a run starts (words from a 16-byte boundary of `staged`, whose base is 256-byte aligned), by front end:
  * general: every key's values of the batch are scattered into `staged` in slot order (batch_off = prefix sums of the per-key counts),
    so the run of the key in slot k starts at the sum of the counts of slots < k: three keys of lengths = 1 (mod 4) start at residues
    0, 1, 2 and three of lengths = 3 (mod 4) at 0, 3, 2;
  * host-local: only spilled keys get a run, from a bump cursor that starts at 0 in every batch (FIN_RUN_ALLOC) in the order in which
    the finalizing threads reach it; runs are not padded.  With three large keys of lengths = 1 (mod 4) the three runs start at
    residues 0, 1, 2 whatever the order, with lengths = 3 (mod 4) at 0, 3, 2 -- and all three keys are large, so each residue is a
    large key's.  (A key that was large in the batch before gets a predicted run of prev + prev / 4 + 64 words from the same cursor;
    the alignment cases use a fresh engine so that only exact runs exist, the repeated cases below run on predicted runs.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_resp import PATHS, _assert_path, _compare_all, _compare_window, _engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    src = open(os.path.join(ROOT, "gyeeta_amd", "csrc", "gys_huge.hpp")).read()
    m = re.search(r"^#define %s\s+\(?\s*(\d+)u(?:\s*<<\s*(\d+))?\s*\)?" % name, src, flags=re.M)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


BINS, CHUNK, TAIL_A, TAIL_B, VEC, TAIL_CAP = (_define(n) for n in ("GYS_HB_BINS", "GYS_HB_CHUNK", "GYS_HB_TAIL_A", "GYS_HB_TAIL_LDS", "GYS_HB_VEC", "GYS_HB_TAIL_CAP"))
SWEEP = 1024 * VEC * 4      # values one sweep of k_huge_count's vector loop takes: GYS_HB_VEC x 1024 pieces of four words
LARGE = BINS + 1            # the smallest large key (empty buffer)
QS = [0.001, 0.5, 0.999]

CAPS = pytest.mark.parametrize("td_cap", [0, 1920], ids=["cap896", "cap1920"])


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def route(T):
    """(entries handed to tier B, entries handed to the fallback) of one large key with T tail values, by the rule in the source"""
    return (0, 0) if T <= TAIL_A else (1, 0) if T <= TAIL_B else (1, 1)


def low(rng, n):
    """n latencies below GYS_HB_BINS: a lognormal body (most bins near the bottom, a long sparse upper part) and both edge bins"""
    v = np.minimum(np.floor(rng.lognormal(4.0, 1.6, n)), BINS - 1).astype(np.uint32)
    v[: min(n, 2)] = (0, BINS - 1)[: min(n, 2)]
    return v


def tail(rng, n):
    """n latencies >= GYS_HB_BINS: a third from a narrow range just above the last bin (ties), the rest up to 10^6, both ends present"""
    v = np.where(rng.random(n) < 0.34, rng.integers(BINS, BINS + 1 + n // 8, n), rng.integers(BINS, 1_000_001, n)).astype(np.uint32)
    v[: min(n, 2)] = (1_000_000, BINS)[: min(n, 2)]
    return v


class Rig:
    """one host with nsvc services in the engine and in the oracle; two_views: a second oracle engine whose records are never cleared
    (the all-time view of a test that closes a window half way -- without one the two views are the same records)"""

    def __init__(self, oracle, nsvc, max_events, resp_path, td_cap, max_services=8, two_views=False):
        self.oracle, self.nsvc, self.resp_path = oracle, nsvc, resp_path
        self.eng = _engine(max_hosts=2, max_services=max_services, max_batch_events=max_events, resp_path=resp_path, td_pend_cap=td_cap,
                           td_buf_values=1984 if td_cap else 1024)
        self.orc = oracle.OracleEngine(max_services, td_cap=td_cap)      # records cleared at every window close
        self.orc_all = oracle.OracleEngine(max_services, td_cap=td_cap) if two_views else None
        info, gids = helpers.register_world(self.eng, self.orc, [0], nsvc)
        if two_views:
            helpers.register_world(None, self.orc_all, [0], nsvc)
        self.mid, self.slot = info[0]
        self.gids = gids[0]

    def send(self, rng, per_svc):
        """one call: {service: latencies}; the events of all services shuffled together"""
        svc = np.concatenate([np.full(len(v), s, dtype=np.int64) for s, v in per_svc.items()])
        lat = np.concatenate([np.asarray(v, dtype=np.uint32) for v in per_svc.values()])
        perm = rng.permutation(len(svc))
        svc, lat = svc[perm], lat[perm]
        ev = helpers.make_resp_events(rng, 0, len(svc), self.nsvc, lat=lat, bad_frac=0, unknown_frac=0, zero_ip_frac=0)
        ev["netns"] = helpers.wire.listener_netns(0, svc)  # the chosen services instead of the drawn ones
        ev["sport_be"] = helpers.wire.listener_port(svc)
        self.eng.handle_resp_events(self.mid, ev)
        raw = ev.tobytes()
        for o in (self.orc, self.orc_all):
            if o is not None:
                o.resp_batch(raw, [self.slot], [0])
        self.eng.sync()
        return len(ev)

    def check(self, huge=None, tier_b=None, fallback=None, svcs=()):
        if huge is not None:
            hc = self.eng.huge_counts()
            assert (hc["huge"], hc["tier_b"], hc["fallback"]) == (huge, tier_b, fallback), hc
        _compare_all(self.eng, self.orc, self.oracle)  # window records, CONN_BITMAP rows, digests, min / max, buffered values
        n = self.orc.nsvc
        helpers.assert_hist_equal(self.eng.export_hist(1, 0, n), (self.orc_all or self.orc).hist(), n)  # all-time records
        for s in svcs:
            want = [self.oracle.lib().gyo_tdb_quantile(C.byref(self.orc.td(s)), q) for q in QS]
            assert self.eng.quantiles(int(self.gids[s]), QS) == want

    def window_close(self):
        self.eng.window_close()
        _compare_window(self.eng, self.orc)
        self.orc.window_clear(clear_hist=True)
        if self.orc_all is not None:
            self.orc_all.window_clear(clear_hist=False)

    def finish(self):
        _assert_path(self.eng, self.resp_path)
        c, oc = self.eng.counters(), self.orc.counters()
        assert c["resp_events"] == oc["events"] == oc["accepted"]
        self.window_close()
        self.eng.close()


# (a second chunk of exactly one sweep and of exactly two, give or take)
RUN_LENGTHS = [LARGE, CHUNK] + [CHUNK + r for r in (1, 3, 4, 5, 7)] + [CHUNK + k * SWEEP + d for k in (1, 2) for d in (-1, 0, 1, 7)] + [2 * CHUNK + 3]


@PATHS
@CAPS
def test_run_lengths(torch_mod, oracle, resp_path, td_cap):
    """T = 0, empty buffer: the smallest large key, exactly one chunk, a second chunk of 1 .. 7 values (nothing but head words, exactly
    one piece, a piece and words behind it), a second chunk of one and of two whole sweeps of the vector loop give or take, a third chunk"""
    rng = np.random.default_rng(4100 + td_cap)
    rig = Rig(oracle, 6, 1 << 19, resp_path, td_cap)
    for i, m in enumerate(RUN_LENGTHS):
        s = i % 6  # (a large key's buffer is empty again after its merge)
        assert rig.send(rng, {s: low(rng, m)}) == m
        rig.check(1, 0, 0, svcs=[s])
        assert rig.eng.huge_counts()["tail_values"] == 0
    rig.finish()


@PATHS
@CAPS
@pytest.mark.parametrize("mod4", [1, 3])
def test_run_alignment(torch_mod, oracle, resp_path, td_cap, mod4):
    """three large keys of run lengths = mod4 (mod 4) in one call of a fresh engine: their runs start at residues {0, 1, 2} resp.
    {0, 3, 2} words from a 16-byte boundary (module docstring); the middle key has a second chunk of 5 resp. 7 values, at the same
    residue as its first.  A few tail values each, so that head words and the words behind the last piece take both branches."""
    rng = np.random.default_rng(4200 + td_cap + mod4)
    lens = [LARGE + mod4 - 1, CHUNK + 4 + mod4, LARGE + 4 + mod4 - 1]
    assert all(m % 4 == mod4 for m in lens)
    rig = Rig(oracle, 3, 1 << 18, resp_path, td_cap)
    rig.send(rng, {s: np.concatenate([low(rng, m - 40 * (s + 1)), tail(rng, 40 * (s + 1))]) for s, m in enumerate(lens)})
    rig.check(3, 0, 0, svcs=range(3))
    assert rig.eng.huge_counts()["tail_values"] == 40 + 80 + 120
    rig.finish()


def _value_cases(rng):
    """(name, latencies, T)"""
    asc = lambda m: np.minimum(np.arange(m, dtype=np.int64), 1_000_000).astype(np.uint32)
    return [
        ("all 16383", np.full(LARGE, BINS - 1, np.uint32), 0),
        ("all 16384", np.full(LARGE, BINS, np.uint32), LARGE),
        ("all 0", np.zeros(LARGE, np.uint32), 0),
        ("all 1000000", np.full(LARGE, 1_000_000, np.uint32), LARGE),
        ("ascending, T in tier A", asc(BINS + 416), 416),
        ("ascending, T in tier B", asc(20000), 20000 - BINS),
        ("ascending, clipped to 10^6", asc(1_000_003), 1_000_003 - BINS),
        ("half 16383, half 16384", np.repeat(np.array([BINS - 1, BINS], np.uint32), 8193), 8193),
        ("equal tail values in tier A", np.concatenate([low(rng, LARGE - 400), np.full(400, BINS, np.uint32)]), 400),
        ("equal tail values in tier B", np.concatenate([low(rng, LARGE - 5000), np.full(5000, BINS, np.uint32)]), 5000),
        ("two equal tail values and the rest below, tier A", np.concatenate([np.full(LARGE, BINS - 1, np.uint32), np.full(2, BINS + 7, np.uint32)]), 2),
    ]


@CAPS
def test_values(torch_mod, oracle, td_cap):
    """runs of equal values on either side of bin 16 383 | 16 384, at both ends of the range, ascending values, ties among the tail
    values in both tiers (tier A breaks them by list position, tier B by the sort, the fallback counts them in its bins)"""
    rng = np.random.default_rng(4300 + td_cap)
    rig = Rig(oracle, 8, 1 << 20, 2, td_cap)
    for i, (name, lat, T) in enumerate(_value_cases(rng)):
        assert int((lat >= BINS).sum()) == T, name
        s = i % 8
        rig.send(rng, {s: lat})
        rig.check(1, *route(T), svcs=[s])
    rig.finish()


TAIL_COUNTS = [0, 1, TAIL_A - 1, TAIL_A, TAIL_A + 1, 1023, 1024, 1025, TAIL_B - 1, TAIL_B, TAIL_B + 1]


@CAPS
@pytest.mark.parametrize("T,L", [(T, max(1, LARGE - T)) for T in TAIL_COUNTS] + [(LARGE, 0)], ids=lambda x: str(x))
def test_tail_counts(torch_mod, oracle, td_cap, T, L):
    """T tail values and L others, twice in a row on one key: into an empty digest, then into one whose upper clusters have means
    above 16 384 (the `vmax >= GYS_HB_BINS` search: linear in tier A, binary in tier B)"""
    rng = np.random.default_rng(4400 + td_cap + T)
    assert L + T >= LARGE
    rig = Rig(oracle, 2, 1 << 16, 2, td_cap)
    for rep in range(2):
        if rep == 1 and T:  # (the second run does meet clusters up there)
            d = rig.orc.td(0).d
            assert max(d.sum[j] // d.cnt[j] for j in range(len(d.cnt)) if d.cnt[j]) > BINS
        rig.send(rng, {0: np.concatenate([low(rng, L), tail(rng, T)]), 1: low(rng, 50)})
        rig.check(1, *route(T), svcs=[0])
        assert rig.eng.huge_counts()["tail_values"] == T
    rig.finish()


@CAPS
@pytest.mark.parametrize("close", [False, True], ids=["samewindow", "windowbetween"])
def test_split_sources(torch_mod, oracle, td_cap, close):
    """300 tail values wait in the key's buffer (an earlier call of 300 events stays buffered), then a run brings 212 more (512: tier A)
    resp. 213 (513: tier B) -- the two sources feed one count.  With a window close in between the buffered words are of an earlier
    window: they go to the all-time record only and the window's record rolls."""
    rng = np.random.default_rng(4500 + td_cap + close)
    rig = Rig(oracle, 3, 1 << 16, 2, td_cap, two_views=close)
    rig.send(rng, {0: tail(rng, 300), 1: tail(rng, 300), 2: low(rng, 300)})
    rig.check()
    assert (rig.eng.export_tdigest_pending(0, 3)[0] == 300).all()
    if close:
        rig.window_close()
    for s, t in ((0, TAIL_A - 300), (1, TAIL_A - 300 + 1)):
        rig.send(rng, {s: np.concatenate([low(rng, LARGE - t), tail(rng, t)]), 2: low(rng, 10)})
        rig.check(1, *route(300 + t), svcs=[s])
        assert rig.eng.huge_counts()["tail_values"] == t  # (the list holds the run's share only)
    rig.finish()


@CAPS
def test_buffered_tail_values_alone(torch_mod, oracle, td_cap):
    """the tail values all wait in the buffer (two calls of 300 and 212 resp. 213 events stay buffered) and the run brings none: 512 fit
    tier A's list, the 513th buffered one hands the entry to tier B -- the buffered words' own bound, which the run's share never meets
    in the cases above"""
    rng = np.random.default_rng(4550 + td_cap)
    rig = Rig(oracle, 3, 1 << 16, 2, td_cap)
    rig.send(rng, {0: tail(rng, 300), 1: tail(rng, 300)})
    rig.send(rng, {0: tail(rng, TAIL_A - 300), 1: tail(rng, TAIL_A - 300 + 1)})
    rig.check()
    assert rig.eng.export_tdigest_pending(0, 2)[0].tolist() == [TAIL_A, TAIL_A + 1]
    for s in (0, 1):
        rig.send(rng, {s: low(rng, LARGE), 2: low(rng, 10)})
        rig.check(1, *route(TAIL_A + s), svcs=[s])
        assert rig.eng.huge_counts()["tail_values"] == 0
    rig.finish()


@PATHS
@CAPS
def test_mixed_batch(torch_mod, oracle, resp_path, td_cap):
    """one call: large keys with T = 0, 1, 600 and 16 385, a key that spills without being large (buffer + 38 values) and one that only
    appends -- every route at once, the runs of different keys next to each other"""
    rng = np.random.default_rng(4600 + td_cap)
    rig = Rig(oracle, 6, 1 << 17, resp_path, td_cap)
    pcap = 1984 if td_cap else 1024
    for rep in range(2):
        call = {0: low(rng, LARGE + 2), 1: np.concatenate([low(rng, LARGE), tail(rng, 1)]), 2: np.concatenate([low(rng, 17000), tail(rng, 600)]),
                3: np.concatenate([low(rng, 9), tail(rng, TAIL_B + 1)]), 4: low(rng, pcap + 38), 5: low(rng, 100)}
        rig.send(rng, call)
        rig.check(4, 2, 1, svcs=range(6))
    rig.finish()


@CAPS
def test_pool_rounds(torch_mod, oracle, td_cap, monkeypatch):
    """a pool of two entries and five large keys: three rounds of plan / clear / count / merge over one huge list; the key with 600
    tail values is in the last round, whose tier B runs on the pool's first entry"""
    monkeypatch.setenv("GYS_HUGE_MAXENT", "2")
    rng = np.random.default_rng(4700 + td_cap)
    rig = Rig(oracle, 6, 1 << 17, 2, td_cap)
    for rep in range(2):
        call = {s: np.concatenate([low(rng, LARGE + 3 * s), tail(rng, 5 * s)]) for s in range(4)}
        call[4] = np.concatenate([low(rng, LARGE), tail(rng, 600)])
        call[5] = low(rng, 70)
        rig.send(rng, call)
        hc = rig.eng.huge_counts()
        assert (hc["huge"], hc["fallback"]) == (5, 0), hc
        rig.check(svcs=range(6))
    rig.finish()


@CAPS
def test_tail_list_full_and_lost(torch_mod, oracle, td_cap):
    """64 keys with 16 384 tail values each fill the global tail list to its last place: nothing is lost, all 64 go through tier B.
    The same call plus a 65th large key with one tail value overflows it: all 65 take the fallback -- one entry more than the
    fallback kernel has workgroups"""
    nk = TAIL_CAP // TAIL_B
    assert nk == 64
    rng = np.random.default_rng(4800 + td_cap)
    rig = Rig(oracle, nk + 1, 1 << 21, 2, td_cap, max_services=128)
    call = {s: np.concatenate([low(rng, 1), tail(rng, TAIL_B)]) for s in range(nk)}
    rig.send(rng, call)
    rig.check(nk, nk, 0, svcs=(0, nk - 1))
    assert rig.eng.huge_counts()["tail_values"] == TAIL_CAP
    call[nk] = np.concatenate([low(rng, BINS), tail(rng, 1)])
    rig.send(rng, call)
    rig.check(nk + 1, 0, nk + 1, svcs=(0, nk - 1, nk))
    assert rig.eng.huge_counts()["tail_values"] == TAIL_CAP + 1
    rig.finish()
