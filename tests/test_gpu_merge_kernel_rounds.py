"""GPU parity of the value-bin merge kernel k_digest_bins at the bounds that decide what a round of 256 values has to test and at the shapes of
its large-value list (the cases of tests/cpp/kemu/test_bins_rounds.cc that can be reached through the engine), in the style of
tests/test_gpu_merge_kernel_edges.py: one host, one key per case, the engine against oracle.OracleEngine bit for bit, for td_pend_cap 0 (896
values: k_digest_bins<false,4>) and 1920 (k_digest_bins<false,8>).
  - The window bound: n1 values of a key stay buffered (1, 255, 256, 257, 512, the buffer size minus 1), the window closes, the next batch
    takes the key just over the buffer size: the merge's first n1 values belong to the earlier window (all-time record only), the window's
    record rolls.  Clusters, min / max, buffers, the window records, the CONN_BITMAP rows and the all-time records (a second oracle engine whose
    records are never cleared) are compared.
  - The same with enable_levels=1: the close folds the buffered part into the records (nh = n1), the merge folds the rest; clusters, min / max
    and buffers after every step, the all-time records at the end (the oracle engine's records are never cleared there, as in
    test_merge_edges_with_a_folded_part).
  - The large-value sets: 0 ... 1 024 large values and one more than the list holds, one cell full of one value / of distinct values, every cell
    once (the latencies an event can carry end at 1 000 000: the cells above it stay empty), the cells' first and last values, and old clusters
    whose thresholds lie in an occupied cell, in an empty one between two occupied ones and exactly on a large value; three batches per key, so
    that the later merges meet old clusters above 1 024.
  - One batch with more merges than the launch has workgroups at the 1 920-value buffer."""
import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_huge_edges import Rig
from tests.test_gpu_merge_kernel_edges import _big, _compare_all, _compare_td, _engine, _events_for, _small, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

CAPS = pytest.mark.parametrize("td_cap", [0, 1920], ids=["cap896", "cap1920"])


def _n1s(cap):
    return [1, 255, 256, 257, 512, cap - 1]


def _calls(n1, cap):
    """the batch sizes that leave n1 values buffered: a key is queued for a merge when its buffer holds more than `cap` values or when another
    batch like the last one would take it past the fast merge size (finalize_one: cur > pend_cap || cur + m > merge_fast), so the fill is
    approached by halves of the room that is left"""
    fast, cur, out = (1024 if cap <= 896 else 2048), 0, []
    while cur < n1:
        m = min(n1 - cur, (fast - cur) // 2)
        assert m > 0
        out.append(m)
        cur += m
    return out


def _mixed(rng, n):
    """n latencies: most below 1 024 with repeats, about one in sixteen a second or longer"""
    v = np.minimum(np.floor(rng.lognormal(4.0, 1.3, n)), 1023).astype(np.uint32)
    k = rng.random(n) < 1 / 16
    return np.where(k, _big(rng, n), v).astype(np.uint32)


@CAPS
def test_window_bound_inside_a_merge(torch_mod, oracle, td_cap):
    cap = td_cap or 896
    n1s = _n1s(cap)
    rng = np.random.default_rng(81 + td_cap)
    rig = Rig(oracle, len(n1s), 1 << 16, 2, td_cap, max_services=8, two_views=True)
    for rnd in range(2):  # (the second round's merges meet old clusters)
        calls = [_calls(n1, cap) for n1 in n1s]
        for c in range(max(len(x) for x in calls)):
            rig.send(rng, {s: _mixed(rng, x[c]) for s, x in enumerate(calls) if c < len(x)})
        rig.check()
        assert rig.eng.export_tdigest_pending(0, len(n1s))[0].tolist() == n1s
        rig.window_close()
        rig.send(rng, {s: _mixed(rng, cap + 1 - n1) for s, n1 in enumerate(n1s)})
        assert (rig.eng.export_tdigest_pending(0, len(n1s))[0] == 0).all()  # every key was merged: n1 buffered values of the earlier window + the rest
        rig.check()
    rig.finish()


@CAPS
def test_folded_bound_inside_a_merge(torch_mod, oracle, td_cap):
    cap = td_cap or 896
    n1s = _n1s(cap)
    ns = len(n1s)
    rng = np.random.default_rng(82 + td_cap)
    eng = _engine(max_hosts=2, max_services=8, max_batch_events=1 << 16, td_pend_cap=td_cap, enable_levels=1)
    orc = oracle.OracleEngine(8, td_cap=td_cap)
    info, gids = helpers.register_world(eng, orc, range(1), ns)
    mid, slot = info[0]
    t = 1_700_000_000
    for rnd in range(2):
        for part in range(2):
            for s, n1 in enumerate(n1s):
                for m in (_calls(n1, cap) if part == 0 else [cap + 1 - n1]):
                    ev = _events_for(rng, 0, s, _mixed(rng, m))
                    eng.handle_resp_events(mid, ev)
                    orc.resp_batch(ev.tobytes(), [slot], [0])
            gn, _ = eng.export_tdigest_pending(0, ns)
            if part == 0:
                assert gn[:ns].tolist() == n1s
                t += 5
                eng.window_close(t * 1_000_000)
            else:
                assert (gn[:ns] == 0).all()
        eng.sync()
        _compare_td(eng, orc)
    t += 5
    eng.window_close(t * 1_000_000)
    eng.sync()
    _compare_td(eng, orc)
    helpers.assert_hist_equal(eng.export_hist(1, 0, orc.nsvc), orc.hist(), orc.nsvc)
    eng.close()


def _cell_lo(c):
    msb = 10 + c // 64
    return (1 << msb) | ((c % 64) << (msb - 6))


def _large_sets(cap):
    """name -> function(rng) -> the values of one batch: more than `cap`, at most what one merge of the instance takes"""
    n = cap + 1
    top = 1024 if cap <= 896 else 2048

    def fill(big):
        big = np.minimum(np.asarray(big, dtype=np.int64), 1_000_000).astype(np.uint32)  # (the largest latency an event carries)
        return lambda rng: rng.permutation(np.concatenate([big, _small(rng, max(n - len(big), 0))]))

    def nbig(k):
        return lambda rng: fill(_big(rng, k))(rng)

    cells = np.array([_cell_lo(c) for c in range(640)], dtype=np.int64)
    widths = np.array([1 << (4 + c // 64) for c in range(640)], dtype=np.int64)
    edge_cells = [0, 1, 63, 64, 200, 377, 634]
    sets = {"nbig-%d" % k: nbig(k) for k in (0, 1, 3, 4, 5, 255, 256, 257, 512, 513, 1023, 1024)}
    if top > 1024:
        sets["nbig-over"] = nbig(1025)  # more large values than the list holds: handed to the general kernel
    sets["one-cell-one-value"] = fill(np.full(300, 5000))
    sets["one-cell-distinct"] = fill(65536 + np.arange(600))
    sets["every-cell"] = lambda rng: fill(cells + rng.integers(0, widths))(rng)
    sets["cell-ends"] = fill(np.concatenate([np.tile([cells[c], cells[c] + widths[c] - 1], 3) for c in edge_cells] + [[1_000_000] * 3, [999_999]]))
    for name, f in sets.items():
        v = f(np.random.default_rng(0))
        assert cap < len(v) <= top, (name, len(v))
    return sets


@CAPS
def test_large_value_sets_three_batches_per_key(torch_mod, oracle, td_cap):
    cap = td_cap or 896
    sets = _large_sets(cap)
    names = list(sets)
    ns = len(names)
    rng = np.random.default_rng(83 + td_cap)
    # the last key: pure old clusters at 5003 (new values in its cell [4992, 5056)), 5100 (none in [5056, 5120), some on both sides), 9000 (a new value)
    thr_hist = np.repeat(np.array([5003, 5100, 9000], dtype=np.uint32), (cap + 3) // 3)
    thr_vals = np.array([5000, 5010, 5002, 5003, 5004, 5055, 4992, 5130, 5150, 5120, 9000, 9000, 9000, 8999, 9001, 8960, 9023], dtype=np.uint32)
    eng = _engine(max_hosts=2, max_services=32, max_batch_events=1 << 16, td_pend_cap=td_cap)
    orc = oracle.OracleEngine(32, td_cap=td_cap)
    info, gids = helpers.register_world(eng, orc, range(1), ns + 1)
    mid, slot = info[0]
    for rnd in range(3):  # key s takes the sets s, s + 1, s + 2: an entry with large values directly behind one with none among them
        for s in range(ns + 1):
            if s < ns:
                lat = sets[names[(s + rnd) % ns]](rng)
            else:
                lat = rng.permutation(thr_hist) if rnd == 0 else rng.permutation(np.concatenate([thr_vals, _small(rng, cap + 1 - len(thr_vals))]))
            ev = _events_for(rng, 0, s, lat)
            eng.handle_resp_events(mid, ev)
            orc.resp_batch(ev.tobytes(), [slot], [0])
            gn, _ = eng.export_tdigest_pending(0, ns + 1)
            assert gn[eng.lookup(int(gids[0][s]))] == 0, (rnd, s)  # the call ended in a merge of exactly its batch
        eng.sync()
        _compare_all(eng, orc)
        if rnd == 0:  # the thresholds the last key's later merges are there for
            gs, gc, _ = eng.export_tdigest(0, ns + 1)
            row = eng.lookup(int(gids[0][ns]))
            for want in (5003, 5100, 9000):
                assert ((gc[row] > 0) & (gs[row] == want * gc[row].astype(np.int64))).any(), want
    helpers.assert_hist_equal(eng.export_hist(1, 0, orc.nsvc), orc.hist(), orc.nsvc)  # the all-time records (no window was closed: the same events)
    eng.close()


def test_more_merges_than_workgroups_at_the_1920_buffer(torch_mod, oracle):
    """3 hosts x 700 services x 1 921 events in ONE call: 2 100 merges of k_digest_bins<false,8> for a launch of at most 8 x CUs workgroups"""
    torch = torch_mod
    nh, sp, per = 3, 700, 1921
    rng = np.random.default_rng(84)
    eng = _engine(max_hosts=nh, max_services=nh * sp, max_batch_events=1 << 23, td_pend_cap=1920)
    assert 8 * torch.cuda.get_device_properties(0).multi_processor_count < nh * sp
    orc = oracle.OracleEngine(nh * sp, td_cap=1920)
    info, gids = helpers.register_world(eng, orc, range(nh), sp)
    from gyeeta_amd import capi
    parts, segs = [], (capi.RespSeg * nh)()
    for h in range(nh):
        svc = rng.permutation(np.repeat(np.arange(sp), per))
        mu = rng.normal(3.0, 1.0, sp)[svc]  # (some services around a second: a few hundred large values per merge)
        lat = np.minimum(np.floor(np.exp(mu + 1.5 * rng.standard_normal(len(svc)))), 1e6).astype(np.uint32)
        parts.append(_events_for(rng, h, svc, lat))
        segs[h].host_slot = info[h][1]
        segs[h].first_event = h * sp * per
    raw = helpers.concat_events(parts)
    d_ev = torch.from_numpy(np.frombuffer(raw.tobytes(), dtype=np.uint8).copy()).cuda()
    eng.handle_resp_events_dev(segs, d_ev.data_ptr(), len(raw))
    orc.resp_batch(raw.tobytes(), [info[h][1] for h in range(nh)], [h * sp * per for h in range(nh)])
    eng.sync()
    gn, _ = eng.export_tdigest_pending(0, nh * sp)
    assert (gn == 0).all()  # every key was merged
    _compare_all(eng, orc)
    eng.close()
