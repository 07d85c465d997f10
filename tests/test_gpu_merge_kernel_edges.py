"""GPU parity of the value-bin merge kernel k_digest_bins at the edges of its phases (the style of tests/test_gpu_resp.py::
test_resp_merge_size_classes): one key per value set, every batch just above the buffer size so that every call ends in a merge of exactly
its own values, three batches in a row per key so that the later merges meet old clusters; the engine against oracle.OracleEngine, bit for bit,
for td_pend_cap 0 (896 values: k_digest_bins<false,4>) and 1920 (k_digest_bins<false,8>).  The value sets are those of
tests/cpp/kemu/test_bins_edges.cc: the list of non-empty one-value bins with 1 / 256 / 257 / 1 024 entries, 512 and 513 large values (the two
sides of the compact / plain choice), more large values than the list holds (hand-over), no one-value bin at all, the edge values of the bins.
Then the same with enable_levels=1 and a window close inside every merge's values (part of the buffer already folded: nh > 0), one batch with
more merges than the launch has workgroups (every workgroup runs entries back to back), and the all-service scan (the SCAN instance)."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

EDGES = np.array([0, 1023, 1024, 1087, 1088, 999999, 1000000], dtype=np.uint32)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine(**kw):
    from gyeeta_amd.engine import SketchEngine
    return SketchEngine(**kw)


def _big(rng, n):
    """n values >= 1024: every octave of the 64-cell bins, the edges of the value domain among them"""
    msb = rng.integers(10, 20, n)
    v = (1 << msb) | (rng.integers(0, 1 << 20, n) & ((1 << msb) - 1))
    v = np.minimum(v, 1000000)
    k = rng.random(n) < 0.2
    return np.where(k, rng.choice(EDGES[2:], n), v).astype(np.uint32)


def _small(rng, n, among=None):
    return (rng.integers(0, 1024, n) if among is None else rng.choice(among, n)).astype(np.uint32)


def _value_sets(cap):
    """name -> function(rng) -> the values of one batch (more than `cap`, at most the merge size)"""
    n = cap + 1
    top = 1024 if cap <= 896 else 2048  # values one merge of the instance takes

    def with_bins(bins):
        bins = np.asarray(bins, dtype=np.uint32)
        return lambda rng: rng.permutation(np.concatenate([bins, _small(rng, max(n, len(bins)) - len(bins), bins)]))

    def with_big(nbig):
        return lambda rng: rng.permutation(np.concatenate([_big(rng, nbig), _small(rng, max(n - nbig, 0))]))

    sets = {
        "one-bin": lambda rng: np.full(n, 37, dtype=np.uint32),
        "bins-256": with_bins(4 * np.arange(256)),
        "bins-257": with_bins(3 * np.arange(257) + 200),
        "bins-1024": with_bins(np.arange(1024)),
        "big-512": with_big(512),
        "big-513": with_big(513),
        "all-big": with_big(n),  # no one-value bin holds a value (896-value buffers: the plain form; 1 920: handed over)
        "edges": lambda rng: rng.permutation(np.concatenate([np.tile(EDGES, 10), _small(rng, n - 70 - 200), _big(rng, 200)])),
    }
    if top > 1024:
        sets["big-over"] = with_big(1025)  # more large values than the list holds: the general kernel's
    for name, f in sets.items():
        v = f(np.random.default_rng(0))
        assert cap < len(v) <= top, (name, len(v))
    return sets


def _events_for(rng, h, svc, lat):
    """a batch of host h whose events all belong to the services `svc` (an index per event) with the response times `lat` (ms)"""
    svc = np.broadcast_to(np.asarray(svc), (len(lat),))
    ev = helpers.make_resp_events(rng, h, len(lat), 1, bad_frac=0.0, unknown_frac=0.0, zero_ip_frac=0.0, lat=np.asarray(lat, dtype=np.uint32))
    ev["netns"] = helpers.wire.listener_netns(h, svc)
    ev["sport_be"] = helpers.wire.listener_port(svc)
    assert (ev["lsndtime"] == ev["lrcvtime"] + np.asarray(lat, dtype=np.uint32)).all()  # (explicit: lsndtime = lrcvtime + lat, modulo 2^32)
    return ev


def _compare_td(eng, orc):
    nsvc = orc.nsvc
    gs, gc, gm = eng.export_tdigest(0, nsvc)
    os_, oc, om = orc.td_arrays()
    assert (gc == oc).all(), f"digest counts differ at {np.argwhere(gc != oc)[:4].tolist()}"
    assert (gs == os_).all()
    assert (gm == om).all()
    gn, gp = eng.export_tdigest_pending(0, nsvc)
    on, op = orc.td_pending()
    assert (gn == on).all(), f"buffer fill differs at {np.argwhere(gn != on)[:4].tolist()}"
    assert (gp == op).all()


def _compare_all(eng, orc):
    nsvc = orc.nsvc
    helpers.assert_hist_equal(eng.export_hist(0, 0, nsvc), orc.hist(), nsvc)
    assert (eng.export_conn_bitmap(0, nsvc) == orc.bitmap()).all()
    _compare_td(eng, orc)


def _compare_quantiles(eng, orc, oracle, gids, nsvc):
    qs = [0.001, 0.25, 0.5, 0.95, 0.99, 0.999]
    L = oracle.lib()
    want = np.array([[L.gyo_tdb_quantile(C.byref(orc.td(i)), q) for q in qs] for i in range(nsvc)])
    got = np.asarray(eng.scan_quantiles(qs)).reshape(-1, len(qs))[:nsvc]  # every service in one pass: k_digest_bins<true, ...>
    assert (got == want).all(), (got[(got != want).any(axis=1)][:3], want[(got != want).any(axis=1)][:3])
    for s in range(nsvc):  # the one-service query: the same merged view through the query form of the merge kernel
        g = int(gids[0][s])
        assert eng.quantiles(g, qs) == got[eng.lookup(g)].tolist()


@pytest.mark.parametrize("td_cap", [0, 1920], ids=["cap896", "cap1920"])
def test_merge_edges_three_batches_per_key(torch_mod, oracle, td_cap):
    cap = td_cap or 896
    sets = _value_sets(cap)
    names = list(sets)
    ns = len(names)
    rng = np.random.default_rng(71)
    eng = _engine(max_hosts=2, max_services=16, max_batch_events=1 << 16, td_pend_cap=td_cap)
    orc = oracle.OracleEngine(16, td_cap=td_cap)
    info, gids = helpers.register_world(eng, orc, range(1), ns)
    mid, slot = info[0]
    for rnd in range(3):  # key s takes the sets s, s + 1, s + 2: every set meets a key without clusters and keys with old clusters
        for s in range(ns):
            ev = _events_for(rng, 0, s, sets[names[(s + rnd) % ns]](rng))
            eng.handle_resp_events(mid, ev)
            orc.resp_batch(ev.tobytes(), [slot], [0])
            gn, _ = eng.export_tdigest_pending(0, ns)
            assert gn[eng.lookup(int(gids[0][s]))] == 0, (rnd, names[(s + rnd) % ns])  # the call ended in a merge of exactly its batch
        eng.sync()
        _compare_all(eng, orc)
    # some values in every buffer, then the merged views: the scan of every service and the one-service query
    for s in range(ns):
        ev = _events_for(rng, 0, s, sets[names[s]](rng)[:150 + 37 * s])
        eng.handle_resp_events(mid, ev)
        orc.resp_batch(ev.tobytes(), [slot], [0])
    eng.sync()
    _compare_all(eng, orc)
    _compare_quantiles(eng, orc, oracle, gids, ns)
    eng.close()


@pytest.mark.parametrize("td_cap", [0, 1920], ids=["cap896", "cap1920"])
def test_merge_edges_with_a_folded_part(torch_mod, oracle, td_cap):
    """enable_levels=1: the window close between the two parts of a merge's values folds the buffered part into the records (nh > 0), the
    merge folds the rest; digests, buffers and extremes against the oracle engine, the all-time records against the oracle's histograms of
    every event so far (the oracle engine's window is never cleared here)"""
    cap = td_cap or 896
    sets = _value_sets(cap)
    names = list(sets)
    ns = len(names)
    rng = np.random.default_rng(72)
    eng = _engine(max_hosts=2, max_services=16, max_batch_events=1 << 16, td_pend_cap=td_cap, enable_levels=1)
    orc = oracle.OracleEngine(16, td_cap=td_cap)
    info, gids = helpers.register_world(eng, orc, range(1), ns)
    mid, slot = info[0]
    t = 1_700_000_000
    for rnd in range(3):
        vals = [sets[names[(s + rnd) % ns]](rng) for s in range(ns)]
        for part in range(2):  # 300 values of every key (buffered), the close, then the rest (the merge: 300 folded + the new ones)
            for s in range(ns):
                v = vals[s][:300] if part == 0 else vals[s][300:]
                ev = _events_for(rng, 0, s, v)
                eng.handle_resp_events(mid, ev)
                orc.resp_batch(ev.tobytes(), [slot], [0])
            if part == 0:
                gn, _ = eng.export_tdigest_pending(0, ns)
                assert (gn[:ns] == 300).all()
                t += 5
                eng.window_close(t * 1_000_000)
        eng.sync()
        _compare_td(eng, orc)
    t += 5
    eng.window_close(t * 1_000_000)
    eng.sync()
    _compare_td(eng, orc)
    helpers.assert_hist_equal(eng.export_hist(1, 0, orc.nsvc), orc.hist(), orc.nsvc)
    _compare_quantiles(eng, orc, oracle, gids, ns)
    eng.close()


def test_more_merges_than_workgroups_in_one_batch(torch_mod, oracle):
    """3 hosts x 768 services x 897 events in ONE call at the 896-value buffer: 2 304 merges for a launch of at most 8 x CUs workgroups, so
    workgroups run several entries back to back (the loop-carried order of an entry's write-back and the next entry's clears and loads)"""
    torch = torch_mod
    nh, sp, per = 3, 768, 897
    rng = np.random.default_rng(73)
    eng = _engine(max_hosts=nh, max_services=nh * sp, max_batch_events=1 << 22)
    assert 8 * torch.cuda.get_device_properties(0).multi_processor_count < nh * sp
    orc = oracle.OracleEngine(nh * sp)
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
