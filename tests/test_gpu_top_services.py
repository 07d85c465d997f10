"""gys_top_services: the service ranking on a sketch result in one call -- the scan, the filter and the exact top-k (gyeeta_amd/csrc/gys_topk_host.hpp).
One engine: 3 hosts x 40 services, td_pend_cap 64, svc_hll_p 4 with svc_hll_levels; latencies scaled per service so that the order is not the slot
order; services without events, services with buffered values only, one listener deleted (a free slot), one window closed (the levels hold data).
Every ranking equals, BIT FOR BIT, the numpy ordering (np.lexsort on (slot, value + 0.0)) of the corresponding scan's column restricted to the
eligible slots; glob_id, slot, host_slot and total are checked; no tolerances."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers
from tests.test_gpu_td_ranks import events_for, torch_mod  # noqa: F401 (torch_mod is a fixture)

pytestmark = pytest.mark.gpu

H, S = 3, 40
T0 = 1_700_000_000 - 1_700_000_000 % 432000 + 17
EMPTY = (3, 17)       # service indices (on every host) that never get an event
BUFFERED = (5, 22)    # ... that get fewer events than a buffer holds
DEAD = (1, 9)         # the listener deleted at the end
X = 180               # the latency threshold (ms) of the rank metrics: inside the data
BOTH = (capi.TOPK_LARGEST, capi.TOPK_SMALLEST)


class World:
    def __init__(self, **kw):
        from gyeeta_amd.engine import SketchEngine
        cfg = dict(max_hosts=H, max_services=H * S + 8, max_batch_events=1 << 16, max_clusters=4, td_pend_cap=64, svc_hll_p=4, svc_hll_levels=1)
        cfg.update(kw)
        self.eng = eng = SketchEngine(**cfg)
        for c in ("cluster0", "cluster1", "cluster2"):
            eng.register_cluster(c)
        self.info, self.gids = helpers.register_world(eng, None, range(H), S)
        self.slot = {(h, s): eng.lookup(int(self.gids[h][s])) for h in range(H) for s in range(S)}
        self.by_slot = {v: k for k, v in self.slot.items()}

    def feed(self, rng, scale):
        for h in range(H):
            per = rng.integers(150, 700, S)
            per[list(EMPTY)] = 0
            per[list(BUFFERED)] = rng.integers(3, 20, 2)
            svc = rng.permutation(np.concatenate([np.full(int(per[s]), s, dtype=np.int64) for s in range(S)]))
            lat = lambda sv: np.clip(np.floor(rng.lognormal(3.5, 0.8, len(sv)) * scale[h][sv]), 0, 1e6)
            self.eng.handle_resp_events(self.info[h][0], events_for(rng, h, svc, lat))
        self.eng.sync()


@pytest.fixture(scope="module")
def world(torch_mod):
    rng = np.random.default_rng(31337)
    w = World()
    scale = rng.permutation(np.linspace(0.3, 30.0, H * S)).reshape(H, S)  # per service: the order is known not to be the slot order
    w.feed(rng, scale)
    w.eng.window_close(T0 * 1_000_000 + 5)
    w.feed(rng, scale)
    w.feed(rng, scale)
    assert w.eng.delete_listeners([int(w.gids[DEAD[0]][DEAD[1]])]) == 1
    w.free = w.slot[DEAD]
    w.live = np.array(sorted(s for k, s in w.slot.items() if k != DEAD))
    yield w
    w.eng.close()


def restated(col, cand, eligible, order):
    rows = np.sort(np.asarray(cand, dtype=np.int64))
    rows = rows[eligible[rows] & ~np.isnan(col[rows])]
    v = col[rows] + 0.0
    return rows[np.lexsort((rows, -v if order == capi.TOPK_LARGEST else v))]


def column(w, metric, param, level=-1, tusec=0):
    """(the metric's column from the scans, the totals, the eligibility by data) at this moment"""
    eng = w.eng
    if metric == capi.TOP_DISTINCT:
        col = eng.scan_distinct() if level < 0 else eng.scan_distinct_level(level, tusec)
        return col, np.zeros(len(col), dtype=np.uint64), np.ones(len(col), dtype=bool)
    below, total = eng.scan_ranks([0 if metric == capi.TOP_QUANTILE else int(param)])
    if metric == capi.TOP_QUANTILE:
        col = eng.scan_quantiles([param])[:, 0]
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            col = below[:, 0] / total.astype(np.float64) if metric == capi.TOP_SHARE_WITHIN else total.astype(np.float64) - below[:, 0]
    return col, total, total >= 1


def check(w, got, nel, want, k, col, total, what):
    want_k = want[:k]
    assert nel == len(want), (what, nel, len(want))
    assert got["slot"].tolist() == want_k.tolist(), (what, got["slot"].tolist()[:12], want_k.tolist()[:12])
    assert got["value"].tobytes() == col[want_k].tobytes(), (what, "the values are not the scan's bits")
    assert (got["total"] == total[want_k]).all(), what
    for e in got:
        h, s = w.by_slot[int(e["slot"])]
        assert int(e["glob_id"]) == int(w.gids[h][s]) and int(e["host_slot"]) == w.info[h][1], (what, e)


METRICS = [(capi.TOP_QUANTILE, 0.5, -1), (capi.TOP_QUANTILE, 0.99, -1), (capi.TOP_SHARE_WITHIN, X, -1), (capi.TOP_MISSES, X, -1),
           (capi.TOP_DISTINCT, 0.0, -1), (capi.TOP_DISTINCT, 0.0, 1)]


@pytest.mark.parametrize("metric,param,level", METRICS, ids=["p50", "p99", "share-within", "misses", "distinct-open", "distinct-level-1"])
def test_rankings_equal_the_ordering_of_the_scan(world, metric, param, level):
    w, eng = world, world.eng
    tus = T0 * 1_000_000 + 6
    col, total, has = column(w, metric, param, level, tus)
    digest = metric != capi.TOP_DISTINCT
    nodata = [w.slot[(h, s)] for h in range(H) for s in EMPTY]
    if digest:
        assert not has[nodata].any() and not has[w.free] and has.sum() == H * S - len(nodata) - 1
        share = col[has]
        assert len(np.unique(share)) > 10 and (np.diff(col[w.live][has[w.live]]) < 0).any()  # (an order of its own, not the slot order)
    else:
        assert col[w.live].max() > 0
    for order in BOTH:
        want = restated(col, w.live, has, order)
        assert w.free not in want and (not digest or not set(nodata) & set(want.tolist()))
        for k in (1, 7, H * S + 5):
            got, nel = eng.top_services(metric, param, k=k, order=order, level=level, tusec=tus)
            check(w, got, nel, want, k, col, total, (metric, param, level, order, k))
        if digest:  # min_total cuts the eligible set
            cut = int(np.median(total[has]))
            elig = total >= max(cut, 1)
            assert 0 < elig.sum() < has.sum()
            got, nel = eng.top_services(metric, param, k=H * S, order=order, min_total=cut)
            check(w, got, nel, restated(col, w.live, elig, order), H * S, col, total, ("min_total", metric, order))
        else:  # ... and is not used for the distinct counts
            got, nel = eng.top_services(metric, param, k=H * S + 5, order=order, level=level, tusec=tus, min_total=1 << 40)
            check(w, got, nel, want, H * S + 5, col, total, ("min_total unused", level, order))
        # filters (GYS_RF_ANY_STATE): two of the hosts; ten services by id (one of them deleted: it matches nothing)
        hosts = [0, 2]
        cand = [s for (h, _), s in w.slot.items() if h in hosts and s != w.free]
        got, nel = eng.top_services(metric, param, k=H * S, order=order, level=level, tusec=tus, any_state=True, machine_ids=[w.info[h][0] for h in hosts])
        check(w, got, nel, restated(col, cand, has, order), H * S, col, total, ("two hosts", metric, order))
        assert [x for x in want.tolist() if x in set(cand)] == got["slot"].tolist()  # the unfiltered ordering restricted to those slots
        pick = [(0, 1), (0, 3), (0, 30), (1, 0), (1, 5), DEAD, (1, 39), (2, 2), (2, 17), (2, 22)]
        cand = [w.slot[p] for p in pick if p != DEAD]
        got, nel = eng.top_services(metric, param, k=4, order=order, level=level, tusec=tus, any_state=True, svcids=[int(w.gids[h][s]) for h, s in pick])
        check(w, got, nel, restated(col, cand, has, order), 4, col, total, ("ten svcids", metric, order))
        assert [x for x in want.tolist() if x in set(cand)][:4] == got["slot"].tolist()
    got, nel = eng.top_services(metric, param, k=0, level=level, tusec=tus)
    assert len(got) == 0 and nel == len(want)
    got, nel = eng.top_services(metric, param, k=3, level=level, tusec=tus, any_state=True, svcids=[12345])  # a filter that selects nothing
    assert len(got) == 0 and nel == 0


def test_error_codes(world):
    eng = world.eng
    out = (capi.TopService * 4)()
    nout, nel = C.c_uint32(), C.c_uint64()
    L, h = eng.L, eng.h
    call = lambda metric=0, level=-1, flags=0, order=0, k=4, o=out, f=None: L.gys_top_services(h, metric, 0.5, level, 0, f, flags, 0, order, k, o, C.byref(nout), C.byref(nel))
    assert call() == capi.OK and nout.value == 4
    assert call(metric=4) == capi.ERR_INVAL and call(metric=-1) == capi.ERR_INVAL
    assert call(order=2) == capi.ERR_INVAL
    assert call(metric=capi.TOP_DISTINCT, level=4) == capi.ERR_INVAL and call(metric=capi.TOP_DISTINCT, level=-2) == capi.ERR_INVAL
    assert call(flags=2) == capi.ERR_INVAL
    assert call(o=None) == capi.ERR_INVAL
    assert call(k=0, o=None) == capi.OK and nout.value == 0 and nel.value > 0
    assert call(level=7) == capi.OK  # (level is read by GYS_TOP_DISTINCT only)


@pytest.mark.parametrize("kw,metric,level", [(dict(enable_tdigest=False), capi.TOP_QUANTILE, -1), (dict(enable_tdigest=False), capi.TOP_SHARE_WITHIN, -1),
                                             (dict(enable_tdigest=False), capi.TOP_MISSES, -1), (dict(svc_hll_p=0, svc_hll_levels=0), capi.TOP_DISTINCT, -1),
                                             (dict(svc_hll_levels=0), capi.TOP_DISTINCT, 1)],
                         ids=["p-no-digest", "share-no-digest", "misses-no-digest", "distinct-no-registers", "level-no-levels"])
def test_state_errors(torch_mod, kw, metric, level):
    w = World(**kw)
    with pytest.raises(capi.GysError) as e:
        w.eng.top_services(metric, 0.5, k=3, level=level)
    assert e.value.code == capi.ERR_STATE
    if metric == capi.TOP_DISTINCT and level >= 0:
        assert w.eng.top_services(metric, k=3)[1] == H * S  # the open window's registers are there
    w.eng.close()
