"""The roll-up digests on the device against the EXACT SORT of what they stand for: response events with chosen latencies go through
SketchEngine (several engines stand in for the ranks of a job), and every level -- host, cluster and global slabs (gys_tdigest_rollup_dev),
the ranks' global slabs rolled up (gys_tdigest_merge_slabs_dev) -- answers every quantile within 1 % in rank of the numpy sort of the
accepted latencies (lsndtime - lrcvtime <= 10^6 on a registered listener), with exact totals and extremes; and stays bit-exact with the
oracle (oracle/gy_oracle_rollup.c) on the way.  Narrow ranges in wide value bins (1.5 s, 600 s), a mixed fleet, point masses and the
domain's edges, buffers of 896 and of 1 920 values."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

QS = [0.001, 0.01] + [round(0.05 * i, 2) for i in range(1, 20)] + [0.99, 0.999]
R, H, S = 3, 6, 4  # ranks (engines), hosts per rank (clusters: host % 3), services per host


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _lat(rng, dist, r):
    """the latencies (ms) of n events for the drawn service indices s of rank r"""
    def f(s):
        n = len(s)
        if dist == "normal-1500-3":
            v = rng.normal(1500, 3, n)
        elif dist == "uniform-600000-605000":
            v = rng.integers(600000, 605001, n)
        elif dist == "mixed-fleet":  # one fast service among services at a fixed 1.5 s
            v = np.where(s == 0, rng.lognormal(1, 0.5, n), rng.normal(1500, 3, n))
        elif dist == "two-point":  # (the jump off the q grid, as in tests/test_oracle_rollup.py)
            v = rng.choice([5, 5000], n, p=[0.325, 0.675])
        elif dist == "rank-heterogeneous":  # each rank an octave and a half above the last
            v = rng.lognormal(3 + 1.5 * np.log(2) * r, 0.4, n)
        else:  # "edges": 0, 1023, 1024 and 10^6 (the largest latency accepted) on a wide background
            v = np.where(rng.random(n) < 0.96, rng.lognormal(6, 2.5, n), rng.choice([0, 1023, 1024, 1000000], n))
        return np.clip(np.floor(v), 0, 1e6)
    return f


def _accepted(ev):
    lat = (ev["lsndtime"].astype(np.uint32) - ev["lrcvtime"].astype(np.uint32)).astype(np.uint32)
    return lat[(lat <= 1000000) & (ev["sport_be"] != 999)].astype(np.int64)


def _rank_err(x, v, q):
    lo, hi = np.searchsorted(x, v, side="left") / len(x), np.searchsorted(x, v, side="right") / len(x)
    return 0.0 if lo <= q <= hi else min(abs(lo - q), abs(hi - q))


def _same_slab(rec, d):
    return bool((rec["sum"] == np.array(d.sum[:], dtype=np.int64)).all() and (rec["cnt"] == np.array(d.cnt[:], dtype=np.uint64)).all()
                and int(rec["vmin"]) == d.vmin and int(rec["vmax"]) == d.vmax)


def _check(what, eng, dev, index, rec, pooled):
    x = np.sort(pooled)
    assert int(rec["cnt"].sum()) == len(x) and int(rec["sum"].sum()) == int(x.sum()), what
    assert (int(rec["vmin"]), int(rec["vmax"])) == (int(x[0]), int(x[-1])), what
    got = eng.slab_quantiles(dev, QS + [0.0, 1.0], index)
    assert got[-2:] == [float(x[0]), float(x[-1])], what
    worst = max((_rank_err(x, v, q), q, v) for v, q in zip(got, QS))
    assert worst[0] <= 0.01, (what, "rank error %.4f at q %g (value %g)" % worst)


CASES = [("normal-1500-3", 0), ("normal-1500-3", 1920), ("uniform-600000-605000", 1920), ("mixed-fleet", 0), ("two-point", 1920),
         ("rank-heterogeneous", 0), ("edges", 1920)]


@pytest.mark.parametrize("dist,td_cap", CASES, ids=["%s-cap%d" % c for c in CASES])
def test_rollup_levels_against_the_exact_sort(torch_mod, oracle, dist, td_cap):
    from gyeeta_amd import capi
    from gyeeta_amd.engine import SketchEngine
    torch = torch_mod
    rng = np.random.default_rng(CASES.index((dist, td_cap)) + 700)
    globals_dev, globals_orc, rank_vals, buffered = [], [], [], 0
    eng = None
    for r in range(R):
        if eng is not None:
            eng.close()
        eng = SketchEngine(max_hosts=H, max_services=H * S, max_batch_events=1 << 16, max_clusters=4, td_pend_cap=td_cap)
        orc = oracle.OracleEngine(H * S, td_cap=td_cap)
        for cname in ("cluster0", "cluster1", "cluster2"):
            eng.register_cluster(cname)
        info, _ = helpers.register_world(eng, orc, range(H), S)
        host_vals = [[] for _ in range(H)]
        for rnd in range(3):
            for h in range(H):
                ev = helpers.make_resp_events(rng, h, int(rng.integers(1500, 4000)), S, lat=_lat(rng, dist, r))
                eng.handle_resp_events(info[h][0], ev)
                orc.resp_batch(ev.tobytes(), [info[h][1]], [0])
                host_vals[h].append(_accepted(ev))
        eng.sync()
        host_vals = [np.concatenate(v) for v in host_vals]
        buffered = max(buffered, max(orc.td(i).npend for i in range(H * S)))
        hosts = [oracle.rollup_services([orc.td(h * S + k) for k in range(S)]) for h in range(H)]
        dev_h, rec_h = eng.tdigest_rollup(capi.ROLLUP_HOST)
        for h in range(H):
            assert _same_slab(rec_h[h], hosts[h]), f"{dist} rank {r}: host slab {h} differs from the oracle's"
            _check(f"{dist} rank {r} host {h}", eng, dev_h, h, rec_h[h], host_vals[h])
        dev_c, rec_c = eng.tdigest_rollup(capi.ROLLUP_CLUSTER)
        for cl in range(3):
            assert _same_slab(rec_c[cl], oracle.rollup_slabs([hosts[h] for h in range(H) if h % 3 == cl])), f"{dist} rank {r}: cluster slab {cl}"
            _check(f"{dist} rank {r} cluster {cl}", eng, dev_c, cl, rec_c[cl], np.concatenate([host_vals[h] for h in range(H) if h % 3 == cl]))
        dev_g, rec_g = eng.tdigest_rollup(capi.ROLLUP_GLOBAL)
        globals_orc.append(oracle.rollup_slabs(hosts))
        assert _same_slab(rec_g[0], globals_orc[-1]), f"{dist} rank {r}: global slab"
        rank_vals.append(np.concatenate(host_vals))
        _check(f"{dist} rank {r} global", eng, dev_g, 0, rec_g[0], rank_vals[-1])
        globals_dev.append(dev_g.clone())
    # all ranks: the ranks' global slabs side by side (as the all-gather leaves them), rolled up
    allg = torch.cat(globals_dev)
    dev_a, rec_a = eng.tdigest_merge_slabs(allg, R)
    want = oracle.rollup_slabs(globals_orc)
    assert _same_slab(rec_a, want), f"{dist}: the ranks' roll-up"
    _check(f"{dist} all ranks", eng, dev_a, 0, rec_a, np.concatenate(rank_vals))
    assert eng.slab_quantiles(dev_a, QS) == [oracle.lib().gyo_td64_quantile(C.byref(want), q) for q in QS]
    if td_cap == 0 or dist == "edges":
        assert buffered > 64  # (the buffers hold values when the roll-up runs: the buffered-value path of both passes)
    eng.close()
