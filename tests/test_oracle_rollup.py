"""The roll-up oracle (oracle/gy_oracle_rollup.c: 64-bit counters) against the per-service digest oracle it extends (oracle/gy_oracle.c,
32-bit counters): with weights that fit both, the two must agree cluster for cluster -- merging values, merging a digest's clusters, and
quantiles -- so that the GPU roll-up's bit-exactness against the 64-bit form is also bit-exactness against the pinned 32-bit definition.
Plus the properties a roll-up must have: totals add up, min / max cover the members.  Round 6: the roll-up itself is the union by value
bin (gyo_tdbins_*): its finish against a point-by-point restatement, conservation, independence of the members' order, rank error."""
import ctypes as C

import numpy as np
import pytest


def _vals(rng, n, mu=3.0):
    return np.ascontiguousarray(np.minimum(np.floor(rng.lognormal(mu, 1.5, n)), 1e6).astype(np.int32))


def _td_equal(L, d32, d64):
    return list(d32.sum) == list(d64.sum) and [int(c) for c in d32.cnt] == [int(c) for c in d64.cnt]


def test_td64_matches_td32_on_values_and_digest_merges(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(5)
    for trial in range(20):
        a32, a64 = oracle.TDigest(), oracle.TD64()
        L.gyo_td_init(C.byref(a32))
        L.gyo_td64_init(C.byref(a64))
        for _ in range(int(rng.integers(1, 6))):  # several value merges in a row
            v = _vals(rng, int(rng.integers(1, 3000)), mu=float(rng.normal(3, 1)))
            L.gyo_td_merge_values(C.byref(a32), oracle.ptr(v, oracle.i32p), len(v))
            L.gyo_td64_merge_values(C.byref(a64), oracle.ptr(v, oracle.i32p), len(v))
            assert _td_equal(L, a32, a64) and a32.vmin == a64.vmin and a32.vmax == a64.vmax
        # another digest's clusters as weighted points: gyo_td_merge_digest vs the service form with an empty buffer
        b = oracle.TDBuffered()
        L.gyo_tdb_init(C.byref(b))
        v = _vals(rng, 2500, mu=float(rng.normal(3, 1)))
        L.gyo_td_merge_values(C.byref(b.d), oracle.ptr(v, oracle.i32p), len(v))
        L.gyo_td_merge_digest(C.byref(a32), C.byref(b.d))
        L.gyo_td64_merge_service(C.byref(a64), C.byref(b))
        assert _td_equal(L, a32, a64) and a32.vmin == a64.vmin and a32.vmax == a64.vmax
        for q in (0.0, 0.01, 0.5, 0.95, 0.999, 1.0):
            assert L.gyo_td_quantile(C.byref(a32), q) == L.gyo_td64_quantile(C.byref(a64), q)


def test_td64_service_merge_is_clusters_then_buffer(oracle):
    """a service contributes its clusters first and its buffered values second: equal to doing the two steps by hand (the buffer is
    merged into the GROUP digest, not into the member's own)"""
    L = oracle.lib()
    rng = np.random.default_rng(6)
    b = oracle.TDBuffered()
    L.gyo_tdb_init(C.byref(b))
    for n in (500, 500, 300):  # 500 buffered, 1000 > 896: one merge, then 300 buffered
        v = _vals(rng, n)
        L.gyo_tdb_add_batch(C.byref(b), oracle.ptr(v, oracle.i32p), len(v))
    assert b.npend == 300 and L.gyo_td_total(C.byref(b.d)) == 1000
    seed = _vals(rng, 4000, mu=2.0)
    g1, g2 = oracle.TD64(), oracle.TD64()
    for g in (g1, g2):
        L.gyo_td64_init(C.byref(g))
        L.gyo_td64_merge_values(C.byref(g), oracle.ptr(seed, oracle.i32p), len(seed))
    L.gyo_td64_merge_service(C.byref(g1), C.byref(b))
    clusters_only = oracle.TDBuffered()
    L.gyo_tdb_init(C.byref(clusters_only))
    clusters_only.d = b.d
    L.gyo_td64_merge_service(C.byref(g2), C.byref(clusters_only))
    pend = np.ascontiguousarray(np.array(b.pend[:b.npend], dtype=np.int32))
    L.gyo_td64_merge_values(C.byref(g2), oracle.ptr(pend, oracle.i32p), len(pend))
    assert list(g1.sum) == list(g2.sum) and list(g1.cnt) == list(g2.cnt) and g1.vmin == g2.vmin and g1.vmax == g2.vmax
    assert L.gyo_td64_total(C.byref(g1)) == 4000 + L.gyo_tdb_total(C.byref(b))


def test_td64_rollup_totals_minmax_and_rank_error(oracle):
    """a group of 300 services with different scales: the roll-up's weight is the sum of the members', its extremes cover theirs, and
    its quantiles rank within 1 % of the pooled exact sort (the group digest is as good as a service's)"""
    L = oracle.lib()
    rng = np.random.default_rng(7)
    g = oracle.TD64()
    L.gyo_td64_init(C.byref(g))
    pooled = []
    for s in range(300):
        b = oracle.TDBuffered()
        L.gyo_tdb_init(C.byref(b))
        mu = float(rng.normal(3, 1))
        for _ in range(int(rng.integers(1, 5))):
            v = _vals(rng, int(rng.integers(50, 900)), mu=mu)
            pooled.append(v)
            L.gyo_tdb_add_batch(C.byref(b), oracle.ptr(v, oracle.i32p), len(v))
        L.gyo_td64_merge_service(C.byref(g), C.byref(b))
    x = np.sort(np.concatenate(pooled))
    assert L.gyo_td64_total(C.byref(g)) == len(x) and g.vmin == int(x[0]) and g.vmax == int(x[-1])
    for q in (0.05, 0.25, 0.5, 0.9, 0.99):
        v = L.gyo_td64_quantile(C.byref(g), q)
        lo, hi = np.searchsorted(x, v, side="left") / len(x), np.searchsorted(x, v, side="right") / len(x)
        err = 0.0 if lo <= q <= hi else min(abs(lo - q), abs(hi - q))
        assert err <= 0.01, (q, v, err)


# ---------------------------------------------------------------- round 6: the roll-up is the union by value bin (gyo_tdbins_*)
def _rank_err(x, v, q):
    lo, hi = np.searchsorted(x, v, side="left") / len(x), np.searchsorted(x, v, side="right") / len(x)
    return 0.0 if lo <= q <= hi else min(abs(lo - q), abs(hi - q))


def test_value_bins_cover_the_domain_in_order(oracle):
    L = oracle.lib()
    v = np.arange(0, 1 << 20, dtype=np.uint32)
    b = np.array([L.gyo_td_value_bin(int(x)) for x in v[:: 7]])
    assert (np.diff(b) >= 0).all() and b[0] == 0
    assert [L.gyo_td_value_bin(x) for x in (0, 1, 1023, 1024, 1039, 1040, 2047, 2048)] == [0, 1, 1023, 1024, 1024, 1025, 1087, 1088]
    assert L.gyo_td_value_bin((1 << 26) - 1) == oracle.TD_BINS - 1 == L.gyo_td_value_bin(0xFFFFFFFF)
    # a cell is at most 1 / 64 of its lower edge wide
    for x in (1024, 5000, 99999, 1 << 19):
        k = L.gyo_td_value_bin(x)
        same = [y for y in range(x, x + x // 32) if L.gyo_td_value_bin(y) == k]
        assert len(same) <= x // 64 + 1


def _bin_edges(k):
    """lower edge and log2 of the width of value bin k >= 1024 (64 cells per octave)"""
    sh = 4 + (k - 1024) // 64
    return (64 + (k - 1024) % 64) << sh, sh


def test_tdbins_refined_finish_equals_the_point_by_point_restatement(oracle):
    """gyo_tdbins_add_* + gyo_tdbins_finish against the definition spelled out in Python from the items themselves: the bins' totals; the
    marked bins (1024 and above, cut by a cluster boundary, more than 1 / 1024 of the weight) and their fine cells; the units (a bin, or the
    cells of a marked bin) laid on the rank axis in order, every unit mid-point getting its cluster from gyo_td_cluster, a unit's sum shared by
    floor(sum r1 / w) - floor(sum r0 / w) over the runs of equal cluster (Python integers)"""
    L = oracle.lib()
    rng = np.random.default_rng(11)
    for case in range(8):
        b = oracle.TDBins()
        L.gyo_tdbins_init(C.byref(b))
        if case < 4:
            v = _vals(rng, int(rng.integers(1, 4000)), mu=float(rng.uniform(0.5, 8.0)))
        else:  # few heavy values in wide bins: cluster boundaries cut them, the cells carry the shape inside the bin
            centers = rng.choice([1500, 2100, 30000, 250000, 602000], int(rng.integers(1, 4)), replace=False)
            v = np.concatenate([rng.normal(c, c / 300, int(rng.integers(500, 2500))) for c in centers] + [_vals(rng, int(rng.integers(0, 300)))])
            v = np.ascontiguousarray(np.clip(v, 0, 1e6).astype(np.int32))
        rng.shuffle(v)
        # (a group's items in two members: one adds values, the other a digest whose clusters go in at the integer threshold of their mean)
        cut = len(v) // 2
        side = oracle.TD64()
        L.gyo_td64_init(C.byref(side))
        L.gyo_td64_merge_values(C.byref(side), oracle.ptr(np.ascontiguousarray(v[cut:]), oracle.i32p), len(v) - cut)
        items = [(int(x), int(x), 1) for x in v[:cut]]
        items += [(-(-int(side.sum[j]) // int(side.cnt[j])), int(side.sum[j]), int(side.cnt[j])) for j in range(oracle.TD_NB) if side.cnt[j]]
        head = np.ascontiguousarray(v[:cut])
        L.gyo_tdbins_add_values(C.byref(b), oracle.ptr(head, oracle.i32p), len(head))
        L.gyo_tdbins_add_td64(C.byref(b), C.byref(side))
        out = oracle.TD64()
        L.gyo_tdbins_finish(C.byref(b), C.byref(out))
        # restatement: bins
        bins = {}
        for at, sm, cn in items:
            k = L.gyo_td_value_bin(min(at, (1 << 26) - 1))
            bins.setdefault(k, []).append((at, sm, cn))
        N = sum(cn for _, _, cn in items)
        assert [int(b.cnt[k]) for k in sorted(bins)] == [sum(cn for _, _, cn in bins[k]) for k in sorted(bins)]
        # marks
        W, marked = 0, []
        for k in sorted(bins):
            w = sum(cn for _, _, cn in bins[k])
            if k >= 1024 and w > N // 1024 and L.gyo_td_cluster(2 * W + 1, 2 * N) != L.gyo_td_cluster(2 * (W + w - 1) + 1, 2 * N):
                marked.append(k)
            W += w
        per = 1920 // len(marked) if marked else 0
        if case >= 4:
            assert marked, case
        # units in order
        units = []
        for k in sorted(bins):
            if k not in marked:
                units.append((sum(cn for _, _, cn in bins[k]), sum(sm for _, sm, _ in bins[k])))
                continue
            lo, sh = _bin_edges(k)
            nc = min(per, 1 << sh)
            cells = [[0, 0] for _ in range(nc)]
            for at, sm, cn in bins[k]:
                c = ((min(at, (1 << 26) - 1) - lo) * nc) >> sh
                cells[c][0] += cn
                cells[c][1] += sm
            units += [tuple(c) for c in cells]
        want_s, want_c, W = [0] * oracle.TD_NB, [0] * oracle.TD_NB, 0
        for w, sm in units:
            if not w:
                continue
            cl = [L.gyo_td_cluster(2 * (W + r) + 1, 2 * N) for r in range(w)]
            r0 = 0
            for r in range(1, w + 1):
                if r == w or cl[r] != cl[r0]:
                    want_s[cl[r0]] += sm * r // w - sm * r0 // w
                    want_c[cl[r0]] += r - r0
                    r0 = r
            W += w
        assert list(out.cnt) == want_c and list(out.sum) == want_s, case
        assert sum(out.sum) == sum(b.sum) == int(v.astype(np.int64).sum()) and sum(out.cnt) == N == len(v)


@pytest.mark.parametrize("name,nsvc,mus,sig", [("mixed", 300, (3, 1), 0.8), ("tight", 300, (1.5, 0.1), 0.3), ("seconds", 200, (7.5, 0.5), 1.0),
                                               ("one-heavy-value", 300, (0.7, 0.05), 0.2)])
def test_tdbins_rollup_totals_order_and_rank_error(oracle, name, nsvc, mus, sig):
    """a group of services rolled up by value bin: weight and sum of the members are conserved exactly, the extremes cover theirs, the
    order of the members does not matter, and the quantiles rank within 1 % of the pooled exact sort (tolerance of the per-service
    digests; here: a few 10^-4) -- on one level and on two (services -> 10 host slabs -> one)"""
    L = oracle.lib()
    rng = np.random.default_rng(7)
    svcs, pooled = [], []
    for s in range(nsvc):
        b = oracle.TDBuffered()
        L.gyo_tdb_init(C.byref(b))
        mu = float(rng.normal(*mus))
        for _ in range(int(rng.integers(1, 6))):
            v = np.ascontiguousarray(np.clip(rng.lognormal(mu, sig, int(rng.integers(50, 900))), 0, 1e6).astype(np.int32))
            pooled.append(v)
            L.gyo_tdb_add_batch(C.byref(b), oracle.ptr(v, oracle.i32p), len(v))
        svcs.append(b)
    x = np.sort(np.concatenate(pooled))
    one = oracle.rollup_services(svcs)
    assert L.gyo_td64_total(C.byref(one)) == len(x) and sum(one.sum) == int(x.sum()) and one.vmin == int(x[0]) and one.vmax == int(x[-1])
    rev = oracle.rollup_services(svcs[::-1])
    assert list(rev.sum) == list(one.sum) and list(rev.cnt) == list(one.cnt)
    hosts = [oracle.rollup_services(svcs[h::10]) for h in range(10)]
    two = oracle.rollup_slabs(hosts)
    assert L.gyo_td64_total(C.byref(two)) == len(x) and sum(two.sum) == int(x.sum()) and two.vmin == int(x[0]) and two.vmax == int(x[-1])
    # the clusters' means rise with the bins; the pieces of ONE bin that is cut by cluster boundaries carry integer shares of its sum, so their
    # means differ by less than one unit per point of the piece among themselves (all of them lie inside the bin)
    means = np.array([s_ / c_ for s_, c_ in zip(one.sum, one.cnt) if c_])
    assert (np.diff(means) > -np.maximum(1.0, means[1:] / 64)).all()
    assert np.abs(np.diff(means)[np.diff(means) < 0]).sum() < 1.0 + means[-1] / 64
    for q in (0.01, 0.05, 0.25, 0.5, 0.9, 0.95, 0.99, 0.999):
        for d in (one, two):
            v = L.gyo_td64_quantile(C.byref(d), q)
            assert _rank_err(x, v, q) <= 0.01, (name, q, v)


# ---------------------------------------------------------------- the roll-up against the exact sort: narrow ranges, edges, several levels
QS = [0.001, 0.01] + [round(0.05 * i, 2) for i in range(1, 20)] + [0.99, 0.999]


def _ms(x):
    return np.ascontiguousarray(np.clip(np.floor(x), 0, 1e6).astype(np.int32))


# name -> values of one batch of n for the service (rank r, host h, service s): the distributions of the issue's matrix
DISTS = {
    "uniform-1024-1040": lambda rng, n, r, h, s: rng.integers(1024, 1041, n),
    "normal-1500-3": lambda rng, n, r, h, s: rng.normal(1500, 3, n),
    "lognormal-7.3-0.01": lambda rng, n, r, h, s: rng.lognormal(7.3, 0.01, n),
    "normal-30000-100": lambda rng, n, r, h, s: rng.normal(30000, 100, n),
    "uniform-600000-605000": lambda rng, n, r, h, s: rng.integers(600000, 605001, n),
    # a fleet at a fixed 1.5 s with one fast service
    "mixed-fleet": lambda rng, n, r, h, s: rng.lognormal(1, 0.5, n) if s == 0 else rng.normal(1500, 3, n),
    "constant": lambda rng, n, r, h, s: np.full(n, 1500),
    # (the jump between the two masses sits off the q grid: where a jump meets a grid q, the answer interpolated across the cluster that
    # straddles it is off by up to half a cluster -- ~0.9 % at the median for a service's own digest (50 / 50), the quantile scan's limit)
    "two-point": lambda rng, n, r, h, s: rng.choice([5, 5000], n, p=[0.325, 0.675]),
    # odd hosts bimodal with nothing in 100 ... 1000 ms, even hosts fill the gap
    "gap-fill": lambda rng, n, r, h, s: (np.where(rng.random(n) < 0.5, rng.uniform(1, 100, n), rng.uniform(1000, 3000, n)) if h % 2
                                         else rng.uniform(100, 1000, n)),
    # each rank's values an octave and a half above the last
    "rank-heterogeneous": lambda rng, n, r, h, s: rng.lognormal(3 + 1.5 * np.log(2) * r, 0.4, n),
    "uniform-0-1e6": lambda rng, n, r, h, s: rng.integers(0, 1000001, n),
    "lognormal-3-1": lambda rng, n, r, h, s: rng.lognormal(3, 1, n),
    # the domain's edges: 0, the last one-value bin, the first wide bin, the largest latency the engine accepts, on a wide background
    "edges": lambda rng, n, r, h, s: np.where(rng.random(n) < 0.96, rng.lognormal(6, 2.5, n), rng.choice([0, 1023, 1024, 1000000], n)),
}


def _service(oracle, rng, dist, r, h, s, nbatch, n):
    """a service fed nbatch batches of n values of `dist`: (its TDBuffered, its values)"""
    L = oracle.lib()
    b = oracle.TDBuffered()
    L.gyo_tdb_init(C.byref(b))
    vals = []
    for _ in range(nbatch):
        v = _ms(DISTS[dist](rng, n, r, h, s))
        vals.append(v)
        L.gyo_tdb_add_batch(C.byref(b), oracle.ptr(v, oracle.i32p), len(v))
    return b, np.concatenate(vals)


def _check_level(oracle, what, d, again, pooled):
    """one roll-up digest d against the exact sort of the values it stands for: count, sum, min and max exactly, the same digest from the
    members in another order (again), every quantile within 1 % in rank, q = 0 / 1 the extremes"""
    L = oracle.lib()
    x = np.sort(pooled)
    assert L.gyo_td64_total(C.byref(d)) == len(x) and sum(d.sum) == int(x.astype(np.int64).sum()), what
    assert (d.vmin, d.vmax) == (int(x[0]), int(x[-1])), what
    assert list(again.sum) == list(d.sum) and list(again.cnt) == list(d.cnt) and (again.vmin, again.vmax) == (d.vmin, d.vmax), what
    assert L.gyo_td64_quantile(C.byref(d), 0.0) == x[0] and L.gyo_td64_quantile(C.byref(d), 1.0) == x[-1], what
    worst = max((_rank_err(x, L.gyo_td64_quantile(C.byref(d), q), q), q) for q in QS)
    assert worst[0] <= 0.01, (what, "rank error %.4f at q %g" % worst)


GROUPS = [  # (distribution, services): every row of the issue's first table, then the other distributions, one group of 3 x 2 000 values each
    ("uniform-1024-1040", 20), ("normal-1500-3", 20), ("normal-1500-3", 1), ("lognormal-7.3-0.01", 50), ("normal-30000-100", 20),
    ("uniform-600000-605000", 20), ("mixed-fleet", 20), ("constant", 10), ("two-point", 10), ("gap-fill", 20), ("rank-heterogeneous", 20),
    ("uniform-0-1e6", 20), ("lognormal-3-1", 20), ("edges", 10),
]


@pytest.mark.parametrize("dist,nsvc", GROUPS, ids=["%s-x%d" % g for g in GROUPS])
def test_tdbins_group_against_the_exact_sort(oracle, dist, nsvc):
    """one group of services (a host slab): quantiles within 1 % in rank of the pooled exact sort, exact totals and extremes, any order"""
    rng = np.random.default_rng(GROUPS.index((dist, nsvc)) + 20)
    svcs, vals = zip(*[_service(oracle, rng, dist, s % 4, s, s, 3, 2000) for s in range(nsvc)])
    d = oracle.rollup_services(list(svcs))
    _check_level(oracle, "%s x %d" % (dist, nsvc), d, oracle.rollup_services(list(svcs)[::-1]), np.concatenate(vals))


@pytest.mark.parametrize("dist", sorted(DISTS))
def test_tdbins_chain_against_the_exact_sort(oracle, dist):
    """the whole chain: services -> host slabs -> cluster slabs and the rank's global slab (from the hosts, as gys_tdigest_rollup_dev) -> the
    ranks' global slabs -> all (as gys_tdigest_merge_slabs_dev); and the four-level form hosts -> clusters -> rank -> all.  4 ranks x 6 hosts
    (3 clusters) x 4 services: every level within 1 % in rank of the exact sort of what it stands for, totals and extremes exact, any order"""
    R, H, S = 4, 6, 4
    rng = np.random.default_rng(sorted(DISTS).index(dist) + 40)
    ranks, ranks4, rank_vals = [], [], []
    for r in range(R):
        hosts, host_vals = [], []
        for h in range(H):
            svcs, vals = zip(*[_service(oracle, rng, dist, r, h, s, 3, 600) for s in range(S)])
            hosts.append(oracle.rollup_services(list(svcs)))
            host_vals.append(np.concatenate(vals))
            _check_level(oracle, "%s rank %d host %d" % (dist, r, h), hosts[-1], oracle.rollup_services(list(svcs)[::-1]), host_vals[-1])
        clusters = []
        for cl in range(3):
            mem = [hosts[h] for h in range(H) if h % 3 == cl]
            clusters.append(oracle.rollup_slabs(mem))
            _check_level(oracle, "%s rank %d cluster %d" % (dist, r, cl), clusters[-1], oracle.rollup_slabs(mem[::-1]),
                         np.concatenate([host_vals[h] for h in range(H) if h % 3 == cl]))
        rank_vals.append(np.concatenate(host_vals))
        ranks.append(oracle.rollup_slabs(hosts))
        _check_level(oracle, "%s rank %d global" % (dist, r), ranks[-1], oracle.rollup_slabs(hosts[::-1]), rank_vals[-1])
        ranks4.append(oracle.rollup_slabs(clusters))
        _check_level(oracle, "%s rank %d from its clusters" % (dist, r), ranks4[-1], oracle.rollup_slabs(clusters[::-1]), rank_vals[-1])
    pooled = np.concatenate(rank_vals)
    _check_level(oracle, "%s all ranks" % dist, oracle.rollup_slabs(ranks), oracle.rollup_slabs(ranks[::-1]), pooled)
    _check_level(oracle, "%s all ranks, four levels" % dist, oracle.rollup_slabs(ranks4), oracle.rollup_slabs(ranks4[::-1]), pooled)


@pytest.mark.parametrize("dist", sorted(DISTS))
def test_tdbins_one_service_group_answers_as_the_service(oracle, dist):
    """the roll-up of a group of one service answers, at every q, within 1 % in rank (in the service's exact sort) of the service's own
    gyo_tdb_quantile -- with values still buffered and without"""
    L = oracle.lib()
    rng = np.random.default_rng(sorted(DISTS).index(dist) + 80)
    for nbatch, n in ((3, 2000), (5, 700), (1, 300)):
        b, vals = _service(oracle, rng, dist, 1, 1, 1, nbatch, n)
        x = np.sort(vals)
        d = oracle.rollup_services([b])
        for q in QS + [0.0, 1.0]:
            mine, own = L.gyo_td64_quantile(C.byref(d), q), L.gyo_tdb_quantile(C.byref(b), q)
            lo1, hi1 = np.searchsorted(x, mine, "left") / len(x), np.searchsorted(x, mine, "right") / len(x)
            lo2, hi2 = np.searchsorted(x, own, "left") / len(x), np.searchsorted(x, own, "right") / len(x)
            assert max(0.0, lo1 - hi2, lo2 - hi1) <= 0.01, (dist, nbatch, n, q, mine, own)


def test_active_conn_and_pair_oracles_against_numpy(oracle):
    from gyeeta_amd import wire
    L = oracle.lib()
    rng = np.random.default_rng(8)
    rec = wire.synth_active_conns(rng, 3000, 2, 9)
    p32 = np.zeros((4, 65536), dtype=np.uint32)
    p64 = np.zeros((4, 65536), dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint64)
    buf = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    L.gyo_active_conn_sketch_batch(oracle.ptr(buf, oracle.u8p), len(rec), oracle.ptr(p32, oracle.u32p), oracle.ptr(p64, oracle.u64p), oracle.ptr(out, oracle.u64p))
    local = (rec["flags"] & wire.ACTIVE_FLAG_REMOTE_LISTEN) == 0
    assert out.tolist() == [int(local.sum()), int((~local).sum())]
    assert p32.sum(axis=1).tolist() == [int(rec["active_conns"][local].sum())] * 4
    assert p64.sum(axis=1).tolist() == [int(rec["bytes_sent"][local].sum() + rec["bytes_received"][local].sum())] * 4
    # Count-Min never under-estimates: a pair's estimate (min over the rows) >= its exact total
    g, t = int(rec["listener_glob_id"][local][0]), int(rec["cli_aggr_task_id"][local][0])
    w = np.array([g & 0xFFFFFFFF, g >> 32, t & 0xFFFFFFFF, t >> 32], dtype=np.uint32)
    est = L.gyo_cms_query(oracle.ptr(p32, oracle.u32p), oracle.ptr(w, oracle.u32p), 4)
    sel = local & (rec["listener_glob_id"] == g) & (rec["cli_aggr_task_id"] == t)
    assert est >= int(rec["active_conns"][sel].sum())
