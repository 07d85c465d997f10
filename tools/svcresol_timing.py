"""Timing of the issue resolution ("Issue resolution" in include/gysketch.h) on one GPU, on the graph of tools/groupflow_timing.py:

  * --services (default 10^6) services under 2 hosts, every one bound to a task group of its own; --rows (default 4 * 10^6) live rows
    with distinct (listener, client) keys, --bound (default 0.1) of them naming a bound task group as the client (~4 * 10^5 edges);
  * a kept LISTENER_STATE_NOTIFY record per service: --sources (default 0.03) Bad / Severe / Down with another issue, 0.35 of them with
    the dependent-listener issue, 0.30 OK, the rest Good / Idle but for 0.05 without a record;
  * gys_svc_resolve_issues_dev from the kept states and from a gys_listener_decision array carrying the same states, and per kernel
    the time gys_profile_get reports (a run of its own, the profile switched on);
  * in the same run the nearest call there was before: gys_svc_deps_dev from the same sources, GYS_DEP_CALLERS, max_hops 8 -- the same
    two-pass edge build and as many levels;
  * and the same resolution on the host: gys_svc_edges_dev with every edge written, the copy of the 64-byte rows to the host, and a numpy
    level-by-level search (np.minimum.at over src << 32 | via).  Its records are compared with the device's: the run fails if they differ.

Every figure: 3 warm calls, then --reps (default 11) timed calls; device time between two events on the engine's stream and the call's
wall time (the call synchronised), median and min .. max.  Run from the repository root on a machine with an MI355X:
    python tools/svcresol_timing.py [--services N] [--rows N] [--bound F] [--sources F] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOSLOT = 0xFFFFFFFF


def host_resolution(nsvc, state, issue, has, pu, pv, tiers=8):
    """the definition with numpy: -> (role, tier, src, via, nresolved) per slot"""
    bad = has & (state >= 3) & (state <= 5)
    source, dep, ok = bad & (issue != 7), bad & (issue == 7), has & (state == 2)
    tier = np.full(nsvc, 0xFE, dtype=np.uint8)
    tier[dep | ok] = 0xFF
    tier[source] = 0
    best = np.full(nsvc, np.iinfo(np.uint64).max, dtype=np.uint64)
    src = np.where(source, np.arange(nsvc, dtype=np.uint64), np.uint64(NOSLOT))
    for level in range(tiers):
        m = (tier[pv] == level) & (tier[pu] == 0xFF)
        if not m.any():
            break
        u, v = pu[m], pv[m]
        np.minimum.at(best, u, (src[v] << np.uint64(32)) | v.astype(np.uint64))
        hit = (tier == 0xFF) & (best != np.iinfo(np.uint64).max)
        tier[hit] = level + 1
        src[hit] = best[hit] >> np.uint64(32)
    reached = (tier >= 1) & (tier <= 8)
    role = np.zeros(nsvc, dtype=np.uint8)
    role[source] = 1
    role[dep & reached] = 2
    role[ok & reached] = 3
    role[dep & ~reached] = 4
    nres = np.bincount(src[role == 2].astype(np.int64), minlength=nsvc).astype(np.uint32)
    via = np.where(reached, best & np.uint64(NOSLOT), np.uint64(NOSLOT)).astype(np.uint32)
    srcw = np.where(reached | source, src, np.uint64(NOSLOT)).astype(np.uint32)
    return role, np.where(reached, tier, 0).astype(np.uint8), srcw, via, nres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--bound", type=float, default=0.1)
    ap.add_argument("--sources", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from gyeeta_amd import capi, wire
    from gyeeta_amd.engine import SketchEngine
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing measured")
    cap = 1
    while cap < a.rows:
        cap *= 2
    lines = []
    medians = {}
    nhosts = 2
    svcs = a.services // nhosts
    eng = SketchEngine(max_hosts=nhosts, max_services=nhosts * svcs, enable_tdigest=False, actconn_pair_cap=cap)
    s = np.arange(svcs)
    gids = []
    for h in range(nhosts):
        mid = wire.machine_id(h)
        eng.register_host(mid, "c%d" % h)
        g = wire.glob_id(np.full(svcs, h), s)
        eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
        gids.append(g)
    gids = np.concatenate(gids)
    nsvc = len(gids)
    assert eng.num_services() == nsvc and eng.lookup(int(gids[svcs])) == svcs  # (slots are handed out in order)
    tasks = wire.splitmix64(np.arange(nsvc, dtype=np.uint64) + np.uint64(0x7A5C0000)) | np.uint64(1)
    assert eng.set_listener_tasks(gids, tasks) == capi.OK
    rng = np.random.default_rng(1)
    chunk = 1 << 20
    for first in range(0, a.rows, chunk):  # (the rows of tools/groupflow_timing.py)
        n = min(chunk, a.rows - first)
        rec = np.zeros(n, dtype=wire.ACTIVE_CONN_STATS)
        j = np.arange(first, first + n, dtype=np.uint64)
        rec["listener_glob_id"] = gids[(j % np.uint64(nsvc)).astype(np.int64)]
        caller = ((j // np.uint64(nsvc)) * np.uint64(7919) + j * np.uint64(31) + np.uint64(1)) % np.uint64(nsvc)
        rec["cli_aggr_task_id"] = np.where(rng.random(n) < a.bound, tasks[caller.astype(np.int64)], wire.splitmix64(j + np.uint64(0x51ED)) & ~np.uint64(1))
        rec["bytes_sent"], rec["active_conns"] = 1000, 1
        batch = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(eng.device)
        eng.order()
        capi.check(eng.L.gys_ingest_active_conns_dev(eng.h, C.c_void_p(batch.data_ptr()), n))
        eng.sync()
    # the states: one record per service but for the 5 % without
    r = rng.random(nsvc)
    p_src, p_dep, p_ok = a.sources, a.sources + 0.35, a.sources + 0.65
    state = np.where(r < p_dep, rng.integers(3, 6, nsvc), np.where(r < p_ok, 2, rng.integers(0, 2, nsvc))).astype(np.uint8)
    issue = np.where(r < p_src, rng.integers(0, 7, nsvc), np.where(r < p_dep, 7, 0)).astype(np.uint8)
    has = r < 0.95
    idx = np.flatnonzero(has)
    host_slot = (np.arange(nsvc) // svcs).astype(np.uint32)
    for first in range(0, len(idx), 1 << 18):
        part = idx[first:first + (1 << 18)]
        rec = np.zeros(len(part), dtype=wire.LISTENER_STATE_NOTIFY)
        rec["glob_id"], rec["curr_state"], rec["curr_issue"], rec["nqrys_5s"] = gids[part], state[part], issue[part], 10
        d_rec = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(eng.device)
        d_off = torch.from_numpy((np.arange(len(part), dtype=np.int64) * 88).astype(np.int32)).to(eng.device)
        d_hs = torch.from_numpy(host_slot[part].astype(np.int32)).to(eng.device)
        eng.order()
        capi.check(eng.L.gys_ingest_listener_state_dev(eng.h, C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_void_p(d_hs.data_ptr()), len(part)))
        eng.sync()
    st = eng.svcgraph_stats()
    ne = int(st["edges"])
    lines.append("== %d hosts x %d services, rows %d, bound clients %.2f, actconn_pair_cap %d" % (nhosts, svcs, a.rows, a.bound, cap))
    lines.append("graph: %s" % st)

    def timed(tag, what, fn):
        for _ in range(3):
            fn()
        eng.sync()
        dev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(eng.stream)
            fn()
            e1.record(eng.stream)
            eng.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        lines.append("%-78s device ms median %.3f (min %.3f max %.3f)   wall ms median %.3f (min %.3f max %.3f)   n=%d" % (
            what, np.median(dev), min(dev), max(dev), np.median(wall), min(wall), max(wall), a.reps))
        medians[tag] = (float(np.median(dev)), float(np.median(wall)))

    d_out = torch.zeros((nsvc, 16), dtype=torch.uint8, device=eng.device)
    d_imp = torch.zeros(nsvc, dtype=torch.float64, device=eng.device)
    dec = np.zeros(nsvc, dtype=eng.DECISION_DT)
    dec["state"], dec["issue"] = np.where(has, state, 9), issue
    d_dec = torch.from_numpy(np.frombuffer(dec.tobytes(), dtype=np.uint8).copy()).to(eng.device)
    d_hops = torch.zeros(nsvc, dtype=torch.int32, device=eng.device)
    rst = capi.SvcResolStats()
    eng.order()
    eng.sync()

    def resolve(dp):
        capi.check(eng.L.gys_svc_resolve_issues_dev(eng.h, dp, 0, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_imp.data_ptr()), C.byref(rst)))

    resolve(None)
    stats = eng._resol_stats(rst)
    lines.append("resolution: %s" % stats)
    got = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=eng.SVC_RESOL_DT).copy()
    resolve(C.c_void_p(d_dec.data_ptr()))
    assert np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=eng.SVC_RESOL_DT).tobytes() == got.tobytes() and eng._resol_stats(rst) == stats, "the decision array gives another result"
    timed("kept", "gys_svc_resolve_issues_dev, kept states, records + impact column", lambda: resolve(None))
    timed("dec", "gys_svc_resolve_issues_dev, the same states as a gys_listener_decision array", lambda: resolve(C.c_void_p(d_dec.data_ptr())))
    # the nearest call there was: the reached set of the same sources
    roots = np.ascontiguousarray(gids[np.flatnonzero(got["role"] == capi.RS_SOURCE)], dtype=np.uint64)
    nr = C.c_uint32()

    def deps():
        capi.check(eng.L.gys_svc_deps_dev(eng.h, roots.ctypes.data_as(capi.u64p), len(roots), capi.DEP_CALLERS, 8, C.c_void_p(d_hops.data_ptr()), C.byref(nr)))

    timed("deps", "gys_svc_deps_dev from the %d sources, GYS_DEP_CALLERS, max_hops 8" % len(roots), deps)
    lines.append("  (it reaches %d services, sources included; whatever their state)" % nr.value)
    # the same resolution on the host
    rows_dev = torch.empty((max(ne, 1), 64), dtype=torch.uint8, device=eng.device)
    rows_host = torch.empty((max(ne, 1), 64), dtype=torch.uint8).pin_memory()
    nm = C.c_uint32()
    eng.order()
    res = {}

    def on_host():
        capi.check(eng.L.gys_svc_edges_dev(eng.h, None, C.c_void_p(rows_dev.data_ptr()), ne, C.byref(nm)))
        with torch.cuda.stream(eng.stream):
            rows_host.copy_(rows_dev, non_blocking=True)
        eng.sync()
        e = np.frombuffer(rows_host.numpy().tobytes(), dtype=eng.SVC_EDGE_DT)[:nm.value]
        res["r"] = host_resolution(nsvc, state, issue, has, e["src_slot"].astype(np.int64), e["dst_slot"].astype(np.int64))

    timed("host", "gys_svc_edges_dev + copy to the host + numpy level-by-level resolution", on_host)
    role, tier, src, via, nres = res["r"]
    same = (got["role"] == role).all() and (got["tier"] == tier).all() and (got["src_slot"] == src).all() and (got["via_slot"] == via).all() and (got["nresolved"] == np.where(role == 1, nres, 0)).all()
    assert same, "the host resolution differs from the device's"
    lines.append("  (the host resolution gives the same %d records)" % nsvc)
    # per kernel: the profile on, a run of its own
    eng.profile(True)
    eng.profile_reset()
    for _ in range(a.reps):
        resolve(None)
    eng.sync()
    prof = eng.profile_get()
    eng.profile(False)
    lines.append("per kernel over %d profiled calls (gys_profile_get: ms per call, launches per call):" % a.reps)
    for name in ("dep_edges", "resol_seed", "resol_level", "resol_settle", "resol_finish"):
        ms, n = prof.get(name, (0.0, 0))
        lines.append("  %-14s %.3f ms   %d launches" % (name, ms / a.reps, n // a.reps))
    lines.append("")
    k, d, h = medians["kept"], medians["deps"], medians["host"]
    lines.append("resolution %.3f ms device / %.3f ms wall;   gys_svc_deps_dev %.3f / %.3f ms: ratio %.2f (device) %.2f (wall);   on the host %.3f ms wall: %.1f x" % (
        k[0], k[1], d[0], d[1], k[0] / d[0], k[1] / d[1], h[1], h[1] / k[1]))
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
