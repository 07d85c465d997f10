"""Timing of the service dependency graph ("Service dependency graph" in include/gysketch.h) on one GPU:

  * --hosts x --svcs services (default 1000 x 1000 = 10^6), every one bound to a task group of its own; --rows (default 4 * 10^6) live
    rows with distinct (listener, client) keys, --bound (default 0.1) of them naming a bound task group as the client, the rest a client
    that is bound to nothing;
  * the edge build: gys_svcgraph_stats (one walk of the table: the count and the counters) and gys_svc_edges_dev with every row written;
  * gys_svc_deps_dev from --roots (default 16) roots: 3 hops, and without a limit; the levels one by one as the difference between
    max_hops = h and max_hops = h - 1 (every such call builds the pair array anew: two walks of the table);
  * for reference, in the same run, the call that walks the same table without the join: gys_actconn_list_dev over all rows (every row
    written, and the count alone).

Every figure: warm calls first, then --reps timed calls; device time between two events on the engine's stream and the call's wall time
(the call synchronised), median and min .. max.  Run from the repository root on a machine with an MI355X:
    python tools/svcdeps_timing.py [--hosts N] [--svcs N] [--rows N] [--bound F] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=1000)
    ap.add_argument("--svcs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--bound", type=float, default=0.1)
    ap.add_argument("--roots", type=int, default=16)
    ap.add_argument("--max-levels", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
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
    eng = SketchEngine(max_hosts=a.hosts, max_services=a.hosts * a.svcs, enable_tdigest=False, actconn_pair_cap=cap)
    s = np.arange(a.svcs)
    gids = []
    t0 = time.perf_counter()
    for h in range(a.hosts):
        mid = wire.machine_id(h)
        eng.register_host(mid, "c%d" % (h % 4))
        g = wire.glob_id(np.full(a.svcs, h), s)
        eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
        gids.append(g)
    gids = np.concatenate(gids)
    nsvc = len(gids)
    tasks = wire.splitmix64(np.arange(nsvc, dtype=np.uint64) + np.uint64(0x7A5C0000)) | np.uint64(1)
    t1 = time.perf_counter()
    assert eng.set_listener_tasks(gids, tasks) == capi.OK
    lines = ["services %d, rows %d, bound clients %.2f, actconn_pair_cap %d" % (nsvc, a.rows, a.bound, cap),
             "registration %.1f s, gys_set_listener_tasks (host) %.1f ms" % (t1 - t0, (time.perf_counter() - t1) * 1e3)]
    rng = np.random.default_rng(1)
    chunk = 1 << 20
    for first in range(0, a.rows, chunk):  # row j: listener j % nsvc, client: a bound task group or splitmix(j) (distinct keys)
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
    lines.append("table: %s" % eng.actconn_table_stats())

    def timed(what, fn, warm=2):
        for _ in range(warm):
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
        lines.append("%-52s device ms median %.3f (min %.3f max %.3f)   wall ms median %.3f (min %.3f max %.3f)   n=%d" % (
            what, np.median(dev), min(dev), max(dev), np.median(wall), min(wall), max(wall), a.reps))
        return float(np.median(wall))

    nm = C.c_uint32()
    st = eng.svcgraph_stats()
    lines.append("graph: %s" % st)
    ne = int(st["edges"])
    timed("gys_svcgraph_stats (one walk, counters)", eng.svcgraph_stats)
    out = torch.empty((max(ne, 1), 64), dtype=torch.uint8, device=eng.device)
    eng.order()
    timed("gys_svc_edges_dev, all edges written", lambda: capi.check(eng.L.gys_svc_edges_dev(eng.h, None, C.c_void_p(out.data_ptr()), ne, C.byref(nm))))
    timed("gys_svc_edges_dev, count only", lambda: capi.check(eng.L.gys_svc_edges_dev(eng.h, None, None, 0, C.byref(nm))))
    rows = torch.empty((a.rows, 128), dtype=torch.uint8, device=eng.device)
    eng.order()
    timed("gys_actconn_list_dev, all rows written (reference)", lambda: capi.check(eng.L.gys_actconn_list_dev(eng.h, None, C.c_void_p(rows.data_ptr()), a.rows, C.byref(nm))))
    timed("gys_actconn_list_dev, count only (reference)", lambda: capi.check(eng.L.gys_actconn_list_dev(eng.h, None, None, 0, C.byref(nm))))
    del rows
    roots = np.ascontiguousarray(gids[rng.integers(0, nsvc, a.roots)], dtype=np.uint64)
    hops = torch.empty(nsvc, dtype=torch.int32, device=eng.device)
    eng.order()

    def deps(max_hops, direction=capi.DEP_CALLEES):
        capi.check(eng.L.gys_svc_deps_dev(eng.h, roots.ctypes.data_as(capi.u64p), len(roots), direction, max_hops, C.c_void_p(hops.data_ptr()), C.byref(nm)))
        return nm.value

    timed("gys_svc_deps_dev, callees, 3 hops", lambda: deps(3))
    lines.append("  reached %d" % deps(3))
    timed("gys_svc_deps_dev, callees, no limit", lambda: deps(0))
    lines.append("  reached %d" % deps(0))
    timed("gys_svc_deps_dev, both ways, no limit", lambda: deps(0, capi.DEP_BOTH))
    full = deps(0, capi.DEP_BOTH)
    lines.append("  reached %d" % full)
    prev_ms, prev_n = None, len(set(int(x) for x in roots))
    for h in range(1, a.max_levels + 1):
        ms = timed("gys_svc_deps_dev, both ways, max_hops %d" % h, lambda: deps(h, capi.DEP_BOTH), warm=1)
        n = deps(h, capi.DEP_BOTH)
        lines.append("  reached %d (+%d)%s" % (n, n - prev_n, "" if prev_ms is None else "   level %d costs %.3f ms wall over max_hops %d" % (h, ms - prev_ms, h - 1)))
        prev_ms, prev_n = ms, n
        if n == full:
            break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    eng.close()


if __name__ == "__main__":
    main()
