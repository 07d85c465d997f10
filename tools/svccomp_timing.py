"""Timing of the service components ("Service components" in include/gysketch.h) on one GPU, beside the level-synchronous search over
the same graph in the same run:

  * graph 1, the one of tools/svcdeps_timing.py: --hosts x --svcs services (default 1000 x 1000 = 10^6), every one bound to a task group of
    its own; --rows (default 4 * 10^6) live rows with distinct (listener, client) keys, --bound (default 0.1) of them naming a bound
    task group (4 * 10^5 edges); gys_svc_deps_dev(GYS_DEP_BOTH, 0) from --roots (default 16) roots beside it;
  * graph 2: ONE PATH of --path (default 10^5) services in shuffled slot order, a row per hop; gys_svc_deps_dev(GYS_DEP_BOTH, 0) from one
    end of the path beside it (a level per hop);
  * on both: gys_svc_components_dev without and with the counts, gys_svc_components(min_services = 2) and gys_label_service_components(2);
    then the profile scopes of one gys_svc_components call -- dep_edges (the two walks that build the pair array), cc_hook (init + hook),
    cc_flatten, cc_figures (sizes + roots), cc_rows (the third walk) -- with their launch counts: the same on both graphs.

Every figure: warm calls first, then --reps timed calls; device time between two events on the engine's stream and the call's wall time
(the call synchronised), median and min .. max.  Run from the repository root on a machine with an MI355X:
    python tools/svccomp_timing.py [--hosts N] [--svcs N] [--rows N] [--bound F] [--path N] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_engine(nhosts, svcs, cap):
    from gyeeta_amd import capi, wire
    from gyeeta_amd.engine import SketchEngine
    eng = SketchEngine(max_hosts=nhosts, max_services=nhosts * svcs, enable_tdigest=False, actconn_pair_cap=cap)
    s = np.arange(svcs)
    gids = []
    for h in range(nhosts):
        mid = wire.machine_id(h)
        eng.register_host(mid, "c%d" % (h % 4))
        g = wire.glob_id(np.full(svcs, h), s)
        eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
        gids.append(g)
    gids = np.concatenate(gids)
    tasks = wire.splitmix64(np.arange(len(gids), dtype=np.uint64) + np.uint64(0x7A5C0000)) | np.uint64(1)
    assert eng.set_listener_tasks(gids, tasks) == capi.OK
    return eng, gids, tasks


def ingest(eng, torch, lids, cids):
    from gyeeta_amd import capi, wire
    chunk = 1 << 20
    for first in range(0, len(lids), chunk):
        n = min(chunk, len(lids) - first)
        rec = np.zeros(n, dtype=wire.ACTIVE_CONN_STATS)
        rec["listener_glob_id"] = lids[first:first + n]
        rec["cli_aggr_task_id"] = cids[first:first + n]
        rec["bytes_sent"], rec["active_conns"] = 1000, 1
        batch = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(eng.device)
        eng.order()
        capi.check(eng.L.gys_ingest_active_conns_dev(eng.h, C.c_void_p(batch.data_ptr()), n))
        eng.sync()


def measure(eng, torch, lines, roots, reps, bfs_reps):
    from gyeeta_amd import capi
    nsvc = eng.num_services()

    def timed(what, fn, warm=2, n=reps):
        for _ in range(warm):
            fn()
        eng.sync()
        dev, wall = [], []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(eng.stream)
            fn()
            e1.record(eng.stream)
            eng.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        lines.append("%-52s device ms median %.3f (min %.3f max %.3f)   wall ms median %.3f (min %.3f max %.3f)   n=%d" % (
            what, np.median(dev), min(dev), max(dev), np.median(wall), min(wall), max(wall), n))
        return float(np.median(wall))

    lines.append("table: %s" % eng.actconn_table_stats())
    lines.append("graph: %s" % eng.svcgraph_stats())
    comp = torch.empty(nsvc, dtype=torch.int32, device=eng.device)
    nc, nl, nm, nout = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    eng.order()
    cp = C.c_void_p(comp.data_ptr())
    t_plain = timed("gys_svc_components_dev, no counts", lambda: capi.check(eng.L.gys_svc_components_dev(eng.h, cp, None, None)))
    timed("gys_svc_components_dev, with counts", lambda: capi.check(eng.L.gys_svc_components_dev(eng.h, cp, C.byref(nc), C.byref(nl))))
    lines.append("  components %d, with two members or more %d" % (nc.value, nl.value))
    out = (capi.SvcComponent * max(nl.value, 1))()
    timed("gys_svc_components(min_services = 2)", lambda: capi.check(eng.L.gys_svc_components(eng.h, 2, out, nl.value, C.byref(nout), C.byref(nm), C.byref(nc))))
    lines.append("  listed %d, the largest: %d services, %d edges, %d rows" % (nout.value, out[0].nservices, out[0].nedges, out[0].nrows))
    timed("gys_label_service_components(2)", lambda: capi.check(eng.L.gys_label_service_components(eng.h, 2, C.byref(nm))))
    lines.append("  labels in use %d" % nm.value)
    hops = torch.empty(nsvc, dtype=torch.int32, device=eng.device)
    eng.order()
    r = np.ascontiguousarray(roots, dtype=np.uint64)
    t_bfs = timed("gys_svc_deps_dev, both ways, no limit, %d root(s)" % len(r),
                  lambda: capi.check(eng.L.gys_svc_deps_dev(eng.h, r.ctypes.data_as(capi.u64p), len(r), capi.DEP_BOTH, 0, C.c_void_p(hops.data_ptr()), C.byref(nm))),
                  warm=1, n=bfs_reps)
    lines.append("  reached %d, deepest %d hops" % (nm.value, int(hops[hops >= 0].max().item())))
    lines.append("  the search / gys_svc_components_dev (no counts), wall: %.2f" % (t_bfs / t_plain))
    # the scopes of ONE gys_svc_components call
    eng.profile(True)
    eng.profile_reset()
    capi.check(eng.L.gys_svc_components(eng.h, 2, out, nl.value, C.byref(nout), C.byref(nm), C.byref(nc)))
    eng.sync()
    pr = eng.profile_get()
    eng.profile(False)
    lines.append("  one gys_svc_components call: " + ", ".join("%s %.3f ms (%d)" % (k, pr[k][0], pr[k][1]) for k in ("dep_edges", "cc_hook", "cc_flatten", "cc_figures", "cc_rows") if k in pr))
    part, build = sum(pr[k][0] for k in ("cc_hook", "cc_flatten") if k in pr), pr.get("dep_edges", (0.0, 0))[0]
    lines.append("  partition (init, hook, flatten) %.3f ms, pair-array build (two walks) %.3f ms: ratio %.2f" % (part, build, part / build if build else 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=1000)
    ap.add_argument("--svcs", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--bound", type=float, default=0.1)
    ap.add_argument("--roots", type=int, default=16)
    ap.add_argument("--path", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from gyeeta_amd import wire
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing measured")
    lines = []
    # ---- graph 1: the graph of tools/svcdeps_timing.py
    cap = 1
    while cap < a.rows:
        cap *= 2
    eng, gids, tasks = make_engine(a.hosts, a.svcs, cap)
    nsvc = len(gids)
    lines.append("GRAPH 1: services %d, rows %d, bound clients %.2f, actconn_pair_cap %d" % (nsvc, a.rows, a.bound, cap))
    rng = np.random.default_rng(1)
    j = np.arange(a.rows, dtype=np.uint64)  # row j: listener j % nsvc, client: a bound task group or splitmix(j) (distinct keys)
    caller = ((j // np.uint64(nsvc)) * np.uint64(7919) + j * np.uint64(31) + np.uint64(1)) % np.uint64(nsvc)
    cids = np.where(rng.random(a.rows) < a.bound, tasks[caller.astype(np.int64)], wire.splitmix64(j + np.uint64(0x51ED)) & ~np.uint64(1))
    ingest(eng, torch, gids[(j % np.uint64(nsvc)).astype(np.int64)], cids)
    measure(eng, torch, lines, gids[rng.integers(0, nsvc, a.roots)], a.reps, a.reps)
    eng.close()
    del eng
    # ---- graph 2: one path
    svcs = 1000
    nh = max(1, (a.path + svcs - 1) // svcs)
    cap = 1
    while cap < a.path:
        cap *= 2
    eng, gids, tasks = make_engine(nh, svcs, cap)
    order = np.random.default_rng(2).permutation(len(gids))[:a.path]
    lines.append("")
    lines.append("GRAPH 2: one path of %d services in shuffled slot order (%d registered), a row per hop, actconn_pair_cap %d" % (len(order), len(gids), cap))
    ingest(eng, torch, gids[order[1:]], tasks[order[:-1]])
    measure(eng, torch, lines, gids[order[:1]], a.reps, 3)
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
