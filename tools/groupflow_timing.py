"""Timing of the group flow map ("Group flow map" in include/gysketch.h) on one GPU, on the graph of tools/svcdeps_timing.py:

  * --services (default 10^6) services, every one bound to a task group of its own; --rows (default 4 * 10^6) live rows with distinct
    (listener, client) keys, --bound (default 0.1) of them naming a bound task group as the client;
  * the same services and rows registered once under 2 hosts (every edge on <= 4 keys) and once under --many-hosts (default 10^4)
    hosts; in the second world also one label per service (every edge its own key);
  * gys_group_edges_dev with every row written, and the count alone;
  * in the same run what it replaces -- gys_svc_edges_dev with every edge written, the copy of the 64-byte rows to the host, and a numpy
    group-by of them (keys from the host's copy of the groups, np.unique, np.add.at over the five sums) -- and the floor: the bare count
    pass of k_dep_edges (gys_svc_edges_dev, count only), which walks the same table.

Every figure: 2 warm calls, then --reps (default 7) timed calls; device time between two events on the engine's stream and the call's
wall time (the call synchronised), median and min .. max.  Run from the repository root on a machine with an MI355X:
    python tools/groupflow_timing.py [--services N] [--rows N] [--bound F] [--many-hosts N] [--out FILE]"""
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
    ap.add_argument("--services", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--bound", type=float, default=0.1)
    ap.add_argument("--many-hosts", type=int, default=10_000)
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
    lines = []
    medians = {}

    def world(nhosts, with_labels):
        svcs = a.services // nhosts
        eng = SketchEngine(max_hosts=nhosts, max_services=nhosts * svcs, enable_tdigest=False, actconn_pair_cap=cap)
        s = np.arange(svcs)
        gids = []
        t0 = time.perf_counter()
        for h in range(nhosts):
            mid = wire.machine_id(h)
            eng.register_host(mid, "c%d" % (h % 4))
            g = wire.glob_id(np.full(svcs, h), s)
            eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
            gids.append(g)
        gids = np.concatenate(gids)
        nsvc = len(gids)
        tasks = wire.splitmix64(np.arange(nsvc, dtype=np.uint64) + np.uint64(0x7A5C0000)) | np.uint64(1)
        assert eng.set_listener_tasks(gids, tasks) == capi.OK
        lines.append("")
        lines.append("== %d hosts x %d services, rows %d, bound clients %.2f, actconn_pair_cap %d (registration %.1f s)" % (nhosts, svcs, a.rows, a.bound, cap, time.perf_counter() - t0))
        rng = np.random.default_rng(1)
        chunk = 1 << 20
        for first in range(0, a.rows, chunk):  # (the rows of tools/svcdeps_timing.py)
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
        st = eng.svcgraph_stats()
        lines.append("graph: %s" % st)
        ne = int(st["edges"])

        def timed(tag, what, fn, sync_inside=False):
            for _ in range(2):
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
            lines.append("%-66s device ms median %.3f (min %.3f max %.3f)   wall ms median %.3f (min %.3f max %.3f)   n=%d" % (
                what, np.median(dev), min(dev), max(dev), np.median(wall), min(wall), max(wall), a.reps))
            medians[tag] = (float(np.median(dev)), float(np.median(wall)))

        nm = C.c_uint32()
        fst = capi.GroupFlowStats()
        tag = "%d hosts" % nhosts
        timed(tag + " floor", "gys_svc_edges_dev, count only (the floor: k_dep_edges' count pass)", lambda: capi.check(eng.L.gys_svc_edges_dev(eng.h, None, None, 0, C.byref(nm))))
        # what the map replaces: every edge as a 64-byte row, to the host, grouped there
        out = torch.empty((max(ne, 1), 64), dtype=torch.uint8, device=eng.device)
        host_rows = torch.empty((max(ne, 1), 64), dtype=torch.uint8).pin_memory()
        slot_host = np.repeat(np.arange(nhosts, dtype=np.uint32), svcs)  # (the caller's own copy of slot -> host: slots are handed out in order)
        eng.order()

        def replaced(group_of_slot, ndomain):
            capi.check(eng.L.gys_svc_edges_dev(eng.h, None, C.c_void_p(out.data_ptr()), ne, C.byref(nm)))
            with torch.cuda.stream(eng.stream):
                host_rows.copy_(out, non_blocking=True)
            eng.sync()
            r = np.frombuffer(host_rows.numpy().tobytes(), dtype=eng.SVC_EDGE_DT)[:nm.value]
            key = group_of_slot[r["src_slot"]].astype(np.uint64) * np.uint64(ndomain) + group_of_slot[r["dst_slot"]].astype(np.uint64)
            uniq, inv = np.unique(key, return_inverse=True)
            sums = np.zeros((len(uniq), 5), dtype=np.uint64)
            np.add.at(sums[:, 0], inv, 1)
            np.add.at(sums[:, 1], inv, r["nrows"])
            np.add.at(sums[:, 2], inv, r["active_conns"])
            np.add.at(sums[:, 3], inv, r["bytes_sent"])
            np.add.at(sums[:, 4], inv, r["bytes_received"])
            return len(uniq)

        def group_edges(group_by, d_out, room):
            capi.check(eng.L.gys_group_edges_dev(eng.h, group_by, None, C.c_void_p(d_out.data_ptr()) if room else None, room, C.byref(nm), C.byref(fst)))
            return nm.value

        cases = [(tag + " HOST", capi.GROUP_HOST, slot_host, nhosts)]
        if with_labels:
            eng.set_service_groups(gids, np.arange(nsvc, dtype=np.uint32))
            cases.append((tag + " LABEL", capi.GROUP_LABEL, np.arange(nsvc, dtype=np.uint32), nsvc))
        for ctag, gb, gos, nd in cases:
            nge = group_edges(gb, None, 0)
            lines.append("%s: %d group edges; stats edges %d, no group %d, self %d" % (ctag, nge, fst.edges, fst.edges_no_group, fst.self_group_edges))
            d_rows = torch.empty((max(nge, 1), 64), dtype=torch.uint8, device=eng.device)
            eng.order()
            timed(ctag, "gys_group_edges_dev %s, all rows written" % ctag, lambda: group_edges(gb, d_rows, nge))
            timed(ctag + " count", "gys_group_edges_dev %s, count only" % ctag, lambda: group_edges(gb, None, 0))
            nu = replaced(gos, nd)
            lines.append("  (the host group-by finds %d group edges)" % nu)
            timed(ctag + " replaced", "gys_svc_edges_dev + copy to the host + numpy group-by, %s" % ctag, lambda: replaced(gos, nd))
        eng.close()

    world(2, False)
    world(a.many_hosts, True)
    lines.append("")
    many = "%d hosts" % a.many_hosts
    for ctag in ("2 hosts HOST", many + " HOST", many + " LABEL"):
        d, w = medians[ctag]
        floor = medians[ctag.rsplit(" ", 1)[0] + " floor"]
        rep = medians[ctag + " replaced"]
        lines.append("%-18s device %.3f ms = %.2f x the floor (%.3f ms);   wall %.3f ms, what it replaces %.3f ms: %.1f x" % (ctag, d, d / floor[0], floor[0], w, rep[1], rep[1] / w))
    lines.append("2 hosts / %s by HOST (device): %.2f" % (many, medians["2 hosts HOST"][0] / medians[many + " HOST"][0]))
    text = "\n".join(lines).lstrip("\n") + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
