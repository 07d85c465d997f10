"""Timing of the live active-connection row table (gys_config.actconn_pair_cap) on one GPU:

  * gys_ingest_active_conns_dev on --rows (default 2^20) device-resident rows that name --keys (default 10^6) distinct (listener, client)
    pairs: the same batch with the table off (--cap 0: the Count-Min roll-up and the per-listener sums alone -- what the call launched before
    the table existed; this mode also runs on a tree that does not know the field) and with the table on;
  * with the table on and all keys live: gys_actconn_list_dev (every row written, and the count alone) and gys_actconn_svc_stats_dev.

Every figure: warm calls first, then --reps timed calls; device time between two events on the engine's stream and the call's wall time
(the call synchronised), median and min .. max.  Run from the repository root on a machine with an MI355X:
    python tools/actconn_pairs_timing.py [--cap N] [--rows N] [--keys N] [--out FILE]
GYS_TREE=<another checkout, built> measures that checkout's package and library with this script (the parent commit: --cap 0)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GYS_TREE", ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=1 << 21)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=100)
    ap.add_argument("--svcs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from gyeeta_amd import capi, wire
    from gyeeta_amd.engine import SketchEngine
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing measured")
    kw = dict(actconn_pair_cap=a.cap) if a.cap else {}
    eng = SketchEngine(max_hosts=a.hosts, max_services=a.hosts * a.svcs, enable_tdigest=False, **kw)
    s = np.arange(a.svcs)
    gids = []
    for h in range(a.hosts):
        mid = wire.machine_id(h)
        eng.register_host(mid, "c%d" % (h % 4))
        g = wire.glob_id(np.full(a.svcs, h), s)
        eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
        gids.append(g)
    gids = np.concatenate(gids)
    rng = np.random.default_rng(1)
    rec = wire.synth_active_conns(rng, a.rows, 0, a.svcs, remote_listen_frac=0.0, unknown_frac=0.0)
    key = np.arange(a.rows, dtype=np.uint64) % np.uint64(a.keys)  # key j: listener j % nsvc, client task group splitmix(j)
    rec["listener_glob_id"] = gids[(key % np.uint64(len(gids))).astype(np.int64)]
    rec["cli_aggr_task_id"] = wire.splitmix64(key + np.uint64(0x51ED))
    batch = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(eng.device)
    torch.cuda.synchronize()
    lines = ["rows %d, distinct keys %d, services %d, actconn_pair_cap %d" % (a.rows, a.keys, len(gids), a.cap)]

    def timed(what, fn, warm=3):
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
        lines.append("%-44s device ms median %.3f (min %.3f max %.3f)   wall ms median %.3f (min %.3f max %.3f)   n=%d" % (
            what, np.median(dev), min(dev), max(dev), np.median(wall), min(wall), max(wall), a.reps))

    eng.order()
    timed("gys_ingest_active_conns_dev, table %s" % ("on" if a.cap else "off"),
          lambda: capi.check(eng.L.gys_ingest_active_conns_dev(eng.h, C.c_void_p(batch.data_ptr()), a.rows)))
    if a.cap:
        st = eng.actconn_table_stats()
        lines.append("table: %s" % st)
        out = torch.empty((a.keys, 128), dtype=torch.uint8, device=eng.device)
        nm = C.c_uint32()
        eng.order()
        timed("gys_actconn_list_dev, all rows written", lambda: capi.check(eng.L.gys_actconn_list_dev(eng.h, None, C.c_void_p(out.data_ptr()), a.keys, C.byref(nm))))
        lines.append("  matches %d" % nm.value)
        sel = eng.actconn_sel(listener=int(gids[7]))
        timed("gys_actconn_list_dev, one listener", lambda: capi.check(eng.L.gys_actconn_list_dev(eng.h, C.byref(sel), C.c_void_p(out.data_ptr()), a.keys, C.byref(nm))))
        lines.append("  matches %d" % nm.value)
        timed("gys_actconn_list_dev, count only", lambda: capi.check(eng.L.gys_actconn_list_dev(eng.h, None, None, 0, C.byref(nm))))
        col = torch.empty((len(gids), 4), dtype=torch.float64, device=eng.device)
        eng.order()
        timed("gys_actconn_svc_stats_dev", lambda: capi.check(eng.L.gys_actconn_svc_stats_dev(eng.h, C.c_void_p(col.data_ptr()))))
        lines.append("  live client groups over all services %d" % int(col[:, 0].sum().item()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    eng.close()


if __name__ == "__main__":
    main()
