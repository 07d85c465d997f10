"""Timing of the listener-deletion calls on one GPU -> profiles/listener_delete_timing.txt

  * at --services (default 10^7) services that all hold a kept state record: gys_list_stale_listeners beside the filter pass of
    gys_query_svcstate_scan in the same run (both read the 96-byte kept records; the ratio is stated);
  * a --batch (default 512) id gys_delete_listeners split into host rebuild, table erase and k_svc_clear (the library's own profile scopes),
    the clear as bytes / time beside a device-to-device copy of the same number of bytes.

Run from the repository root on a machine with an MI355X:  python tools/listener_delete_timing.py [--services N] [--batch N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=10_000_000)
    ap.add_argument("--hosts", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "listener_delete_timing.txt"))
    a = ap.parse_args()
    import torch
    from gyeeta_amd import wire
    from gyeeta_amd.engine import SketchEngine
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing measured, nothing written")
    per = a.services // a.hosts
    eng = SketchEngine(max_hosts=a.hosts, max_services=a.hosts * per, max_batch_events=1 << 20, enable_levels=True, svc_hll_p=6, svc_hll_levels=1)
    rng = np.random.default_rng(1)
    mids = [wire.machine_id(h) for h in range(a.hosts)]
    s = np.arange(per)
    for h in range(a.hosts):
        eng.register_host(mids[h], "c%d" % (h % 8))
        eng.register_listeners_np(mids[h], wire.glob_id(np.full(per, h), s), wire.listener_netns(h, s), wire.listener_port(s))
    for h in range(a.hosts):  # a kept record per service
        rec = wire.synth_listener_states(rng, h, s)
        for i in range(0, per, 512):
            eng.partha_listener_state(mids[h], rec[i:i + 512].tobytes(), len(rec[i:i + 512]))
    eng.window_close(1_700_000_000_000_000)
    eng.sync()
    lines = ["services %d, hosts %d, batch %d" % (a.hosts * per, a.hosts, a.batch)]
    eng.profile(True)

    def scope_ms(fn, scope, reps=5):
        """device time of the library's profile scope `scope` (events on the stream), per call, and the call's wall time: best of reps"""
        fn()
        eng.sync()
        dev = wall = 1e9
        for _ in range(reps):
            eng.profile_reset()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            wall = min(wall, (time.perf_counter() - t0) * 1e3)
            dev = min(dev, eng.profile_get()[scope][0])
        return dev, wall

    # nobody is stale (the worst case of the pass is the same read: two words of every record)
    d_stale, w_stale = scope_ms(lambda: eng.list_stale_listeners(3, 360, cap=65536), "svc_stale")
    d_filt, w_scan = scope_ms(lambda: eng.svcstate_scan(maxrecs=1000), "svc_filter")
    lines.append("gys_list_stale_listeners: device pass %.3f ms (call %.3f ms); filter pass of gys_query_svcstate_scan: %.3f ms (call with top 1000: %.3f ms); "
                 "ratio stale / filter pass %.2f" % (d_stale, w_stale, d_filt, w_scan, d_stale / d_filt))
    ids = wire.glob_id(np.full(a.batch, 1), np.arange(a.batch) % per)
    eng.profile_reset()
    t0 = time.perf_counter()
    nd = eng.delete_listeners(ids)
    eng.sync()
    t_del = (time.perf_counter() - t0) * 1e3
    prof = eng.profile_get()
    lines.append("gys_delete_listeners of %d ids: %.3f ms wall; stream time of the scopes (ms): %s"
                 % (nd, t_del, ", ".join("%s %.4f" % (k, prof[k][0]) for k in ("host_rebuild", "table_erase", "svc_clear"))))
    per_svc = eng.svc_state_bytes()  # what k_svc_clear writes per slot, summed by the library over its own segment list
    nbytes = nd * per_svc
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst.copy_(src)
    ev0.record()
    dst.copy_(src)
    ev1.record()
    torch.cuda.synchronize()
    t_clear, t_copy = prof["svc_clear"][0], ev0.elapsed_time(ev1)
    lines.append("k_svc_clear: %d bytes (%d per slot) in %.4f ms = %.1f GB/s; a device copy of as many bytes: %.4f ms = %.1f GB/s"
                 % (nbytes, per_svc, t_clear, nbytes / t_clear / 1e6, t_copy, nbytes / t_copy / 1e6))
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
