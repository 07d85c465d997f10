"""Timing of gys_pack_services_dev / gys_unpack_services_dev on one GPU -> profiles/svcpack_timing.txt

--services (default 10^6) services at the benchmark's per-service configuration (t-digest on, td_pend_cap 1 920, no levels), their value
buffers filled to a spread of levels by generated response events.  Every service is packed into one device blob and unpacked into a
second context with the same registrations; the kernels' stream time is the library's own profile scopes (svc_pack / svc_unpack), and
a device-to-device copy of as many bytes as the blob's records runs beside them in the same run.  The three times and the two ratios are
written.

Run from the repository root on a machine with an MI355X:  python tools/svcpack_timing.py [--services N]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=1_000_000)
    ap.add_argument("--hosts", type=int, default=1000)
    ap.add_argument("--td-pend-cap", type=int, default=1920)
    ap.add_argument("--td-buf-values", type=int, default=2304, help="buffer words per service (what the library picks at the benchmark's 10^7 services)")
    ap.add_argument("--events", type=int, default=1 << 26)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svcpack_timing.txt"))
    a = ap.parse_args()
    import torch
    from gyeeta_amd import capi, wire
    from gyeeta_amd.engine import SketchEngine
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing measured, nothing written")
    per = a.services // a.hosts
    nsvc = per * a.hosts
    engs = [SketchEngine(max_hosts=a.hosts, max_services=nsvc, max_batch_events=a.events, td_pend_cap=a.td_pend_cap, td_buf_values=a.td_buf_values) for _ in range(2)]
    s = np.arange(per)
    for h in range(a.hosts):
        mid = wire.machine_id(h)
        g, ns, pt = wire.glob_id(np.full(per, h), s), wire.listener_netns(h, s), wire.listener_port(s)
        for eng in engs:
            eng.register_host(mid, "c%d" % (h % 8))
            eng.register_listeners_np(mid, g, ns, pt)
    src, dst = engs
    d_ev = torch.empty(a.events * 24, dtype=torch.uint8, device="cuda")
    for k in range(a.batches):
        segs = src.gen_resp_events(d_ev.data_ptr(), a.events, 1 + k, 0, a.hosts, per, 0xFFFFFFFF)  # GYS_GEN_SPREAD: evenly spread fill levels
        src.handle_resp_events_dev(segs, d_ev.data_ptr(), a.events)
        if k == 0:
            src.window_close(1_700_000_000_000_000)
    src.sync()
    del d_ev
    npend = src.export_tdigest_pending(0, min(nsvc, 4096))[0]
    ids = src.list_service_ids()
    nbytes = src.service_blob_bytes(len(ids))
    stride = src.service_blob_bytes(1) - 80
    rec_bytes = len(ids) * stride
    lines = ["services %d (hosts %d), td_pend_cap %d, %d batches of %d events: record stride %d B, blob %d B; buffered values of the first %d services: mean %.0f"
             % (len(ids), a.hosts, a.td_pend_cap, a.batches, a.events, stride, nbytes, len(npend), float(npend.mean()))]
    for eng in engs:
        eng.profile(True)

    def scope_ms(eng, fn, scope):
        fn()
        best = 1e9
        for _ in range(a.reps):
            eng.profile_reset()
            fn()
            eng.sync()
            best = min(best, eng.profile_get()[scope][0])
        return best

    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idp = ids.ctypes.data_as(src.L.gys_pack_services_dev.argtypes[1])

    def pack():
        capi.check(src.L.gys_pack_services_dev(src.h, idp, len(ids), C.c_void_p(blob.data_ptr()), nbytes))

    t_pack = scope_ms(src, pack, "svc_pack")
    t_unpack = scope_ms(dst, lambda: dst.unpack_services(blob), "svc_unpack")
    a_, b_ = torch.empty(rec_bytes, dtype=torch.uint8, device="cuda"), torch.empty(rec_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_copy = 1e9
    for _ in range(a.reps + 1):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        b_.copy_(a_)
        ev1.record()
        torch.cuda.synchronize()
        t_copy = min(t_copy, ev0.elapsed_time(ev1))
    gbs = lambda ms: rec_bytes / ms / 1e6
    lines.append("k_svc_pack   %.3f ms (%.0f GB/s of record bytes)" % (t_pack, gbs(t_pack)))
    lines.append("k_svc_unpack %.3f ms (%.0f GB/s of record bytes)" % (t_unpack, gbs(t_unpack)))
    lines.append("device-to-device copy of %d bytes: %.3f ms (%.0f GB/s)" % (rec_bytes, t_copy, gbs(t_copy)))
    lines.append("ratios to the copy: pack %.2f, unpack %.2f (best of %d each; the pack writes the whole record and reads only the live part of the buffers, "
                 "the unpack reads and writes only the live part)" % (t_pack / t_copy, t_unpack / t_copy, a.reps))
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    for eng in engs:
        eng.close()


if __name__ == "__main__":
    main()
