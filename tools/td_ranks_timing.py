"""Timing of gys_scan_ranks_dev at 10^7 services (10 000 hosts x 1 000) at the benchmark's gys_config (td_pend_cap 1 920, 2^29 events per
window, no levels) on one MI355X, after the benchmark's own set-up: the de-phase pass that spreads the buffers' fill levels, then one buffer
cycle of ordinary windows -- every service has re-clustered and holds about half a buffer.  Device events on the engine's stream around
the C call, 3 warm-up calls, 20 repeats, for 1, 3 and 16 thresholds; beside each the bytes the pass moves and, in the same run, a device
copy that moves the same number of bytes (a copy of B / 2 bytes reads B / 2 and writes B / 2); and, in the same process for comparison,
gys_scan_quantiles_dev for three quantiles (the pass that re-clusters every service: what a bisection for "how many within x ms" would
cost per step) and gys_tdigest_rollup_dev(HOST) with its profile scope (k_rollup_accum and the kernels around it read the same state).
Bytes per service: 200 x (8 + 4) of clusters + 16 (TdMeta) + 8 (td_minmax) + 4 per buffered value + 8 per threshold + 8 (total) written;
the buffered values per service are the mean of a sample of 20 hosts' services (gys_export_tdigest_pending).
Usage: python tools/td_ranks_timing.py [output file [hosts services-per-host]]   (profiles/td_ranks_timing.txt keeps a run)."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gyeeta_amd import build, capi, wire
from gyeeta_amd.engine import SketchEngine

NH, SP, NEV, REPS, CAP = 10000, 1000, 1 << 29, 20, 1920
if len(sys.argv) > 2:  # a rehearsal size: hosts, services per host
    NH, SP = int(sys.argv[2]), int(sys.argv[3])
    NEV = max(1 << 16, NH * SP * 54)
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def P(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True); out.write(s + "\n"); out.flush()

NSVC = NH * SP
P("device code", build.device_code_sha(), "| one MI355X |", NH, "hosts x", SP, "services, td_pend_cap", CAP, "enable_levels 0,", NEV, "events per window")
t0 = time.perf_counter()
eng = SketchEngine(max_hosts=NH, max_services=NSVC, max_clusters=16, enable_tdigest=True, max_batch_events=NEV, td_pend_cap=CAP)
s_ = np.arange(SP)
mids = [wire.machine_id(h) for h in range(NH)]
for h in range(NH):
    eng.register_host(mids[h], "cluster%d" % (h % 8))
    eng.register_listeners_np(mids[h], wire.glob_id(np.full(SP, h), s_), wire.listener_netns(h, s_), wire.listener_port(s_))
bufs = [torch.empty(NEV * 24, dtype=torch.uint8, device="cuda") for _ in range(2)]
# the benchmark's de-phase pass (CAP / 2 events per service on average, per-service weights spread over 0 .. 255 / 256), then a buffer cycle
total = NSVC * (CAP // 2 - 1)
nb = max(1, -(-total // NEV))
per = min(NEV, total // nb)
for b in range(nb):
    sg = eng.gen_resp_events(bufs[0].data_ptr(), per, 0xdef0 + 77 * b, 0, NH, SP, 0xFFFFFFFF)
    eng.handle_resp_events_dev(sg, bufs[0].data_ptr(), per)
eng.window_close(0)
segs = [eng.gen_resp_events(bufs[b].data_ptr(), NEV, 0x67796565746121 + b, 0, NH, SP) for b in range(2)]
nwin = min(100, int(CAP * NSVC / NEV) + 2)
for i in range(nwin):
    eng.handle_resp_events_dev(segs[i % 2], bufs[i % 2].data_ptr(), NEV)
    eng.window_close(0)
eng.sync()
P("setup %.1f s: de-phase pass of %d batches, then %d windows" % (time.perf_counter() - t0, nb, nwin))
L, h = eng.L, eng.h
sample = np.concatenate([eng.export_tdigest_pending(first=hh * SP, n=SP)[0] for hh in range(0, NH, max(1, NH // 20))])
npend_mean = float(sample.mean())
P("buffered values per service (sample of %d services): mean %.1f, min %d, max %d" % (len(sample), npend_mean, sample.min(), sample.max()))
torch.cuda.synchronize()

def timed(name, fn, reps=REPS, warm=3):
    """device events on the engine's stream around the call"""
    for _ in range(warm):
        fn(); eng.sync()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(eng.stream); fn(); e1.record(eng.stream); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    P("%-58s min %8.3f ms  median %8.3f ms  max %8.3f ms  (%d repeats)" % (name, min(ts), statistics.median(ts), max(ts), reps))
    return min(ts), statistics.median(ts)

def scopes(fn, reps=REPS):
    eng.profile(True); eng.profile_reset()
    for _ in range(reps):
        fn()
    eng.sync()
    pf = eng.profile_get()
    eng.profile(False)
    return {k: v[0] / reps for k, v in pf.items()}

def copy_rate(nbytes):
    """a device copy that moves nbytes in all (reads half, writes half), on the engine's stream"""
    a = torch.empty(int(nbytes) // 2, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
    a.fill_(1); torch.cuda.synchronize()
    def cp():
        with torch.cuda.stream(eng.stream):
            b.copy_(a)
    mn, med = timed("  device copy moving %.2f GB (reads + writes)" % (nbytes / 1e9), cp)
    del a, b
    return nbytes / (med * 1e-3)

below = torch.empty((NSVC, 16), dtype=torch.float64, device="cuda")
tot = torch.empty(NSVC, dtype=torch.int64, device="cuda")
pb, pt = C.c_void_p(below.data_ptr()), C.c_void_p(tot.data_ptr())
THR = {1: [100], 3: [50, 100, 250], 16: [1, 2, 3, 5, 8, 12, 20, 30, 50, 80, 120, 200, 300, 500, 1000, 5000]}
rank_ms = {}
for nt in (1, 3, 16):
    ta = (C.c_int64 * nt)(*THR[nt])
    call = lambda: capi.check(L.gys_scan_ranks_dev(h, ta, nt, pb, pt))
    mn, med = timed("gys_scan_ranks_dev(%d threshold%s)" % (nt, "" if nt == 1 else "s"), call)
    rank_ms[nt] = med
    nbytes = NSVC * (200 * 12 + 16 + 8 + 4 * npend_mean + 8 * nt + 8)
    sc = scopes(call).get("scan_ranks", 0.0)
    cr = copy_rate(nbytes)
    kr = nbytes / (sc * 1e-3) if sc else 0.0
    eng.sync()
    row = below.view(-1)[:nt].cpu().numpy()
    P("  k_td_ranks (profile scope) %.3f ms per call: %.2f GB -> %.1f GB/s = %.0f %% of the copy's %.1f GB/s | slot 0: below %s of %d" %
      (sc, nbytes / 1e9, kr / 1e9, 100.0 * kr / cr, cr / 1e9, np.array2string(row, precision=1), int(tot[0])))
qa = (C.c_double * 3)(0.25, 0.95, 0.99)
qout = torch.empty((NSVC, 3), dtype=torch.float64, device="cuda")
mn, qmed = timed("gys_scan_quantiles_dev(3 quantiles)", lambda: capi.check(L.gys_scan_quantiles_dev(h, qa, 3, C.c_void_p(qout.data_ptr()))))
slabs = torch.zeros(NH * C.sizeof(capi.TDigestSlab), dtype=torch.uint8, device="cuda")
roll = lambda: capi.check(L.gys_tdigest_rollup_dev(h, capi.ROLLUP_HOST, C.c_void_p(slabs.data_ptr())))
mn, rmed = timed("gys_tdigest_rollup_dev(HOST)", roll)
P("  its profile scope (k_rollup_init, _accum, _mark, _refine, _cluster) %.3f ms per call" % scopes(roll).get("rollup_services", 0.0))
P("rank pass / quantile pass: %s" % ", ".join("%d thresholds %.2f" % (nt, rank_ms[nt] / qmed) for nt in (1, 3, 16)))
# the host slabs through the same kernel
ta = (C.c_int64 * 3)(*THR[3])
timed("gys_tdigest_slab_ranks_dev(%d host slabs, 3 thresholds)" % NH, lambda: capi.check(L.gys_tdigest_slab_ranks_dev(h, C.c_void_p(slabs.data_ptr()), NH, ta, 3, pb, pt)))
eng.close()
