"""Timing of gys_hist_rollup_period_dev at 10^7 services (10 000 hosts x 1 000, enable_levels = 1, lazily folded records) on one MI355X, with
device events on the engine's stream: the whole call for HOST scope, its fold pass and its union launches (the engine's profile scopes "fold"
and "hist_rollup_union": k_hist_period_union, members -> chunks, then the plain k_hist_level_union, chunks -> hosts), and in the same run a
device copy that moves the same number of bytes (a copy of B / 2 bytes reads B / 2 and writes B / 2).  Three periods, asked right after a close
(no service's open window is folded: no window record is read):
  * a level-1 period over the whole 300-s ring, every ring bucket whole: 10 boundary snapshots + the cumulative record per member;
  * the same ring with the first and the last bucket partly covered (two scales that truncate): the same bytes;
  * the since-start level: the cumulative record and first_sec.
Bytes per member, from the formula in gys_histroll.hpp: 4 (member index) + 16 (TdMeta) + 256 x (boundary snapshots + cumulative), + 8
(first_sec) for the since-start level; + 256 per chunk written.
Usage: python tools/hist_period_rollup_timing.py [output file]   (profiles/hist_period_rollup_timing.txt keeps a run)."""
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

NH, SP, NEV, REPS = 10000, 1000, 1 << 26, 20
if len(sys.argv) > 2:  # a rehearsal size: hosts, services per host
    NH, SP, NEV = int(sys.argv[2]), int(sys.argv[3]), 1 << 20
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def P(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True); out.write(s + "\n"); out.flush()

NSVC = NH * SP
P("device code", build.device_code_sha(), "| one MI355X |", NH, "hosts x", SP, "services, enable_levels 1, enable_tdigest 1,", NEV, "events per window")
t0 = time.perf_counter()
eng = SketchEngine(max_hosts=NH, max_services=NSVC, max_clusters=16, enable_tdigest=True, enable_levels=True, max_batch_events=NEV)
s_ = np.arange(SP)
mids = [wire.machine_id(h) for h in range(NH)]
for h in range(NH):
    eng.register_host(mids[h], "cluster%d" % (h % 8))
    eng.register_listeners_np(mids[h], wire.glob_id(np.full(SP, h), s_), wire.listener_netns(h, s_), wire.listener_port(s_))
ev = torch.empty(NEV * 24, dtype=torch.uint8, device="cuda")
T = 1_700_000_003
for k in range(12):  # closes 30 s apart: every bucket of the 300-s ring gets a snapshot and a window
    segs = eng.gen_resp_events(ev.data_ptr(), NEV, k + 1, 0, NH, SP)
    eng.handle_resp_events_dev(segs, ev.data_ptr(), NEV)
    T += 30
    eng.window_close(T * 1_000_000)
eng.sync()
P("setup %.1f s" % (time.perf_counter() - t0))
L, h = eng.L, eng.h
recs = torch.zeros((NH, 16, 2), dtype=torch.int64, device="cuda")
pr = C.c_void_p(recs.data_ptr())
lvu = C.c_int(-1)
nchunks = NH * ((SP + 1023) // 1024)
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
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
    a.fill_(1); torch.cuda.synchronize()
    def cp():
        with torch.cuda.stream(eng.stream):
            b.copy_(a)
    mn, med = timed("  device copy moving %.2f GB (reads + writes)" % (nbytes / 1e9), cp)
    return nbytes / (med * 1e-3)

tq, tus = T, T * 1_000_000
cur = tq - tq % 30  # start of the ring bucket that holds tq
# boundary snapshots a level-1 period over buckets [cur - 270, cur + 30) loads: the boundaries at or before the last close (the end is "now")
snaps = sum(1 for s in range(cur - 270, cur + 31, 30) if s <= tq)
cases = [("level 1, the whole ring, 10 whole buckets", cur - 270, tq, 1, 4 + 16 + 256 * (snaps + 1)),
         ("level 1, the whole ring, first and last bucket partly", cur - 270 + 7, tq - 2, 1, 4 + 16 + 256 * (snaps + 1)),
         ("since start", 0, tq + 5, 3, 4 + 16 + 256 + 8)]
for name, a, b, want_lv, per_member in cases:
    nbytes = NSVC * per_member + nchunks * 256
    call = lambda: capi.check(L.gys_hist_rollup_period_dev(h, capi.ROLLUP_HOST, a, b, tus, pr, C.byref(lvu)))
    mn, med = timed("gys_hist_rollup_period_dev(HOST, %s)" % name, call)
    assert lvu.value == want_lv, (name, lvu.value)
    sc = scopes(call)
    un = sc.get("hist_rollup_union", 0.0)
    P("  level used %d, %d B per member | scopes, ms per call: fold %.3f, union launches %.3f | total_count of host 0: %d" %
      (lvu.value, per_member, sc.get("fold", 0.0), un, int(recs[0, 15, 0])))
    cr = copy_rate(nbytes)
    kr = nbytes / (un * 1e-3) if un else 0.0
    P("  union kernel: %.2f GB -> %.1f GB/s = %.0f %% of the copy's %.1f GB/s" % (nbytes / 1e9, kr / 1e9, 100.0 * kr / cr, cr / 1e9))
eng.close()
