"""Timing of gys_hist_rollup_level_dev / gys_hist_rollup_filtered_dev at 10^7 services (10 000 hosts x 1 000, enable_levels = 1, lazily folded
records) on one MI355X, with device events on the engine's stream: the whole call for HOST scope at levels 0, 1 and 3, its fold pass and its
union launches (the engine's profile scopes "fold" and "hist_rollup_union"), one filtered call grouped by host, and in the same run a device
copy that moves the same number of bytes (a copy of B / 2 bytes reads B / 2 and writes B / 2).  The bytes of a level are those the kernel asks
for (gys_histroll.hpp): 4 (member index) + per level 256 + 16 (level 3: cumulative record, TdMeta), 512 + 16 (level 1: + snapshot), 256 + 16 + 4
(level 0: last-window record, pair 15 of the cumulative record, tag), + 256 per chunk written.  Phase A is taken right after a close (no
service's open window is folded: no window record is read), phase B after an ingest into the open window and a fold (every touched service's
window record is read too, up to + 256 per member: the time is reported, the rate against the phase-A bytes is a lower bound).
Usage: python tools/hist_level_rollup_timing.py [output file]   (profiles/hist_level_rollup_timing.txt keeps a run)."""
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
def window(seed):
    segs = eng.gen_resp_events(ev.data_ptr(), NEV, seed, 0, NH, SP)
    eng.handle_resp_events_dev(segs, ev.data_ptr(), NEV)
for k in range(3):
    window(k + 1)
    T += 5
    eng.window_close(T * 1_000_000)
eng.sync()
P("setup %.1f s" % (time.perf_counter() - t0))
L, h = eng.L, eng.h
recs = torch.zeros((NH, 16, 2), dtype=torch.int64, device="cuda")
pr = C.c_void_p(recs.data_ptr())
rows = (capi.RollupRow * NH)()
n = C.c_uint32()
f0, k0 = eng._svc_filter(None)
nchunks = NH * ((SP + 1023) // 1024)
BYTES = {3: NSVC * (4 + 256 + 16) + nchunks * 256, 1: NSVC * (4 + 512 + 16) + nchunks * 256, 0: NSVC * (4 + 256 + 16 + 4) + nchunks * 256}
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

def phase(tag, tus):
    for lv in (3, 1, 0):
        call = lambda: capi.check(L.gys_hist_rollup_level_dev(h, capi.ROLLUP_HOST, lv, tus, pr))
        mn, med = timed("%s gys_hist_rollup_level_dev(HOST, level %d)" % (tag, lv), call)
        sc = scopes(call)
        un = sc.get("hist_rollup_union", 0.0)
        P("  scopes, ms per call: fold %.3f, union launches %.3f" % (sc.get("fold", 0.0), un))
        cr = copy_rate(BYTES[lv])
        kr = BYTES[lv] / (un * 1e-3) if un else 0.0
        P("  union kernel: %.2f GB -> %.1f GB/s = %.0f %% of the copy's %.1f GB/s" % (BYTES[lv] / 1e9, kr / 1e9, 100.0 * kr / cr, cr / 1e9))
    call = lambda: capi.check(L.gys_hist_rollup_filtered_dev(h, C.byref(f0), 1, capi.GROUP_HOST, 1, tus, rows, NH, C.byref(n), pr))
    timed("%s gys_hist_rollup_filtered_dev(no terms, HOST, ANY_STATE, level 1)" % tag, call)
    P("  rows", n.value, "| scopes, ms per call:", {k: round(v, 3) for k, v in scopes(call).items()})

phase("A (after a close)", T * 1_000_000)
window(9)
eng.sync()
phase("B (open window folded)", (T + 1) * 1_000_000)
eng.close()
