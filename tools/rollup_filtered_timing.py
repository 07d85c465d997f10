"""Timing of gys_rollup_filtered_dev at 10^7 services on one MI355X against the calls it stands for -- gys_tdigest_rollup_dev(HOST),
gys_hll_rollup_dev(HOST) and the filter pass of gys_query_svcstate_scan -- in one process on one engine state; also a filter that selects 1 % of
the services grouped by cluster, and a label grouping with 10^4 groups.  Usage: python tools/rollup_filtered_timing.py [output file]
(profiles/rollup_filtered_timing.txt keeps a run)."""
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

NH, SP, NEV, REPS = 10000, 1000, 1 << 28, 20
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def P(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True); out.write(s + "\n"); out.flush()

P("device code", build.device_code_sha(), "| one MI355X |", NH, "hosts x", SP, "services, svc_hll_p 4, td_pend_cap 1920,", NEV, "events x 2")
t0 = time.perf_counter()
eng = SketchEngine(max_hosts=NH, max_services=NH * SP, max_clusters=16, svc_hll_p=4, td_pend_cap=1920, max_batch_events=NEV)
s_ = np.arange(SP)
mids = [wire.machine_id(h) for h in range(NH)]
for h in range(NH):
    eng.register_host(mids[h], "cluster%d" % (h % 8))
    eng.register_listeners_np(mids[h], wire.glob_id(np.full(SP, h), s_), wire.listener_netns(h, s_), wire.listener_port(s_))
ev = torch.empty(NEV * 24, dtype=torch.uint8, device="cuda")
for seed in (1, 2):
    segs = eng.gen_resp_events(ev.data_ptr(), NEV, seed, 0, NH, SP)
    eng.handle_resp_events_dev(segs, ev.data_ptr(), NEV)
eng.sync()
del ev
P("setup %.1f s" % (time.perf_counter() - t0))
L, h = eng.L, eng.h
cap = NH
slabs = torch.zeros(cap * C.sizeof(capi.TDigestSlab), dtype=torch.uint8, device="cuda")
regs = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
est = torch.zeros(cap, dtype=torch.float64, device="cuda")
ps, pr, pe = C.c_void_p(slabs.data_ptr()), C.c_void_p(regs.data_ptr()), C.c_void_p(est.data_ptr())
rows = (capi.RollupRow * cap)()
n = C.c_uint32()
torch.cuda.synchronize()

def timed(name, fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn(); eng.sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); eng.sync(); ts.append((time.perf_counter() - t) * 1e3)
    P("%-46s min %8.3f ms  median %8.3f ms  max %8.3f ms  (%d repeats)" % (name, min(ts), statistics.median(ts), max(ts), reps))
    return min(ts), statistics.median(ts), max(ts)

f0, k0 = eng._svc_filter(None)
a = timed("gys_tdigest_rollup_dev(HOST)", lambda: capi.check(L.gys_tdigest_rollup_dev(h, 0, ps)))
b = timed("gys_hll_rollup_dev(HOST)", lambda: capi.check(L.gys_hll_rollup_dev(h, 0, pr, pe)))
eng.profile(True); eng.profile_reset()
for _ in range(REPS):
    eng.svcstate_scan(maxrecs=10)
eng.sync()
pf = eng.profile_get()
filt = pf["svc_filter"][0] / max(pf["svc_filter"][1], 1)
P("filter pass of gys_query_svcstate_scan (profile, whole scope incl. its read): %.3f ms per call" % filt, pf["svc_filter"])
eng.profile(False)
call = lambda flt, flags, gb, mr: capi.check(L.gys_rollup_filtered_dev(h, C.byref(flt), flags, gb, -1, 0, rows, mr, C.byref(n), ps, pr, pe))
c = timed("gys_rollup_filtered_dev(no terms, HOST, ANY_STATE)", lambda: call(f0, 1, 1, cap))
P("  rows", n.value, "| reference sum (min) %.3f ms + one more filter pass = allowance %.3f ms; spread of the reference calls (max - min) %.3f ms" %
  (a[0] + b[0] + filt, a[0] + b[0] + 2 * filt, (a[2] - a[0]) + (b[2] - b[0])))
eng.profile(True); eng.profile_reset()
for _ in range(REPS):
    call(f0, 1, 1, cap)
eng.sync()
P("  scopes (total ms, launches):", {k: v for k, v in eng.profile_get().items()})
eng.profile(False)
f1, k1 = eng._svc_filter(None, machine_ids=[mids[i] for i in range(0, NH, 100)])
timed("... 1 % of the services (100 hosts), by cluster", lambda: call(f1, 1, 2, 16))
P("  rows", n.value, [(rows[i].group, rows[i].nmembers) for i in range(min(n.value, 8))])
t0 = time.perf_counter()
for h0 in range(0, NH, 1000):
    ids = np.concatenate([wire.glob_id(np.full(SP, hh), s_) for hh in range(h0, h0 + 1000)])
    eng.set_service_groups(ids, ((np.arange(len(ids)) + h0 * SP) % 10000).astype(np.uint32))
P("gys_set_service_groups of 10^7 services in 10 calls: %.1f s" % (time.perf_counter() - t0))
timed("... label grouping, 10^4 groups of 1000", lambda: call(f0, 1, 3, cap), reps=REPS)
P("  rows", n.value, [(rows[i].group, rows[i].nmembers) for i in range(3)])
eng.profile(True); eng.profile_reset()
for _ in range(5):
    call(f0, 1, 3, cap)
eng.sync()
P("  scopes (total ms of 5, launches):", eng.profile_get())
eng.close()
