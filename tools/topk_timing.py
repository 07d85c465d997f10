"""Timing of the rankings on sketch results at 10^7 services (10 000 hosts x 1 000) at the benchmark's gys_config (td_pend_cap 1 920, 2^29 events per
window, no levels; svc_hll_p 4 added for the distinct metric) on one MI355X, after the benchmark's own set-up as in tools/td_ranks_timing.py.
Device events on the engine's stream around the C call, 3 warm-up calls, 20 repeats.
  (i)   gys_topk_dev, k = 1 000, on a resident scan column (the p99 of every service: heavy ties, a few hundred distinct values) and on a
        distinct-valued column: the call, and its steps by profile scope (keys pass, rounds, gather, read-back).  Beside it what the parent commit
        offers for the same answer -- the device-to-pinned-host copy of the column plus np.argpartition and a sort of the k -- and
        gys_query_svcstate_scan's top-1 000 at the same size (state records of every service ingested first).
  (ii)  gys_top_services per metric: the scan's share and the selection's share by profile scope.
  (iii) gys_tdigest_slab_quantiles_dev on the 10^4 host slabs x 3 quantiles, beside the one-slab host call timed over 300 slabs and SCALED to 10^4.
Usage: python tools/topk_timing.py [output file [hosts services-per-host]]   (profiles/topk_timing.txt keeps a run)."""
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

NH, SP, NEV, REPS, CAP, K = 10000, 1000, 1 << 29, 20, 1920, 1000
if len(sys.argv) > 2:  # a rehearsal size: hosts, services per host
    NH, SP = int(sys.argv[2]), int(sys.argv[3])
    NEV = max(1 << 16, NH * SP * 54)
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def P(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True); out.write(s + "\n"); out.flush()

NSVC = NH * SP
P("device code", build.device_code_sha(), "| one MI355X |", NH, "hosts x", SP, "services, td_pend_cap", CAP, "enable_levels 0, svc_hll_p 4,", NEV, "events per window, k", K)
t0 = time.perf_counter()
eng = SketchEngine(max_hosts=NH, max_services=NSVC, max_clusters=16, enable_tdigest=True, max_batch_events=NEV, td_pend_cap=CAP, svc_hll_p=4)
s_ = np.arange(SP)
mids = [wire.machine_id(h) for h in range(NH)]
for h in range(NH):
    eng.register_host(mids[h], "cluster%d" % (h % 8))
    eng.register_listeners_np(mids[h], wire.glob_id(np.full(SP, h), s_), wire.listener_netns(h, s_), wire.listener_port(s_))
bufs = [torch.empty(NEV * 24, dtype=torch.uint8, device="cuda") for _ in range(2)]
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
eng.handle_resp_events_dev(segs[0], bufs[0].data_ptr(), NEV)  # the open window holds events (the distinct metric reads its registers)
eng.sync()
del bufs
P("setup %.1f s: de-phase pass of %d batches, then %d windows and an open one" % (time.perf_counter() - t0, nb, nwin))
L, h = eng.L, eng.h
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
    P("%-72s min %8.3f ms  median %8.3f ms  max %8.3f ms  (%d repeats)" % (name, min(ts), statistics.median(ts), max(ts), reps))
    return statistics.median(ts)

def scopes(fn, reps=REPS):
    eng.profile(True); eng.profile_reset()
    for _ in range(reps):
        fn()
    eng.sync()
    pf = eng.profile_get()
    eng.profile(False)
    return {k: v[0] / reps for k, v in pf.items()}

def scope_line(what, sc, names):
    P("  %s by profile scope (ms per call): %s" % (what, ", ".join("%s %.3f" % (n, sc.get(n, 0.0)) for n in names)))

# ---- (i) gys_topk_dev on a resident column
qa = (C.c_double * 1)(0.99)
p99 = torch.empty(NSVC, dtype=torch.float64, device="cuda")
capi.check(L.gys_scan_quantiles_dev(h, qa, 1, C.c_void_p(p99.data_ptr())))
eng.sync()
distinct_col = (p99 + torch.rand(NSVC, dtype=torch.float64, device="cuda")).contiguous()
torch.cuda.synchronize()
ent = (capi.TopkEntry * K)()
nout, nel = C.c_uint32(), C.c_uint64()
TOPK_SCOPES = ("topk_keys", "topk_rounds", "topk_gather", "topk_read")
for name, col in (("the p99 column (%d distinct values)" % len(torch.unique(p99)), p99), ("a distinct-valued column", distinct_col)):
    call = lambda: capi.check(L.gys_topk_dev(h, C.c_void_p(col.data_ptr()), 1, NSVC, None, None, 0, capi.TOPK_LARGEST, K, ent, C.byref(nout), C.byref(nel)))
    timed("gys_topk_dev(k = %d) on %s" % (K, name), call)
    scope_line("gys_topk_dev", scopes(call), TOPK_SCOPES)
    # what the parent offers: the column to pinned host memory, np.argpartition, the k sorted (wall clock: the host part is not on the stream)
    pinned = torch.empty(NSVC, dtype=torch.float64).pin_memory()
    ts_copy, ts_host = [], []
    for r in range(3 + 5):
        torch.cuda.synchronize()
        a = time.perf_counter()
        pinned.copy_(col, non_blocking=True); torch.cuda.synchronize()
        b = time.perf_counter()
        v = pinned.numpy()
        part = np.argpartition(-v, K)[:K]
        order = part[np.lexsort((part, -v[part]))]
        c = time.perf_counter()
        if r >= 3:
            ts_copy.append((b - a) * 1e3); ts_host.append((c - b) * 1e3)
    P("  the host round trip it replaces (5 repeats, wall clock): copy of %.0f MB to pinned memory median %.3f ms + np.argpartition and sort median %.3f ms" %
      (NSVC * 8 / 1e6, statistics.median(ts_copy), statistics.median(ts_host)))
    assert [ent[i].row for i in range(nout.value)][:5] == order[:5].tolist() or len(torch.unique(col)) < NSVC  # (argpartition cuts ties anywhere)
    del pinned

# ---- (ii) gys_top_services per metric
svc = (capi.TopService * K)()
for mname, metric, param, scan_scopes in (("GYS_TOP_QUANTILE(0.99)", capi.TOP_QUANTILE, 0.99, ("scan_quantiles", "scan_ranks")), ("GYS_TOP_SHARE_WITHIN(100 ms)", capi.TOP_SHARE_WITHIN, 100.0, ("scan_ranks", "top_metric")),
                                          ("GYS_TOP_MISSES(100 ms)", capi.TOP_MISSES, 100.0, ("scan_ranks", "top_metric")), ("GYS_TOP_DISTINCT(open window)", capi.TOP_DISTINCT, 0.0, ("hll_scan", "top_metric"))):
    call = lambda: capi.check(L.gys_top_services(h, metric, param, -1, 0, None, 0, 0, capi.TOPK_LARGEST, K, svc, C.byref(nout), C.byref(nel)))
    med = timed("gys_top_services(%s, k = %d)" % (mname, K), call)
    sc = scopes(call)
    scan = sum(sc.get(n, 0.0) for n in scan_scopes)
    sel = sum(sc.get(n, 0.0) for n in TOPK_SCOPES)
    P("  the scan's share %.3f ms (%s), the selection's share %.3f ms (%s); %d eligible, first slot %d value %.6g total %d" %
      (scan, " + ".join(scan_scopes), sel, " + ".join(TOPK_SCOPES), nel.value, svc[0].slot, svc[0].value, svc[0].total))

# ---- (iii) the host slabs' quantiles
slabs = torch.zeros(NH * C.sizeof(capi.TDigestSlab), dtype=torch.uint8, device="cuda")
capi.check(L.gys_tdigest_rollup_dev(h, capi.ROLLUP_HOST, C.c_void_p(slabs.data_ptr())))
eng.sync()
q3 = (C.c_double * 3)(0.25, 0.95, 0.99)
qo = torch.empty((NH, 3), dtype=torch.float64, device="cuda")
call = lambda: capi.check(L.gys_tdigest_slab_quantiles_dev(h, C.c_void_p(slabs.data_ptr()), NH, q3, 3, C.c_void_p(qo.data_ptr())))
timed("gys_tdigest_slab_quantiles_dev(%d host slabs, 3 quantiles)" % NH, call)
scope_line("k_td_slab_quantiles", scopes(call), ("slab_quantiles",))
nsome = min(300, NH)
o3 = (C.c_double * 3)()
eng.sync()
a = time.perf_counter()
for i in range(nsome):
    capi.check(L.gys_tdigest_slab_quantiles(h, C.c_void_p(slabs.data_ptr() + i * C.sizeof(capi.TDigestSlab)), q3, 3, o3))
b = time.perf_counter()
P("  the one-slab host call over %d slabs: %.3f ms each (wall clock); SCALED to %d slabs: %.1f ms" % (nsome, (b - a) * 1e3 / nsome, NH, (b - a) * 1e3 / nsome * NH))
assert qo[nsome - 1].cpu().tolist() == list(o3)

# ---- gys_query_svcstate_scan's top-1 000 at the same size: a state record for every service first
t0 = time.perf_counter()
rng = np.random.default_rng(1)
for hh in range(NH):
    rec = np.zeros(SP, dtype=wire.LISTENER_STATE_NOTIFY)
    rec["glob_id"] = wire.glob_id(np.full(SP, hh), s_)
    rec["nqrys_5s"] = rng.integers(0, 100000, SP)
    rec["p95_5s_resp_ms"] = rng.integers(0, 5000, SP)
    eng.partha_listener_state(mids[hh], rec.tobytes(), SP)
eng.sync()
P("state records of %d services ingested in %.1f s" % (NSVC, time.perf_counter() - t0))
rows = (capi.SvcRow * K)()
nm = C.c_uint64()
call = lambda: capi.check(L.gys_query_svcstate_scan(h, None, capi.SVC_COLS.index("p95resp5s"), 1, K, rows, C.byref(nout), C.byref(nm)))
timed("gys_query_svcstate_scan(sorted by p95resp5s, top %d)" % K, call)
P("  %d records matched, %d written" % (nm.value, nout.value))
eng.close()
