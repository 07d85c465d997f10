"""HIP-event times (gys_profile_*) of the distinct-count levels (gys_config.svc_hll_levels) on one GPU, one JSON line per configuration:
the close kernel k_hll_level_roll without / with a ring-boundary crossing beside a device-to-device copy of the same number of bytes, the
whole window close with svc_hll_levels 0 and 1 alternated, and the level scans / host roll-up beside their open-window siblings.
    python tools/hll_levels_timing.py [--cases 10000x1000x4,1000x1000x8] [--events 16777216] [--closes 12]
Bytes are the algorithmic ones of DESIGN.md section 5 (close: 4 m read + 5 m written per service; view: live buckets x m per service)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gyeeta_amd import capi  # noqa: E402
from gyeeta_amd.engine import SketchEngine  # noqa: E402
from tests import helpers  # noqa: E402


def _ms(eng, name):
    ms, n = eng.profile_get().get(name, (0.0, 0))
    return (ms / n if n else None), n


def run(nh, sp, P, nev, ncloses):
    m, nsvc = 1 << P, nh * sp
    engs = {}
    for lv in (0, 1):
        e = SketchEngine(max_hosts=nh + 2, max_services=nsvc + 64, max_batch_events=nev, enable_tdigest=False, svc_hll_p=P, svc_hll_levels=lv)
        helpers.register_world(e, None, range(nh), sp)
        e.profile(True)
        engs[lv] = e
    ev = torch.empty(nev * 24, dtype=torch.uint8, device="cuda")
    base = 1_700_000_000 - 1_700_000_000 % 432000
    res = {"hosts": nh, "services": nsvc, "p": P, "events_per_window": nev, "close_bytes": 9 * m * nsvc}
    for crossing in (False, True):
        for e in engs.values():
            e.sync()
            e.profile_reset()
        for k in range(ncloses):
            # without a crossing: every close inside one 30-s bucket of a fresh 300-s period; with: every close 30 s after the last one
            t = base + (600 + 10 + k if not crossing else 1200 + 30 * (k + 1))
            for lv in (0, 1):
                e = engs[lv]
                segs = e.gen_resp_events(ev.data_ptr(), nev, 0x700 + k, 0, nh, sp)
                e.handle_resp_events_dev(segs, ev.data_ptr(), nev)
                e.window_close(t * 1_000_000)
                e.sync()
        tag = "crossing" if crossing else "plain"
        roll, n = _ms(engs[1], "hll_level_roll")
        res[f"roll_ms_{tag}"] = roll
        res[f"roll_launches_{tag}"] = n
        res[f"roll_TBps_{tag}"] = res["close_bytes"] / (roll * 1e-3) / 1e12 if roll else None
        for lv in (0, 1):
            res[f"close_graph_ms_levels{lv}_{tag}"] = _ms(engs[lv], "window_close_graph")[0]
    # a device-to-device copy that moves the same number of bytes (half read, half written)
    half = res["close_bytes"] // 2
    a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(10):
        b.copy_(a)
    t1.record()
    torch.cuda.synchronize()
    res["copy_ms_same_bytes"] = t0.elapsed_time(t1) / 10
    res["copy_TBps"] = res["close_bytes"] / (res["copy_ms_same_bytes"] * 1e-3) / 1e12
    del a, b
    # queries: the last close was at `t`; the open window gets events so that the open-window calls have something to read
    e = engs[1]
    segs = e.gen_resp_events(ev.data_ptr(), nev, 0x7ff, 0, nh, sp)
    e.handle_resp_events_dev(segs, ev.data_ptr(), nev)
    e.sync()
    e.profile_reset()
    out = torch.zeros(nsvc, dtype=torch.float64, device="cuda")
    hest = torch.zeros(nh + 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    reps = 10
    for _ in range(reps):
        capi.check(e.L.gys_scan_distinct_dev(e.h, out.data_ptr()))
        capi.check(e.L.gys_hll_rollup_dev(e.h, capi.ROLLUP_HOST, None, hest.data_ptr()))
        capi.check(e.L.gys_hll_rollup_level_dev(e.h, capi.ROLLUP_HOST, 1, t * 1_000_000, None, hest.data_ptr()))
    e.sync()
    res["open_scan_ms"] = _ms(e, "hll_scan")[0]
    res["open_rollup_hosts_ms"] = _ms(e, "hll_rollup_hosts")[0]  # (per launch; the level roll-up runs the same launches on the scratch files)
    res["level1_files_ms"] = _ms(e, "hll_level_files")[0]
    for lvl in range(4):
        e.profile_reset()
        for _ in range(reps):
            capi.check(e.L.gys_scan_distinct_level_dev(e.h, lvl, t * 1_000_000, out.data_ptr()))
        e.sync()
        res[f"level{lvl}_scan_ms"] = _ms(e, "hll_level_scan")[0]
    res["live_buckets_level1"] = ncloses if ncloses < 10 else 10
    for x in engs.values():
        x.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10000x1000x4,1000x1000x8")
    ap.add_argument("--events", type=int, default=1 << 24)
    ap.add_argument("--closes", type=int, default=12)
    a = ap.parse_args()
    for case in a.cases.split(","):
        nh, sp, P = (int(x) for x in case.split("x"))
        print(json.dumps(run(nh, sp, P, a.events, a.closes)), flush=True)


if __name__ == "__main__":
    main()
