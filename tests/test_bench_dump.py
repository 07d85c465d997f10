"""A plain `bench.py` run does only what its headline figure needs (set-up, warm-up, the timed steps, the JSON line); everything else is
behind --full.  --dump-outputs DIR writes what the last timed step computed as .npy files (float32 / float64, <= 64 MB in all), the same
from run to run for the same arguments, so that two builds can be compared output for output."""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _arrays(d):
    files = sorted(glob.glob(os.path.join(d, "*.npy")))
    assert files
    out = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    for k, a in out.items():
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    return out


def test_bench_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


SMALL = ["--gpus", "1", "--hosts", "40", "--svcs", "100", "--events", str(1 << 22), "--nbuf", "2", "--prime-windows", "2"]


@pytest.mark.gpu
def test_plain_bench_is_lean_and_dumps_the_same_outputs_twice():
    tmp = tempfile.mkdtemp(prefix="gys_bench_dump_")
    lines = []
    for i in range(2):
        lines.append(_run(*SMALL, "--steps", "3", "--warmup", "1", "--dump-outputs", os.path.join(tmp, str(i))))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert d.get(k) is not None, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - (1 << 22) / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3  # value = events per step / step time
    # the plain line carries no figure that needs work of its own
    assert d["parity_ok"] is None and "cpu_baseline" not in d and "quantile_error" not in d and "configs" not in d and "detail" not in d
    assert "kernel" not in d["roofline"] and d["roofline"]["frac"] > 0
    a, b = _arrays(os.path.join(tmp, "0")), _arrays(os.path.join(tmp, "1"))
    assert set(a) == set(b) and {"hll", "cms0", "cms1", "global_hist", "sample_quantiles", "sample_td_sums"} <= set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["sample_slots"]) == 40 * 100 and a["sample_td_counts"].sum() > 0 and a["hll"].max() > 0


@pytest.mark.gpu
def test_full_bench_keeps_the_checks():
    d = _run(*SMALL, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-host-fed", "--detail-out", "none")
    assert d["parity_ok"] is True and d["quantile_error"]["keys_checked"] > 0
    assert d["roofline"]["kernel"] and d["roofline"]["kernel_avg_ms"] > 0


@pytest.mark.gpu
def test_plain_conn_bench_dumps_outputs():
    tmp = tempfile.mkdtemp(prefix="gys_bench_dump_conn_")
    d = _run("--workload", "conn", "--steps", "2", "--warmup", "1", "--dump-outputs", tmp)
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["parity_ok"] is None and "cpu_baseline" not in d
    a = _arrays(tmp)
    assert {"hll", "cms0", "cms1", "svc_counters", "distinct_flows"} <= set(a) and a["svc_counters"].sum() > 0
