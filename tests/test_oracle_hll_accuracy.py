"""What the distinct-flow numbers mean, on the oracle alone (no GPU): flows drawn as tests/helpers.make_resp_events draws them, hashed
into per-service HyperLogLog files with gyo_hll_add_words (the reference's own flow-key bytes), files merged per host with gyo_hll_merge,
gyo_hll_estimate against the EXACT distinct count (numpy.unique over the flow words).  Gate: relative error <= 4 x 1.04 / sqrt(m) -- the
standard error of the estimator (Flajolet, Fusy, Gandouet, Meunier 2007), four of them because the seeds are fixed -- for counts in the
raw range (above 2.5 m), p = 8 and 10.  The device kernels are held to these same functions byte for byte / to 1e-12
(tests/test_gpu_hll_rollup.py, tests/test_kernel_logic_hll_cpu.py)."""
import numpy as np
import pytest

from tests import helpers


def _flows(ev, sp):
    """kept events of a batch as (service index, flow-key words): the filters of the event kernel (latency range, known listener)"""
    lat = (ev["lsndtime"] - ev["lrcvtime"]).astype(np.uint32)
    svc = ev["sport_be"].astype(np.int64) - 1024
    keep = (lat <= 1000000) & (svc >= 0) & (svc < sp)
    for daddr, dport, saddr, sport, s, k in zip(ev["daddr"].tolist(), ev["dport_be"].tolist(), ev["saddr"].tolist(), ev["sport_be"].tolist(), svc.tolist(), keep.tolist()):
        if k:
            yield s, tuple(([daddr] if daddr else [0, 0, 0, 0]) + [dport] + ([saddr] if saddr else [0, 0, 0, 0]) + [sport])


@pytest.mark.parametrize("P", [8, 10])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_estimate_against_exact_distinct_count(oracle, P, seed):
    L = oracle.lib()
    m = 1 << P
    gate = 4 * 1.04 / np.sqrt(m)
    rng = np.random.default_rng(1000 * P + seed)
    # (host, services, events): per-service and per-host counts from about 3 m to 100 m distinct flows
    worlds = [(0, 2, 8 * m), (1, 5, 60 * m), (2, 1, 110 * m), (3, 3, 12 * m)]
    checked = 0
    worst = 0.0
    for h, sp, n in worlds:
        regs = np.zeros((sp, m), dtype=np.uint8)
        words = [[] for _ in range(sp)]
        for part in range(2):
            ev = helpers.make_resp_events(rng, h, n // 2, sp)
            if part:
                ev[: n // 8] = first[: n // 8]  # a quarter of the second batch repeats flows of the first: a flow counts once
            first = ev
            for s, w in _flows(ev, sp):
                wa = np.array(w, dtype=np.uint32)
                L.gyo_hll_add_words(oracle.ptr(regs[s], oracle.u8p), P, oracle.ptr(wa, oracle.u32p), len(wa))
                words[s].append(list(w) + [0] * (10 - len(w)) + [len(w)])
        host = np.zeros(m, dtype=np.uint8)
        for s in range(sp):
            L.gyo_hll_merge(oracle.ptr(host, oracle.u8p), oracle.ptr(regs[s], oracle.u8p), P)
        assert (host == regs.max(axis=0)).all()

        def distinct(rows):
            return len(np.unique(np.array(rows, dtype=np.uint64), axis=0)) if rows else 0
        files = [(regs[s], distinct(words[s]), f"host {h} service {s}") for s in range(sp)] + [(host, distinct(sum(words, [])), f"host {h}")]
        for row, exact, what in files:
            if exact <= 2.5 * m:
                continue
            est = float(L.gyo_hll_estimate(oracle.ptr(np.ascontiguousarray(row), oracle.u8p), P))
            rel = abs(est - exact) / exact
            worst = max(worst, rel)
            print(f"p {P} seed {seed} {what}: exact {exact} estimate {est:.1f} relative error {rel:.4f} (gate {gate:.4f})")
            assert rel <= gate, f"{what}: exact {exact}, estimate {est}, relative error {rel:.4f} > {gate:.4f}"
            checked += 1
    assert checked >= 8, checked
