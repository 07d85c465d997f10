"""Distinct-flow counts per service, host, cluster and rank on the device (gys_scan_distinct_dev, gys_query_distinct, gys_hll_rollup_dev,
gys_hll_merge_files_dev, gys_hll_global_rccl; kernels in gyeeta_amd/csrc/gys_hllroll.hpp):
  * group register files are the byte-wise maximum of the members' rows of gys_export_svc_hll and equal the files the oracle builds
    from the reference's own flow-key bytes (gyo_hll_add_words + gyo_hll_merge);
  * estimates equal gyo_hll_estimate on the same bytes within 1e-12 relative: both sides add at most 1024 positive terms, each
    addition off by at most 2^-53 relative (2 x 1023 x 1.1e-16 = 2.3e-13), plus a few ulp for the division and the logarithm;
  * the open-window rule, no side effects, registrations, the union of caller-supplied files, one and two ranks, the error codes."""
import ctypes as C
import os

import numpy as np
import pytest

from gyeeta_amd import capi, wire
from tests import helpers

pytestmark = pytest.mark.gpu

EST_RTOL = 1e-12
# hosts 0..11 in clusters h % 3; services per host: host 3 has none, host 7's services get no events
SVCS = [5, 1, 9, 0, 17, 3, 40, 6, 2, 11, 4, 8]
NHOSTS = len(SVCS)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    return torch


def _engine(**kw):
    from gyeeta_amd.engine import SketchEngine
    return SketchEngine(**kw)


def _flow_words(ev):
    """the bytes PAIR_IP_PORT(cli = daddr:dport, ser = saddr:sport).get_hash() hashes as u32 words (as tests/test_gpu_round2.py builds them)"""
    out = []
    for daddr, dport, saddr, sport in zip(ev["daddr"].tolist(), ev["dport_be"].tolist(), ev["saddr"].tolist(), ev["sport_be"].tolist()):
        w = ([daddr] if daddr else [0, 0, 0, 0]) + [dport] + ([saddr] if saddr else [0, 0, 0, 0]) + [sport]
        out.append(np.array(w, dtype=np.uint32))
    return out


def _world(eng, hosts=range(NHOSTS)):
    """registers the hosts with their uneven service counts; {host: (machine id, host slot, glob ids)}"""
    info = {}
    for h in hosts:
        mid = wire.machine_id(h)
        slot = eng.register_host(mid, "cluster%d" % (h % 3))
        s = np.arange(SVCS[h])
        g = wire.glob_id(np.full(SVCS[h], h), s)
        if SVCS[h]:
            eng.register_listeners_np(mid, g, wire.listener_netns(h, s), wire.listener_port(s))
        info[h] = (mid, slot, g)
    return info


def _feed(eng, oracle, info, rng, P, counts, regs=None):
    """counts: {host: events}; regs (optional): the oracle's per-slot files, updated from the same events"""
    L = oracle.lib()
    for h, n in counts.items():
        sp = SVCS[h]
        ev = helpers.make_resp_events(rng, h, n, sp, zero_ip_frac=0.03)
        eng.handle_resp_events(info[h][0], ev)
        if regs is None:
            continue
        lat = (ev["lsndtime"] - ev["lrcvtime"]).astype(np.uint32)
        svc = ev["sport_be"].astype(np.int64) - 1024
        keep = (lat <= 1000000) & (svc >= 0) & (svc < sp)
        for w, s, k in zip(_flow_words(ev), svc.tolist(), keep.tolist()):
            if k:
                slot = eng.lookup(int(info[h][2][s]))
                L.gyo_hll_add_words(oracle.ptr(regs[slot], oracle.u8p), P, oracle.ptr(w, oracle.u32p), len(w))


def _members(eng, info):
    """service slots of every host slot, host slots of every cluster index (cluster c = hosts with h % 3 == c: registered in that order)"""
    hosts = {info[h][1]: [eng.lookup(int(g)) for g in info[h][2]] for h in info}
    clusters = {c: [info[h][1] for h in info if h % 3 == c] for c in range(3)}
    return hosts, clusters


def _union(rows, m):
    rows = list(rows)
    return np.maximum.reduce(rows) if rows else np.zeros(m, dtype=np.uint8)


def _oracle_merge(oracle, rows, P):
    out = np.zeros(1 << P, dtype=np.uint8)
    for r in rows:
        oracle.lib().gyo_hll_merge(oracle.ptr(out, oracle.u8p), oracle.ptr(np.ascontiguousarray(r), oracle.u8p), P)
    return out


def _oracle_est(oracle, row, P):
    L = oracle.lib()
    L.gyo_hll_estimate.restype = C.c_double
    return float(L.gyo_hll_estimate(oracle.ptr(np.ascontiguousarray(row), oracle.u8p), P))


def _raw(row, P):
    """the raw estimator alpha m^2 / sum 2^-rank of a file (the value the estimator's switch at 2.5 m looks at)"""
    m = 1 << P
    alpha = {16: 0.673, 32: 0.697, 64: 0.709}.get(m, 0.7213 / (1.0 + 1.079 / m))
    return alpha * m * m / float(np.ldexp(1.0, -row.astype(np.int64)).sum())


def _close(got, want):
    return got == want if want == 0.0 else abs(got - want) <= EST_RTOL * abs(want)


# events per host: a spread that puts services, hosts, clusters and the rank on both sides of the 2.5 m switch for every p tested
COUNTS = {0: 900, 1: 30, 2: 2500, 4: 6000, 5: 40, 6: 9000, 8: 12, 9: 3000, 10: 200, 11: 1500}


@pytest.mark.parametrize("resp_path", [1, 2], ids=["general", "hostlocal"])
@pytest.mark.parametrize("P", [4, 8, 10])
def test_files_bit_exact_and_estimates(torch_mod, oracle, P, resp_path):
    """checks 1 and 2 of the issue: HOST / CLUSTER / GLOBAL files == numpy maximum over the exported rows == gyo_hll_add_words + gyo_hll_merge;
    the scan, the one-service query and the roll-up estimates against gyo_hll_estimate on the same bytes; both estimator branches reached and
    no value near the switch; scan and query the same bits; untouched service exactly 0.0"""
    rng = np.random.default_rng(77 + P)
    m = 1 << P
    eng = _engine(max_hosts=16, max_services=128, max_batch_events=1 << 16, svc_hll_p=P, resp_path=resp_path)
    assert eng.L.gys_hll_file_bytes(eng.h) == m
    info = _world(eng)
    nsvc = eng.num_services()
    assert nsvc == sum(SVCS)
    regs = np.zeros((nsvc, m), dtype=np.uint8)
    for rnd in range(3):
        _feed(eng, oracle, info, rng, P, COUNTS, regs)
    eng.sync()
    rows = eng.export_svc_hll()
    assert (rows == regs).all()
    hosts, clusters = _members(eng, info)
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    cf, ce = eng.hll_rollup(capi.ROLLUP_CLUSTER)
    gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    assert hf.shape == (NHOSTS, m) and cf.shape == (3, m) and gf.shape == (1, m) and he.shape == (NHOSTS,) and ge.shape == (1,)
    for hs, slots in hosts.items():
        assert (hf[hs] == _union((rows[s] for s in slots), m)).all(), f"host slot {hs}"
        assert (hf[hs] == _oracle_merge(oracle, [regs[s] for s in slots], P)).all(), f"host slot {hs} (oracle)"
    assert hf[info[3][1]].sum() == 0 and hf[info[7][1]].sum() == 0  # the host without services, the host without events
    for c, hl in clusters.items():
        assert (cf[c] == _union((hf[h] for h in hl), m)).all(), f"cluster {c}"
        assert (cf[c] == _oracle_merge(oracle, [regs[s] for h in hl for s in hosts[h]], P)).all(), f"cluster {c} (oracle)"
    assert (gf[0] == _union(rows, m)).all() and (gf[0] == _oracle_merge(oracle, regs, P)).all()
    # estimates only (no files asked for): the same doubles
    for scope, e in ((capi.ROLLUP_HOST, he), (capi.ROLLUP_CLUSTER, ce), (capi.ROLLUP_GLOBAL, ge)):
        none, e2 = eng.hll_rollup(scope, want_regs=False)
        assert none is None and e2.tobytes() == e.tobytes()
    scan = eng.scan_distinct()
    assert scan.shape == (nsvc,)
    lin = raw = 0
    cases = [(scan[s], rows[s], f"service {s}") for s in range(nsvc)] + [(he[h], hf[h], f"host {h}") for h in range(NHOSTS)] + \
            [(ce[c], cf[c], f"cluster {c}") for c in range(3)] + [(ge[0], gf[0], "global")]
    for got, row, what in cases:
        want = _oracle_est(oracle, row, P)
        print(f"p {P} {what}: {got!r} oracle {want!r}")
        rawv = _raw(row, P)
        assert abs(want - 2.5 * m) > 1e-9 * 2.5 * m and abs(rawv - 2.5 * m) > 1e-9 * 2.5 * m, f"{what}: a value on the switch between the estimator's branches"
        assert _close(got, want), f"{what}: {got!r}, oracle {want!r}"
        if want > 0:
            if (row == 0).any() and rawv <= 2.5 * m:
                lin += 1
            else:
                assert want == rawv or abs(want - rawv) <= 1e-12 * rawv
                raw += 1
    assert lin >= 3 and raw >= 3, f"p {P}: {lin} linear-counting and {raw} raw cases"
    for h in info:
        for g in info[h][2]:
            q = eng.query_distinct(int(g))
            assert np.float64(q).tobytes() == scan[eng.lookup(int(g))].tobytes()
    for s in hosts[info[7][1]]:
        assert scan[s].tobytes() == np.float64(0.0).tobytes()  # +0.0 exactly
    assert he[info[3][1]] == 0.0 and he[info[7][1]] == 0.0
    eng.close()


def test_many_services_several_chunks_per_host(torch_mod):
    """check 3: 105 000 services at p = 4, every host's member list spans three chunks of GYS_RB_CHUNK_SERVICES = 1024 (one host with a
    single chunk and one empty host besides), events from gys_gen_resp_events_dev"""
    torch = torch_mod
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gyeeta_amd", "csrc", "gys_engine.hip")).read()
    import re
    chunk = int(re.search(r"#define GYS_RB_CHUNK_SERVICES (\d+)u", src).group(1))
    nh, sp, n, P = 50, 2100, 1 << 22, 4
    assert sp > 2 * chunk and nh * sp >= 100_000
    m = 1 << P
    eng = _engine(max_hosts=nh + 2, max_services=nh * sp + 64, max_batch_events=n, svc_hll_p=P)
    helpers.register_world(eng, None, range(nh), sp)
    small = wire.machine_id(nh)
    s = np.arange(7)
    eng.register_host(small, "cluster1")
    eng.register_listeners_np(small, wire.glob_id(np.full(7, nh), s), wire.listener_netns(nh, s), wire.listener_port(s))
    eng.register_host(wire.machine_id(nh + 1), "cluster2")  # no services
    ev = torch.empty(n * 24, dtype=torch.uint8, device="cuda")
    for rnd in range(2):
        segs = eng.gen_resp_events(ev.data_ptr(), n, 0x411 + rnd, 0, nh, sp)
        eng.handle_resp_events_dev(segs, ev.data_ptr(), n)
        eng.sync()
    eng.handle_resp_events(small, helpers.make_resp_events(np.random.default_rng(5), nh, 300, 7))
    eng.sync()
    rows = eng.export_svc_hll()
    nsvc = eng.num_services()
    assert rows.shape == (nsvc, m) and nsvc == nh * sp + 7
    assert (rows[:nh * sp].max(axis=1) > 0).mean() > 0.9  # the generator reached the services
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    for h in range(nh):  # register_world: host slot h owns the slots [h * sp, (h + 1) * sp)
        assert (hf[h] == rows[h * sp:(h + 1) * sp].max(axis=0)).all(), f"host {h}"
    assert (hf[nh] == rows[nh * sp:].max(axis=0)).all() and hf[nh + 1].sum() == 0
    assert (gf[0] == rows.max(axis=0)).all()
    scan = eng.scan_distinct()
    assert scan.shape == (nsvc,) and ((scan > 0) == (rows.max(axis=1) > 0)).all()
    assert (eng.export_svc_hll() == rows).all()
    eng.close()


def test_no_side_effects_registrations_and_window_close(torch_mod, oracle):
    """checks 4 and 5: the registers are unchanged by every new call, a second call returns the same bytes, a host registered later is
    included after it received events, and after window_close every file is zero and every estimate 0.0"""
    P = 8
    m = 1 << P
    rng = np.random.default_rng(91)
    eng = _engine(max_hosts=16, max_services=160, max_batch_events=1 << 16, svc_hll_p=P)
    first = [h for h in range(NHOSTS) if h != 6]
    info = _world(eng, first)
    _feed(eng, oracle, info, rng, P, {h: n for h, n in COUNTS.items() if h != 6})
    eng.sync()
    rows = eng.export_svc_hll()

    def everything():
        out = [eng.scan_distinct().tobytes()]
        for scope in (capi.ROLLUP_HOST, capi.ROLLUP_CLUSTER, capi.ROLLUP_GLOBAL):
            f, e = eng.hll_rollup(scope)
            out += [f.tobytes(), e.tobytes()]
        hf, _ = eng.hll_rollup(capi.ROLLUP_HOST)
        f, e = eng.hll_merge_files(hf)
        out += [f.tobytes(), np.float64(e).tobytes(), np.float64(eng.query_distinct(int(info[0][2][0]))).tobytes()]
        return out
    a = everything()
    assert (eng.export_svc_hll() == rows).all()
    b = everything()
    assert a == b and (eng.export_svc_hll() == rows).all()
    # a digest roll-up in between shares the hosts' member lists
    eng.tdigest_rollup(capi.ROLLUP_CLUSTER)
    assert everything() == a
    # another host with services, and events for it
    info.update(_world(eng, [6]))
    gf0, _ = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    assert gf0.tobytes() == a[5]  # registered, no events yet: nothing changes
    _feed(eng, oracle, info, rng, P, {6: 5000})
    eng.sync()
    rows2 = eng.export_svc_hll()
    assert rows2.shape[0] == rows.shape[0] + SVCS[6] and (rows2[:rows.shape[0]] == rows).all()
    hosts, clusters = _members(eng, info)
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    cf, _ = eng.hll_rollup(capi.ROLLUP_CLUSTER)
    gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    assert hf.shape[0] == NHOSTS
    for hs, slots in hosts.items():
        assert (hf[hs] == _union((rows2[s] for s in slots), m)).all()
    assert hf[info[6][1]].sum() > 0 and he[info[6][1]] > 0
    for c, hl in clusters.items():
        assert (cf[c] == _union((hf[h] for h in hl), m)).all()
    assert (gf[0] == _union(rows2, m)).all() and ge[0] > 0
    # a host that moves to another cluster: the clusters' lists follow
    eng.register_host(info[0][0], "cluster2")
    cf2, _ = eng.hll_rollup(capi.ROLLUP_CLUSTER)
    assert (cf2[0] == _union((hf[info[h][1]] for h in info if h % 3 == 0 and h != 0), m)).all()
    assert (cf2[2] == _union((hf[info[h][1]] for h in info if h % 3 == 2 or h == 0), m)).all()
    assert (cf2[1] == cf[1]).all()
    # the open-window rule
    eng.window_close()
    assert eng.export_svc_hll().sum() == 0
    for scope in (capi.ROLLUP_HOST, capi.ROLLUP_CLUSTER, capi.ROLLUP_GLOBAL):
        f, e = eng.hll_rollup(scope)
        assert f.sum() == 0 and e.tobytes() == np.zeros(len(e)).tobytes()
    assert eng.scan_distinct().tobytes() == np.zeros(eng.num_services()).tobytes()
    assert eng.query_distinct(int(info[6][2][0])) == 0.0
    eng.close()


def test_merge_files(torch_mod, oracle):
    """check 6, first half: the union of the 12 host files is the GLOBAL file with the GLOBAL estimate, the union of one file is that file;
    2 500 caller-made files (three chunks) against numpy"""
    torch = torch_mod
    P = 10
    m = 1 << P
    rng = np.random.default_rng(17)
    eng = _engine(max_hosts=16, max_services=128, max_batch_events=1 << 16, svc_hll_p=P)
    info = _world(eng)
    _feed(eng, oracle, info, rng, P, COUNTS)
    eng.sync()
    hf, he = eng.hll_rollup(capi.ROLLUP_HOST)
    gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
    f, e = eng.hll_merge_files(hf)
    assert (f == gf[0]).all() and np.float64(e).tobytes() == ge[0].tobytes() and e > 0
    busy = info[6][1]
    f1, e1 = eng.hll_merge_files(hf[busy:busy + 1])
    assert (f1 == hf[busy]).all() and np.float64(e1).tobytes() == he[busy].tobytes()
    many = rng.integers(0, 256, (2500, m), dtype=np.uint8)  # any byte values
    many[::7] = 0
    fm, _ = eng.hll_merge_files(many)
    assert (fm == many.max(axis=0)).all()
    # estimate only / file only through the C ABI
    d_in = torch.from_numpy(hf.reshape(-1).copy()).cuda()
    d_est = torch.zeros(1, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(m, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi.check(eng.L.gys_hll_merge_files_dev(eng.h, C.c_void_p(d_in.data_ptr()), NHOSTS, None, C.c_void_p(d_est.data_ptr())))
    capi.check(eng.L.gys_hll_merge_files_dev(eng.h, C.c_void_p(d_in.data_ptr()), NHOSTS, C.c_void_p(d_out.data_ptr()), None))
    eng.sync()
    assert d_est.cpu().numpy().tobytes() == ge.tobytes() and (d_out.cpu().numpy() == gf[0]).all()
    eng.close()


def _one_rank_worker(q):
    """body of test_global_rccl_one_rank in its own process (RCCL's bootstrap does not return on part of the GPU pool)"""
    import torch
    from oracle import oracle
    try:
        P = 8
        rng = np.random.default_rng(33)
        eng = _engine(max_hosts=16, max_services=128, max_batch_events=1 << 16, svc_hll_p=P)
        info = _world(eng)
        L = eng.L
        uid = (C.c_uint8 * 128)()
        capi.check(L.gys_rccl_unique_id(uid))
        comm = C.c_void_p()
        q.put("joining")
        rc = L.gys_rccl_comm_create(eng.h, uid, 1, 0, C.byref(comm))
        if rc != capi.OK:
            q.put("bootstrap-failed: " + L.gys_last_error().decode(errors="replace"))
            return
        q.put("joined")
        eng.comm = comm
        _feed(eng, oracle, info, rng, P, COUNTS)
        eng.sync()
        gf, ge = eng.hll_rollup(capi.ROLLUP_GLOBAL)
        f, e = eng.hll_global_rccl()
        assert gf.sum() > 0 and (f == gf[0]).all() and np.float64(e).tobytes() == ge[0].tobytes()
        d_est = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        capi.check(L.gys_hll_global_rccl(eng.h, comm, None, C.c_void_p(d_est.data_ptr())))
        assert d_est.cpu().numpy().tobytes() == ge.tobytes()
        eng.leave_rccl()
        eng.close()
        q.put("ok")
    except BaseException as ex:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put("error: " + "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))[-1500:])


def test_global_rccl_one_rank(torch_mod):
    """check 6: gys_hll_global_rccl with a one-rank communicator made through the C ABI equals the GLOBAL roll-up (pattern:
    tests/test_gpu_round2.py::test_window_close_rccl_inside_the_library, its treatment of a box whose RCCL bootstrap stalls included)"""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(q,))
    p.start()
    seen = []
    try:
        while True:
            msg = q.get(timeout=75 if seen else 150)
            seen.append(msg)
            if msg == "ok" or msg.startswith("error") or msg.startswith("bootstrap-failed"):
                break
    except queue.Empty:
        p.kill()
        p.join(timeout=30)
        if seen and seen[-1] in ("joining", "joined"):
            pytest.skip(f"RCCL did not return within 75 s on this box (after {seen[-1]!r}); the in-library exchange was not exercised")
        pytest.fail(f"RCCL worker stalled after {seen}")
    p.join(timeout=60)
    if seen[-1].startswith("bootstrap-failed"):
        pytest.skip("ncclCommInitRank returned an error on this box (" + seen[-1] + "); the in-library exchange was not exercised")
    assert seen[-1] == "ok", seen[-1]


def _fake_rank(rank, q_uid, q_res):
    """one rank of test_global_rccl_two_ranks: its shard of the hosts, the in-library all-gather + union"""
    import torch
    from gyeeta_amd.engine import mid_buf
    from oracle import oracle
    try:
        torch.cuda.set_device(0)
        P = 8
        L = capi.load()
        glob = C.CDLL(os.environ["GYS_RCCL_LIB"])
        glob.fakerccl_allgather_calls.restype = C.c_uint64
        mine = [h for h in range(NHOSTS) if L.gys_shard_of(mid_buf(wire.machine_id(h)), 2) == rank]
        eng = _engine(max_hosts=16, max_services=128, max_batch_events=1 << 16, svc_hll_p=P, rank=rank, nranks=2, device=0)
        info = _world(eng, mine)
        rng = np.random.default_rng(100 + rank)
        _feed(eng, oracle, info, rng, P, {h: n for h, n in COUNTS.items() if h in mine})
        eng.sync()
        if rank == 0:
            uid = bytes(eng.rccl_unique_id())
            q_uid.put(uid)
        else:
            uid = q_uid.get(timeout=120)
        eng.join_rccl(uid)
        local, le = eng.hll_rollup(capi.ROLLUP_GLOBAL)
        merged, me = eng.hll_global_rccl()
        calls = int(glob.fakerccl_allgather_calls())
        after, _ = eng.hll_rollup(capi.ROLLUP_GLOBAL)
        eng.leave_rccl()
        eng.close()
        q_res.put((rank, "ok", local.tobytes(), merged.tobytes(), me, calls, len(mine), after.tobytes()))
    except BaseException as ex:  # noqa: BLE001 -- reported to the parent
        import traceback
        q_res.put((rank, "error: " + "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))[-2000:]))


def test_global_rccl_two_ranks(torch_mod, oracle):
    """check 6: two ranks (two processes on the one GPU, the RCCL entry points served by tests/cpp/fakerccl as in
    tests/test_gpu_round3.py::test_window_close_rccl_two_ranks): both ranks hold the byte-wise maximum of the two shards' GLOBAL files and
    its estimate"""
    import subprocess
    import torch.multiprocessing as mp
    P = 8
    here = os.path.dirname(os.path.abspath(__file__))
    fake = os.path.join(here, "cpp", "fakerccl", "libfakerccl.so")
    if not os.path.exists(fake):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               os.path.join(here, "cpp", "fakerccl", "fakerccl.cc"), "-o", fake, "-L/opt/rocm/lib", "-lamdhip64", "-lrt",
                               "-Wl,-rpath,/opt/rocm/lib"])
    ctx = mp.get_context("spawn")
    q_uid, q_res = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_fake_rank, args=(r, q_uid, q_res)) for r in range(2)]
    old = os.environ.get("GYS_RCCL_LIB")
    os.environ["GYS_RCCL_LIB"] = fake
    try:
        for p in procs:
            p.start()
    finally:
        if old is None:
            del os.environ["GYS_RCCL_LIB"]
        else:
            os.environ["GYS_RCCL_LIB"] = old
    try:
        res = sorted(q_res.get(timeout=300) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", r[1]
    for p in procs:
        assert p.exitcode == 0
    assert res[0][6] > 0 and res[1][6] > 0 and res[0][6] + res[1][6] == NHOSTS
    loc = [np.frombuffer(res[r][2], dtype=np.uint8) for r in range(2)]
    assert loc[0].sum() > 0 and loc[1].sum() > 0 and (loc[0] != loc[1]).any()
    want = np.maximum(loc[0], loc[1])
    for r in range(2):
        assert res[r][5] >= 1, "the library's all-gather did not go through the stand-in"
        assert (np.frombuffer(res[r][3], dtype=np.uint8) == want).all(), f"rank {r}"
        assert _close(res[r][4], _oracle_est(oracle, want, P))
        assert res[r][7] == res[r][2]  # the rank's own registers are as they were
    assert np.float64(res[0][4]).tobytes() == np.float64(res[1][4]).tobytes()


def test_errors(torch_mod):
    """check 7: svc_hll_p = 0 -> GYS_ERR_STATE; null outputs, scope 3, n = 0, unknown glob_id -> GYS_ERR_INVAL with a message"""
    torch = torch_mod
    off = _engine(max_hosts=4, max_services=16, max_batch_events=1 << 14)
    mid = wire.machine_id(0)
    off.register_host(mid)
    off.register_listeners_np(mid, wire.glob_id(np.zeros(2, dtype=np.int64), np.arange(2)), wire.listener_netns(0, np.arange(2)), wire.listener_port(np.arange(2)))
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d, L = C.c_void_p(buf.data_ptr()), off.L
    out = C.c_double()
    assert L.gys_hll_file_bytes(off.h) == 0
    for rc in (L.gys_scan_distinct_dev(off.h, d), L.gys_query_distinct(off.h, int(wire.glob_id(0, 0)), C.byref(out)),
               L.gys_hll_rollup_dev(off.h, capi.ROLLUP_HOST, d, d), L.gys_hll_merge_files_dev(off.h, d, 1, d, d),
               L.gys_hll_global_rccl(off.h, d, d, d)):
        assert rc == capi.ERR_STATE and b"svc_hll_p" in L.gys_last_error()
    with pytest.raises(capi.GysError):
        off.scan_distinct()
    off.close()
    eng = _engine(max_hosts=4, max_services=16, max_batch_events=1 << 14, svc_hll_p=6)
    eng.register_host(mid)
    eng.register_listeners_np(mid, wire.glob_id(np.zeros(2, dtype=np.int64), np.arange(2)), wire.listener_netns(0, np.arange(2)), wire.listener_port(np.arange(2)))
    h = eng.h
    bad = [L.gys_scan_distinct_dev(h, None), L.gys_query_distinct(h, int(wire.glob_id(0, 0)), None), L.gys_query_distinct(h, 0x1234, C.byref(out)),
           L.gys_hll_rollup_dev(h, capi.ROLLUP_HOST, None, None), L.gys_hll_rollup_dev(h, 3, d, d), L.gys_hll_rollup_dev(h, -1, d, d),
           L.gys_hll_merge_files_dev(h, None, 1, d, d), L.gys_hll_merge_files_dev(h, d, 0, d, d), L.gys_hll_merge_files_dev(h, d, 1, None, None),
           L.gys_hll_global_rccl(h, None, d, d), L.gys_hll_global_rccl(h, d, None, None)]
    assert bad == [capi.ERR_INVAL] * len(bad), bad
    assert L.gys_query_distinct(h, 0x1234, C.byref(out)) == capi.ERR_INVAL and b"glob_id" in L.gys_last_error()
    assert L.gys_hll_rollup_dev(h, 3, d, d) == capi.ERR_INVAL and len(L.gys_last_error()) > 0
    assert L.gys_hll_merge_files_dev(h, d, 0, d, d) == capi.ERR_INVAL and len(L.gys_last_error()) > 0
    # and the good calls still work afterwards
    assert eng.query_distinct(int(wire.glob_id(0, 1))) == 0.0 and eng.scan_distinct().tolist() == [0.0, 0.0]
    eng.close()
