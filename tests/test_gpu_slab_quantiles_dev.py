"""gys_tdigest_slab_quantiles_dev: the quantiles of any number of device slabs in one launch (kernel k_td_slab_quantiles in
gyeeta_amd/csrc/gys_tdrank.hpp).  Every entry is compared BIT FOR BIT with the existing one-slab host call gys_tdigest_slab_quantiles on that
slab.  No tolerances.
  1. hand-built slabs uploaded from numpy, 1, 3, 4, 5 and 257 of them with 1, 3 and 16 quantiles: an empty slab, one cluster, only cluster 199
     non-empty, gaps, equal neighbouring means, counts above 2^32 (the weight below 2^53), q = -0.5, 0, 1, 1.5 and a q whose target weight
     falls exactly on a cluster centre;
  2. the HOST / CLUSTER / GLOBAL roll-ups and the filtered rows of a small engine (6 hosts x 4 services, td_pend_cap 64, a few thousand events:
     merges and buffered values both occur);
  3. the error codes; nothing is written for 0 slabs."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi
from tests.test_gpu_td_ranks import H, S, World, latencies, torch_mod  # noqa: F401 (torch_mod is a fixture)

pytestmark = pytest.mark.gpu

NB = capi.TD_NB
STYLES = ["empty", "one", "only-199", "all", "equal-means", "gaps", "row-borders", "wide", "centres"]


def make_slab(rng, style, SLAB_DT):
    arr = np.zeros(1, dtype=SLAB_DT)
    cnt, sm = arr["cnt"][0], arr["sum"][0]  # (views)
    if style == "centres":  # N = 16: the centres 2, 8 and 14 are q = 0.125, 0.5 and 0.875 exactly
        cnt[[10, 70, 130]] = [4, 8, 4]
        sm[[10, 70, 130]] = [4 * 100 + 1, 8 * 250 + 3, 4 * 900]
        arr["vmin"][0], arr["vmax"][0] = 90, 950
        return arr[0]
    idx = {"empty": [], "one": [int(rng.integers(0, NB))], "only-199": [199], "all": list(range(NB)), "equal-means": list(range(NB)),
           "gaps": [k for k in range(NB) if rng.random() < 0.33] or [5], "row-borders": [63, 64, 127, 128, 191, 192, 199], "wide": list(range(0, NB, 2))}[style]
    if not idx:
        arr["vmin"][0], arr["vmax"][0] = 12345, -7  # (an empty slab's extremes are not valid and must not show)
        return arr[0]
    b = int(rng.integers(0, 5000))
    for i, k in enumerate(idx):
        cn = (1 << 32) + int(rng.integers(0, 1 << 34)) if style == "wide" and i % 3 == 1 else 1 + int(rng.integers(0, 3 if i % 5 == 0 else 5000))
        rem = 0 if style == "equal-means" else int(rng.integers(0, cn))
        if style != "equal-means" or i % 3 == 0:
            b += int(rng.integers(0, 900)) + 1
        cnt[k], sm[k] = cn, b * cn + rem
        if i == 0:
            arr["vmin"][0] = b - int(rng.integers(0, 40))
        arr["vmax"][0] = b + 1 + int(rng.integers(0, 40))
        b += 1 if rem else 0
    assert int(cnt.sum()) < 1 << 53
    return arr[0]


QS = [0.5, -0.5, 0.0, 1.0, 1.5, 0.125, 0.875, 0.99, 0.25, 1e-9, 1.0 - 1e-12, 0.95, 0.75, 0.001, 0.999999, 0.1]


def upload(eng, slabs):
    return eng.torch.from_numpy(np.frombuffer(slabs.tobytes(), dtype=np.uint8).copy()).to(eng.device)


def compare(eng, dev, n, qs, what):
    d_out, got = eng.slab_quantiles_dev(dev, n, qs)
    assert got.shape == (n, len(qs))
    for i in range(n):
        want = np.array(eng.slab_quantiles(dev, qs, index=i), dtype=np.float64)
        assert got[i].tobytes() == want.tobytes(), (what, "slab %d" % i, qs, got[i].tolist(), want.tolist())
    return got


@pytest.mark.parametrize("nq", [1, 3, 16])
@pytest.mark.parametrize("nslabs", [1, 3, 4, 5, 257])
def test_hand_built_slabs(torch_mod, nslabs, nq):
    from gyeeta_amd.engine import SketchEngine
    rng = np.random.default_rng(nslabs * 100 + nq)
    eng = SketchEngine(max_hosts=2, max_services=8, max_batch_events=1 << 12)
    first = {1: {1: "centres", 3: "empty", 16: "wide"}[nq]}.get(nslabs)
    styles = [first or STYLES[(i + nq) % len(STYLES)] for i in range(nslabs)]
    slabs = np.array([make_slab(rng, st, eng.SLAB_DT) for st in styles], dtype=eng.SLAB_DT)
    dev = upload(eng, slabs)
    qs = QS[:nq] if nq > 1 else [[0.5, -0.5, 0.0, 1.0, 1.5][nslabs % 5]]
    got = compare(eng, dev, nslabs, qs, (nslabs, nq))
    for i, st in enumerate(styles):
        if st == "empty":
            assert not got[i].any()
        if st == "centres":
            c = slabs[i]
            for q, centre in ((0.125, 2.0), (0.5, 8.0), (0.875, 14.0)):
                assert q * float(c["cnt"].sum()) == centre  # the target weight is the centre itself
            assert compare(eng, dev[i * slabs.itemsize:], 1, [0.125, 0.5, 0.875], "centres").tolist() == [[100.0, 250.0, 900.0]]
    if nslabs == 257:
        assert set(styles) == set(STYLES)
        for qs in ([0.125, 0.5, 0.875], [-0.5], [1.5, 0.0, 1.0, 2.0 ** -60]):
            compare(eng, dev, nslabs, qs, "every style")
    eng.close()


def test_rollups_and_filtered_rows_of_an_engine(torch_mod):
    rng = np.random.default_rng(4242)
    w = World(64)
    eng = w.eng
    lat = latencies(rng, "lognormal")
    for rnd in range(3):
        w.counts(rng, rng.integers(0, 400, H * S), lat)
    w.counts(rng, rng.integers(1, 30, H * S), lat)
    npend, _ = eng.export_tdigest_pending()
    _, cnts, _ = eng.export_tdigest()
    assert int(cnts.sum()) > 0 and int(npend.max()) > 0  # (merges have happened and buffers hold values)
    scopes = [("host", H, eng.tdigest_rollup(capi.ROLLUP_HOST)[0]), ("cluster", 3, eng.tdigest_rollup(capi.ROLLUP_CLUSTER)[0]),
              ("global", 1, eng.tdigest_rollup(capi.ROLLUP_GLOBAL)[0])]
    rows, nrows, out = eng.rollup_filtered(capi.GROUP_CLUSTER, any_state=True, want=("slabs",))
    assert nrows == 3
    scopes.append(("filtered by cluster", 3, out["slabs_dev"]))
    rows, nrows, out = eng.rollup_filtered(capi.GROUP_HOST, any_state=True, want=("slabs",), machine_ids=[w.info[1][0], w.info[4][0]])
    assert nrows == 2
    scopes.append(("filtered hosts", 2, out["slabs_dev"]))
    for name, n, dev in scopes:
        for qs in (QS, [0.99], [0.25, 0.5, 0.95]):
            got = compare(eng, dev, n, qs, name)
            assert got[:, qs.index(0.99) if 0.99 in qs else 1].min() > 0  # (every group has data)
    eng.close()


def test_error_codes_and_no_slabs(torch_mod):
    from gyeeta_amd.engine import SketchEngine
    eng = SketchEngine(max_hosts=2, max_services=8, max_batch_events=1 << 12)
    dev = upload(eng, np.zeros(2, dtype=eng.SLAB_DT))
    out = eng.torch.full((4,), 7.0, dtype=eng.torch.float64, device=eng.device)
    q = (C.c_double * 17)(*([0.5] * 17))
    L, h, vp = eng.L, eng.h, C.c_void_p
    eng.torch.cuda.synchronize()
    assert L.gys_tdigest_slab_quantiles_dev(h, None, 2, q, 1, vp(out.data_ptr())) == capi.ERR_INVAL
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 2, None, 1, vp(out.data_ptr())) == capi.ERR_INVAL
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 2, q, 1, None) == capi.ERR_INVAL
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 2, q, 0, vp(out.data_ptr())) == capi.ERR_INVAL
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 2, q, 17, vp(out.data_ptr())) == capi.ERR_INVAL
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 0, q, 2, vp(out.data_ptr())) == capi.OK
    eng.sync()
    assert out.cpu().tolist() == [7.0] * 4  # nothing was written
    assert L.gys_tdigest_slab_quantiles_dev(h, vp(dev.data_ptr()), 2, q, 2, vp(out.data_ptr())) == capi.OK
    eng.sync()
    assert out.cpu().tolist() == [0.0] * 4  # empty slabs
    eng.close()
