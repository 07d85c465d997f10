"""gys_topk_dev on the device: the exact top-k of a column of doubles ("Top-k" in include/gysketch.h; kernels k_topk_keys, k_topk_ties, k_topk_gather in
gyeeta_amd/csrc/gys_topk.hpp with the selection rounds of gys_svcquery.hpp).  Every answer is compared BIT FOR BIT with the definition restated in
numpy: np.lexsort on (row, value with + 0.0 applied so that -0.0 ties +0.0) over the eligible rows.  No tolerances.
  sizes    1, 2, 255, 256, 257, 1 023, 1 025, 4 095, 4 096, 4 097 and one that no single launch of k_topk_keys covers without grid-striding (a
           workgroup takes a tile of 1 024 rows, at most four workgroups per CU are launched: CUs * 4 * 1 024 + 4 097 rows)
  k        0, 1, nrows - 1, nrows, nrows + 3; both orders
  columns  distinct normal doubles; all rows equal (the answer is rows 0 .. k - 1); two values with the cut inside the lower value's ties;
           1.0 + i 2^-52, i < 512 (they differ in the last selection round's nine bits only); +-0.0, +-inf, denormals, negatives and NaNs (NaNs
           never appear and are not counted); the integers 0 .. 49
  and      a stride of 3; a shuffled 60 % subset of the rows against the same subset sorted; weights with a threshold that removes about half the
           rows; k above the eligible count; the GYS_ERR_INVAL cases."""
import ctypes as C

import numpy as np
import pytest

from gyeeta_amd import capi

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 255, 256, 257, 1023, 1025, 4095, 4096, 4097]
COLUMNS = ["distinct", "equal", "two-values", "last-nine-bits", "specials", "ints-0-49"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    from gyeeta_amd.engine import SketchEngine
    e = SketchEngine(max_hosts=2, max_services=8, max_batch_events=1 << 12)
    yield e
    e.close()


def striding_size(eng):
    """rows that k_topk_keys cannot cover without grid-striding: it launches min(tiles of 1 024 rows, 4 per CU) workgroups (topk_keys_grid)"""
    cus = eng.torch.cuda.get_device_properties(eng.device).multi_processor_count
    return cus * 4 * 1024 + 4097


def make_col(rng, kind, n):
    perm = rng.permutation(n)
    if kind == "distinct":
        return (perm.astype(np.float64) - n // 2) * 1.25 + 0.125
    if kind == "equal":
        return np.full(n, 42.5)
    if kind == "two-values":
        return np.where(perm % 3 == 0, 7.0, 3.0)
    if kind == "last-nine-bits":
        return (np.float64(1.0).view(np.uint64) + (perm % 512).astype(np.uint64)).view(np.float64)
    if kind == "specials":
        den = np.float64(5e-324)
        sp = np.array([0.0, -0.0, np.inf, -np.inf, den, -den, 4 * den, -1.5, 1.5, -1e300, 1e300, np.nan, -np.nan, 0.0, -0.0, 2.0])
        return sp[rng.integers(0, 16, n)]
    return rng.integers(0, 50, n).astype(np.float64)


def restated(col, cand, weight, min_weight, order):
    """the definition: all eligible rows of `cand` in their total order"""
    rows = np.sort(np.asarray(cand, dtype=np.int64))
    v = col[rows]
    ok = ~np.isnan(v)
    if weight is not None:
        ok &= weight[rows] >= min_weight
    rows, v = rows[ok], v[ok] + 0.0
    return rows[np.lexsort((rows, -v if order == capi.TOPK_LARGEST else v))]


def check(got, nel, want_rows, k, colvals, weight, what):
    want = want_rows[:k]
    assert nel == len(want_rows), (what, nel, len(want_rows))
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got["row"] != want)
    assert not len(bad), (what, "entry %d is row %d, want %d" % (bad[0], got["row"][bad[0]], want[bad[0]]))
    assert (got["value"].view(np.uint64) == colvals[want].view(np.uint64)).all(), (what, "the values are not the column's stored bits")
    assert (got["weight"] == (weight[want] if weight is not None else 0)).all() and not got["reserved"].any(), what


def run_table(eng, rng, n, kind):
    torch = eng.torch
    col = make_col(rng, kind, n)
    d_col = torch.from_numpy(col).to(eng.device)
    ks = [0, 1, n - 1, n, n + 3]
    if kind == "two-values":
        n7 = int((col == 7.0).sum())
        ks.append(n7 + (n - n7) // 2)  # LARGEST: inside the run of the lower value; SMALLEST: inside a run as well (both values repeat)
    for order in (capi.TOPK_LARGEST, capi.TOPK_SMALLEST):
        want = restated(col, np.arange(n), None, 0, order)
        if kind == "equal":
            assert (want == np.arange(n)).all()
        if kind == "specials":
            assert len(want) == n - int(np.isnan(col).sum())
        for k in ks:
            got, nel = eng.topk(d_col, k, order=order)
            check(got, nel, want, k, col, None, (kind, n, k, order))


@pytest.mark.parametrize("kind", COLUMNS)
@pytest.mark.parametrize("n", SMALL)
def test_topk_equals_the_definition(eng, n, kind):
    run_table(eng, np.random.default_rng(SMALL.index(n) * 10 + COLUMNS.index(kind)), n, kind)


@pytest.mark.parametrize("kind", COLUMNS)
def test_topk_at_a_size_that_needs_grid_striding(eng, kind):
    n = striding_size(eng)
    assert n > eng.torch.cuda.get_device_properties(eng.device).multi_processor_count * 4 * 1024
    run_table(eng, np.random.default_rng(77 + COLUMNS.index(kind)), n, kind)


@pytest.mark.parametrize("n", [257, 4097])
def test_stride_rows_and_weights(eng, n):
    torch = eng.torch
    rng = np.random.default_rng(n)
    arr = (rng.integers(0, 97, (n, 3)) - 48).astype(np.float64)
    arr[rng.integers(0, n, 5), 1] = np.nan
    d_arr = torch.from_numpy(arr).to(eng.device)
    col = arr[:, 1].copy()
    sub = np.flatnonzero(rng.random(n) < 0.6)
    shuf = rng.permutation(sub)
    assert (shuf != sub).any()
    weight = rng.integers(0, 1000, n).astype(np.uint64)
    d_w = torch.from_numpy(weight.view(np.int64)).to(eng.device)
    d_sub, d_shuf = (torch.from_numpy(x.astype(np.int32)).to(eng.device) for x in (sub, shuf))
    d_col1 = d_arr.reshape(-1)[1:]  # column 1 of the n x 3 array: row r at r * 3
    for order in (capi.TOPK_LARGEST, capi.TOPK_SMALLEST):
        for k in (1, 33, len(sub) - 1, n + 3):
            what = (n, order, k)
            got, nel = eng.topk(d_col1, k, order=order, stride=3, nrows=n)
            check(got, nel, restated(col, np.arange(n), None, 0, order), k, col, None, ("stride 3",) + what)
            want = restated(col, sub, None, 0, order)
            a, nela = eng.topk(d_col1, k, order=order, stride=3, rows=d_shuf)
            b, nelb = eng.topk(d_col1, k, order=order, stride=3, rows=d_sub)
            assert a.tobytes() == b.tobytes() and nela == nelb, ("the order of d_rows changed the answer",) + what
            check(a, nela, want, k, col, None, ("shuffled subset",) + what)
            want = restated(col, np.arange(n), weight, 500, order)
            assert 0.3 * n < len(want) < 0.7 * n  # (the threshold removes about half the rows)
            got, nel = eng.topk(d_col1, k, order=order, stride=3, nrows=n, weight=d_w, min_weight=500)
            check(got, nel, want, k, col, weight, ("weights",) + what)
            got, nel = eng.topk(d_col1, k, order=order, stride=3, rows=d_shuf, weight=d_w, min_weight=500)
            check(got, nel, restated(col, sub, weight, 500, order), k, col, weight, ("weights on a subset",) + what)
    # k above the eligible count: everything eligible, in order; a threshold nothing reaches: nothing
    got, nel = eng.topk(d_col1, n, stride=3, nrows=n, weight=d_w, min_weight=500)
    assert len(got) == nel == len(restated(col, np.arange(n), weight, 500, 0)) < n
    got, nel = eng.topk(d_col1, 5, stride=3, nrows=n, weight=d_w, min_weight=1000)
    assert len(got) == 0 and nel == 0
    got, nel = eng.topk(d_col1, 5, stride=3, nrows=0)
    assert len(got) == 0 and nel == 0


def test_error_codes(eng):
    torch = eng.torch
    d_col = torch.arange(16, dtype=torch.float64, device=eng.device)
    out = (capi.TopkEntry * 4)()
    nout, nel = C.c_uint32(), C.c_uint64()
    col = C.c_void_p(d_col.data_ptr())
    L, h = eng.L, eng.h
    eng.sync()
    assert L.gys_topk_dev(h, None, 1, 16, None, None, 0, 0, 4, out, C.byref(nout), C.byref(nel)) == capi.ERR_INVAL  # no column
    assert L.gys_topk_dev(h, col, 0, 16, None, None, 0, 0, 4, out, C.byref(nout), C.byref(nel)) == capi.ERR_INVAL  # stride 0
    assert L.gys_topk_dev(h, col, 1, 16, None, None, 0, 2, 4, out, C.byref(nout), C.byref(nel)) == capi.ERR_INVAL  # unknown order
    assert L.gys_topk_dev(h, col, 1, 16, None, None, 0, -1, 4, out, C.byref(nout), C.byref(nel)) == capi.ERR_INVAL
    assert L.gys_topk_dev(h, col, 1, 16, None, None, 0, 0, 4, None, C.byref(nout), C.byref(nel)) == capi.ERR_INVAL  # k > 0 without out
    # k == 0 needs no out and still counts; neligible may be NULL
    assert L.gys_topk_dev(h, col, 1, 16, None, None, 0, 0, 0, None, C.byref(nout), C.byref(nel)) == capi.OK and nout.value == 0 and nel.value == 16
    assert L.gys_topk_dev(h, col, 1, 16, None, None, 0, 1, 4, out, C.byref(nout), None) == capi.OK and [out[i].row for i in range(nout.value)] == [0, 1, 2, 3]
