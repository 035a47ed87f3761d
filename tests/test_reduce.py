"""``storage.reduce``: the numpy restatement (CPU) and the reduction library against it (GPU).

The CPU part pins the restatement: the folds are exact and order-independent, the non-finite and
zero rules, both ends of the exponent range, integer wrap-around, signed-zero ordering, boxes.
The GPU part compares every device result bit for bit with the restatement on the same data
copied to the host, over the layouts, boxes, grid sizes and partitions the kernels take
different paths for.
"""

import math
from fractions import Fraction

import numpy as np
import pytest

import gt4py_amd  # noqa: F401
from gt4py_amd import storage
from gt4py_amd.storage import reduce as R

BE = "gt:mi355x"
DTYPES = [np.float64, np.float32, np.int32, np.int64]


def _wide(rng, shape, binades=30, dtype=np.float64):
    """Uniform mantissas over ``+-binades`` binades, some exact zeros of both signs."""
    n = int(np.prod(shape))
    x = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-binades, binades + 1, n))
    x[rng.integers(0, n, max(1, n // 50))] = 0.0
    x[rng.integers(0, n, max(1, n // 50))] = -0.0
    return x.astype(dtype).reshape(shape)


def _data(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return _wide(rng, shape, dtype=dtype)
    i = np.iinfo(dtype)
    return rng.integers(i.min, i.max, shape, dtype=dtype, endpoint=True)


def _bits(v):
    """A scalar result (numpy or 0-d tensor) as ``(dtype name, bit pattern)``; every NaN is one pattern."""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    assert v.shape == ()
    if v.dtype.kind == "f" and np.isnan(v):
        return (v.dtype.name, "nan")
    return (v.dtype.name, v.tobytes())


def _same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if isinstance(want, int) and not isinstance(want, np.generic):
        return int(got) == want
    return _bits(got) == _bits(want)


def _exact(values):
    return sum((Fraction(float(v)) for v in values), Fraction(0))


def _manual_folds(x, M, N):
    """The fold rule written out element by element: per fold the list of q's, and the last r's."""
    p = R.fold_plan(M, N)
    qs = [[], [], []]
    rs = []
    for v in x:
        r = float(v) * p.scale
        for f in range(3):
            q = r if p.ident[f] else (r + p.c[f]) - p.c[f]
            qs[f].append(q)
            r = r - q
        rs.append(r)
    return p, qs, rs


# ---------------------------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_fold_sums_are_exact_and_order_independent(n):
    rng = np.random.default_rng(100 + n)
    x = _wide(rng, (n,))
    M = np.abs(x).max()
    p, qs, rs = _manual_folds(x, M, n)
    S = R.fold_sums(x, M, n)
    for f in range(3):
        assert Fraction(float(S[f])) == _exact(qs[f]), f
        # every q of a fold is a multiple of the fold's grid
        grid = Fraction(2) ** (p.E[f] - 52)
        assert all((Fraction(q) / grid).denominator == 1 for q in qs[f])
    assert all(abs(Fraction(r)) <= Fraction(2) ** (p.E[2] - 53) for r in rs)
    assert _same(R.fold_sums(x[::-1], M, n), S)
    assert _same(R.fold_sums(x[rng.permutation(n)], M, n), S)
    parts = [R.fold_sums(c, M, n) for c in np.array_split(x, 13) if c.size]
    added = tuple(np.float64(math.fsum(float(c[f]) for c in parts)) for f in range(3))
    acc = [np.float64(0.0)] * 3
    for c in parts:  # plain f64 additions in strip order: exact as well
        acc = [a + c[f] for f, a in enumerate(acc)]
    assert _same(tuple(acc), S) and _same(added, S)


def test_cancellation():
    tiny = 3 * 2.0**-120
    for x, t in ((1.0, tiny), (1e16, 1.0), (-2.0**600, 2.0**460)):
        for order in ([x, -x, t], [t, x, -x], [x, t, -x]):
            got = R.sum(np.array(order))
            assert got.dtype == np.float64 and got == t, (order, got)
    assert (1e16 + 1.0) - 1e16 != 1.0  # what a plain sum in this order loses


def test_nonfinite_rules():
    nan, inf = np.nan, np.inf
    assert np.isnan(R.sum(np.array([1.0, nan, 2.0])))
    assert np.isnan(R.sum(np.array([inf, 1.0, -inf])))
    assert np.isnan(R.sum(np.array([inf, nan])))
    assert R.sum(np.array([1.0, inf, 2.0, inf])) == inf
    assert R.sum(np.array([-inf, 5.0])) == -inf
    assert np.isnan(R.dot(np.array([0.0, 1.0]), np.array([inf, 1.0])))  # 0 * inf
    assert R.dot(np.array([1e200, 1.0]), np.array([1e200, 1.0])) == inf  # a product overflows
    assert R.count_nonfinite(np.array([1.0, nan, inf, -inf, nan])) == 4
    assert R.count_nonfinite(np.arange(5, dtype=np.int32)) == 0
    sc = R.scan(np.array([nan, 3.0, inf, -inf, -7.0, nan]))
    assert _same(sc, (np.float64(inf), np.float64(-inf), np.float64(inf), np.int64(2), np.int64(1), np.int64(1), 6))
    # non-finite summands count as 0 in the folds
    assert _same(R.fold_sums(np.array([nan, 3.0, inf]), 4.0, 3), R.fold_sums(np.array([0.0, 3.0, 0.0]), 4.0, 3))
    assert _same(R.scan(np.array([nan, nan])), (np.float64(0.0), np.float64(inf), np.float64(-inf), np.int64(2),
                                                 np.int64(0), np.int64(0), 2))


def test_zero_maximum_gives_plus_zero():
    for x in ([0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0], [0.0, -0.0]):
        got = R.sum(np.array(x))
        assert got == 0 and not np.signbit(got), x
        assert _same(R.fold_sums(np.array(x), 0.0, len(x)), (np.float64(0.0),) * 3)
    assert R.sum(np.zeros((0, 3))) == 0 and R.sum(np.zeros((0, 3))).dtype == np.float64
    assert R.dot(np.zeros(0), np.zeros(0)) == 0
    assert R.sum(np.zeros(0, dtype=np.int32)) == 0 and R.sum(np.zeros(0, dtype=np.int32)).dtype == np.int64


def test_huge_maximum_edge():
    big = 1.7e308
    rng = np.random.default_rng(3)
    assert R.fold_plan(big, 2).scale == 2.0**-3 and R.fold_plan(big, 2).E[0] == 1022
    assert R.sum(np.array([big, 1.0e308])) == np.inf  # the sum itself overflows
    assert R.sum(np.array([-big, -1.0e308])) == -np.inf
    x = np.array([big, -1.0e308, 2.0**980, -big, 1.5e308, 2.0**-1074, -2.0**-1060])
    want = math.fsum(x)
    for _ in range(5):
        got = R.sum(x[rng.permutation(x.size)])
        assert got == want and np.isfinite(got)
    # E0 = 1023: the unscaled rule would round r + C up to 2^1024
    m = np.nextafter(2.0**1022, 0.0)
    assert R.sum(np.array([m, -(2.0**1000)])) == math.fsum([m, -(2.0**1000)])
    # the folds of the scaled summands are exact as well
    y = _wide(rng, (1000,), binades=10) * 2.0**1010
    p, qs, _ = _manual_folds(y, np.abs(y).max(), y.size)
    assert p.scale < 1.0
    S = R.fold_sums(y, np.abs(y).max(), y.size)
    assert all(Fraction(float(S[f])) == _exact(qs[f]) for f in range(3))
    assert _same(R.fold_sums(y[::-1], np.abs(y).max(), y.size), S)
    assert R.sum(y) == math.fsum(y)


def test_subnormal_edge():
    rng = np.random.default_rng(4)
    x = rng.integers(-(2**20), 2**20, 4097).astype(np.float64) * 2.0**-1074
    p = R.fold_plan(np.abs(x).max(), x.size)
    assert p.ident == (True, True, True)
    assert R.sum(x) == math.fsum(x) and R.sum(x[::-1]) == math.fsum(x)
    assert _same(R.fold_sums(x, np.abs(x).max(), x.size), R.fold_sums(x[rng.permutation(x.size)], np.abs(x).max(), x.size))
    # the first fold on a normal grid, the later ones below the smallest subnormal
    y = np.concatenate([x, rng.uniform(-1, 1, 100) * 2.0**-1000])
    p = R.fold_plan(np.abs(y).max(), y.size)
    assert p.ident == (False, True, True)
    assert R.sum(y) == math.fsum(y)
    assert _same(R.sum(y[::-1]), R.sum(y))
    xf = (rng.integers(-(2**10), 2**10, 300) * 2.0**-149).astype(np.float32)  # subnormal f32
    assert np.abs(xf).max() < np.finfo(np.float32).tiny and R.sum(xf) == math.fsum(xf.astype(np.float64))


def test_f32_in_f64_out():
    rng = np.random.default_rng(5)
    a, b = _wide(rng, (9, 11), dtype=np.float32), _wide(rng, (9, 11), dtype=np.float32)
    assert R.sum(a).dtype == np.float64 and _same(R.sum(a), R.sum(a.astype(np.float64)))
    assert _same(R.dot(a, b), R.sum(a.astype(np.float64) * b.astype(np.float64)))
    # an f32 product is exact in f64
    exact = sum(Fraction(float(u)) * Fraction(float(v)) for u, v in zip(a.ravel(), b.ravel()))
    p = R.fold_plan(R.scan(a, b)[0], a.size)
    assert abs(Fraction(float(R.dot(a, b))) - exact) <= a.size * Fraction(2) ** (p.E[2] - 52) + abs(exact) * Fraction(2) ** -52
    assert R.min(a).dtype == np.float32 and R.min(a) == a.min() and R.absmax(a) == np.abs(a).max()
    assert _same(R.norm2(a), np.sqrt(R.dot(a, a)))


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_integer_wrap_around(dtype):
    rng = np.random.default_rng(6)
    i = np.iinfo(dtype)
    x = rng.integers(i.max - 1000, i.max, (7, 33), dtype=dtype, endpoint=True)
    y = rng.integers(i.min, i.min + 1000, (7, 33), dtype=dtype)
    for v in (x, y, np.concatenate([x, y])):
        got = R.sum(v)
        assert got.dtype == np.int64 and got == np.sum(v, dtype=np.int64)
    with np.errstate(over="ignore"):
        want = np.sum(x.astype(np.int64) * y.astype(np.int64), dtype=np.int64)
    assert R.dot(x, y) == want
    assert R.min(y) == y.min() and R.min(y).dtype == dtype and R.max(x) == x.max()
    assert R.absmax(y).dtype == np.int64
    if dtype == np.int32:
        assert R.absmax(np.array([i.min, 5], dtype=dtype)) == 2**31  # computed in int64
    assert _same(R.fold_sums(x, 0, x.size), (np.sum(x, dtype=np.int64), np.int64(0), np.int64(0)))


def test_ordering_of_zeros_and_nan_propagation():
    for order in ([0.0, -0.0], [-0.0, 0.0], [-0.0, 0.0, -0.0, 0.0]):
        x = np.array(order)
        assert np.signbit(R.min(x)) and R.min(x) == 0
        assert not np.signbit(R.max(x)) and R.max(x) == 0
    assert np.signbit(R.max(np.array([-0.0, -1.0]))) and not np.signbit(R.min(np.array([0.0, 1.0])))
    x = np.array([3.0, np.nan, -1.0], dtype=np.float32)
    for fn in (R.min, R.max, R.absmax):
        assert np.isnan(fn(x)) and fn(x).dtype == np.float32
    assert R.absmax(np.array([-5.0, 3.0])) == 5.0


def test_boxes():
    rng = np.random.default_rng(7)
    full = np.full((9, 8, 5), np.nan)
    inner = _wide(rng, (6, 5, 5))
    full[2:8, 1:6, :] = inner
    kw = dict(origin=(2, 1, 0), domain=(6, 5, 5))
    assert _same(R.sum(full, **kw), R.sum(inner)) and np.isfinite(R.sum(full, **kw))
    assert _same(R.min(full, **kw), R.min(inner)) and _same(R.absmax(full, **kw), R.absmax(inner))
    assert R.count_nonfinite(full, **kw) == 0 and R.count_nonfinite(full) == full.size - inner.size
    assert _same(R.dot(full, full, **kw), R.dot(inner, inner))
    assert _same(R.sum(full, origin=(2, 1, 0), domain=(6, 5, 5)), R.sum(full[:8, :6], origin=(2, 1, 0)))
    # empty boxes
    assert R.sum(full, origin=(2, 1, 0), domain=(0, 5, 5)) == 0
    assert R.count_nonfinite(full, origin=(0, 0, 0), domain=(3, 0, 5)) == 0
    for fn in (R.min, R.max, R.absmax):
        with pytest.raises(ValueError):
            fn(full, origin=(2, 1, 0), domain=(0, 5, 5))
    with pytest.raises(ValueError, match="too large"):
        R.sum(full, origin=(2, 1, 0), domain=(8, 5, 5))
    with pytest.raises(ValueError, match="origin"):
        R.sum(full, origin=(2, 1))
    with pytest.raises(ValueError, match="Origin too small"):
        R.sum(full, origin=(-1, 0, 0))
    with pytest.raises(ValueError, match="domain"):
        R.sum(full, domain=(1, 1))
    with pytest.raises(ValueError, match="dtype"):
        R.sum(np.zeros(4, dtype=np.float16))
    with pytest.raises(ValueError, match="dtypes differ"):
        R.dot(np.zeros(4), np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError):
        R.sum(np.zeros((1,) * 9))
    # host storages and host tensors take the same path
    st = storage.from_array(inner, backend="numpy", aligned_index=(1, 1, 0))
    assert _same(R.sum(st), R.sum(inner))
    import torch

    assert _same(R.sum(torch.from_numpy(inner)), R.sum(inner))


@pytest.mark.parametrize("n", [7, 4097, 100003])
def test_accuracy_bound(n):
    """``|sum - fsum| <= N * 2**(E2 - 52)``; and the rule's own bound: the three exact fold sums
    miss the exact sum by the N remainders, at most ``2**(E2 - 53)`` each."""
    rng = np.random.default_rng(n)
    x = _wide(rng, (n,))
    p = R.fold_plan(np.abs(x).max(), n)
    S = R.fold_sums(x, np.abs(x).max(), n)
    exact = _exact(x)
    assert abs(_exact(S) - exact) <= n * Fraction(2) ** (p.E[2] - 53)
    got = R.sum(x)
    assert got == S[0] + (S[1] + S[2])
    assert abs(Fraction(float(got)) - Fraction(math.fsum(x))) <= n * Fraction(2) ** (p.E[2] - 52)


def test_plan_canonical_form():
    # an I-first storage box: rows along I, the padded J/K strides kept
    assert R.plan((65, 3, 67), (1, 72, 300)) == ((67, 3, 65), (300, 72, 1), (0, 0, 0), R.ROW)
    # ... and merged where the K stride continues the J rows
    assert R.plan((65, 3, 67), (1, 72, 216)) == ((201, 65), (72, 1), (0, 0), R.ROW)
    # dense C order merges into one row
    assert R.plan((4, 5, 6), (30, 6, 1)) == ((120,), (1,), (0,), R.ROW)
    assert R.plan((4, 5, 6), (30, 6, 1), (30, 6, 1)) == ((120,), (1,), (1,), R.ROW)
    # the second source keeps the dimensions apart
    assert R.plan((4, 6), (6, 1), (8, 1)) == ((4, 6), (6, 1), (8, 1), R.GENERIC)  # short rows
    assert R.plan((4, 64), (64, 1), (1, 4))[3] == R.GENERIC
    assert R.plan((40, 1, 1), (1, 40, 40)) == ((40,), (1,), (0,), R.ROW)
    assert R.plan((5, 64), (128, 2))[3] == R.GENERIC
    assert R.plan((1, 1), (1, 1)) == ((1,), (1,), (1,), R.GENERIC)
    assert R.plan((3, 0), (1, 1))[3] is None
    with pytest.raises(ValueError):
        R.plan((3, 4), (-4, 1))


# ---------------------------------------------------------------------------------------------
# GPU: the library against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------
def _device():
    import torch

    torch.empty(1, device="cuda")
    return torch


def _check_every_function(dev_a, dev_b, host_a, host_b, what, **kw):
    """Every public function on device views against the restatement on their host copies."""
    for fn in (R.sum, R.min, R.max, R.absmax, R.count_nonfinite, R.norm2):
        assert _same(fn(dev_a, **kw), fn(host_a, **kw)), (what, fn.__name__, kw)
    assert _same(R.dot(dev_a, dev_b, **kw), R.dot(host_a, host_b, **kw)), (what, "dot", kw)
    for args_d, args_h in (((dev_a,), (host_a,)), ((dev_a, dev_b), (host_a, host_b))):
        sc = R.scan(*args_h, **kw)
        assert _same(R.scan(*args_d, **kw), sc), (what, "scan", kw)
        assert _same(R.fold_sums(*args_d, sc[0], sc[6], **kw), R.fold_sums(*args_h, sc[0], sc[6], **kw)), (what, "folds", kw)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(65, 3, 67), (257, 33, 40)], ids=lambda s: "x".join(map(str, s)))
def test_storages_match_the_restatement(shape, dtype):
    _device()
    rng = np.random.default_rng(21)
    ha, hb = _data(rng, shape, dtype), _data(rng, shape, dtype)
    for ai in ((0, 0, 0), (1, 2, 0)):
        da = storage.from_array(ha, dtype, backend=BE, aligned_index=ai)
        db = storage.from_array(hb, dtype, backend=BE, aligned_index=ai)
        _check_every_function(da, db, ha, hb, ai)
        box = dict(origin=(1, 2, 0), domain=(shape[0] - 2, shape[1] - 2, shape[2]))
        _check_every_function(da, db, ha, hb, ai, **box)
    # two sources whose rows start at different 16-B phases: one element per lane
    db = storage.from_array(hb, dtype, backend=BE, aligned_index=(0, 0, 0))
    assert _same(R.dot(da, db), R.dot(ha, hb))
    assert _same(R.dot(da, db, origin=(3, 0, 0)), R.dot(ha, hb, origin=(3, 0, 0)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32], ids=lambda d: np.dtype(d).name)
def test_masks_data_dimensions_and_generic_views(dtype):
    torch = _device()
    rng = np.random.default_rng(22)
    for shape, dims in (((65, 20), "IJ"), ((20, 33), "IK"), ((40,), "K"), ((5, 6, 7, 2, 3), None)):
        ha, hb = _data(rng, shape, dtype), _data(rng, shape, dtype)
        if dims is None:  # data dimensions
            da = storage.from_array(ha, np.dtype((dtype, (2, 3))), backend=BE)
            db = storage.from_array(hb, np.dtype((dtype, (2, 3))), backend=BE)
        else:
            da = storage.from_array(ha, dtype, backend=BE, dimensions=tuple(dims))
            db = storage.from_array(hb, dtype, backend=BE, dimensions=tuple(dims))
        _check_every_function(da, db, ha, hb, shape)
        if len(shape) == 2:
            _check_every_function(da, db, ha, hb, shape, origin=(1, 2), domain=(shape[0] - 2, shape[1] - 3))
    # a view with innermost stride 2 (not a storage): the generic path
    h = _data(rng, (9, 70, 6), dtype)
    wide = torch.from_numpy(h).cuda()
    va, ha = wide[:, ::2, 1], np.ascontiguousarray(h[:, ::2, 1])
    assert R.plan(va.shape, va.stride())[3] == R.GENERIC
    _check_every_function(va, va, ha, ha, "stride 2")
    # a broadcast (stride 0) second source and a C-order tensor
    hb = _data(rng, (9, 1, 6), dtype)
    vb = torch.from_numpy(hb).cuda().expand(9, 70, 6)
    assert _same(R.dot(wide, vb), R.dot(h, np.broadcast_to(hb, h.shape)))
    _check_every_function(wide, wide, h, h, "c order")

    class Foreign:  # any object with __cuda_array_interface__ takes the device path
        __cuda_array_interface__ = wide.__cuda_array_interface__

    got = R.sum(Foreign())
    assert got.is_cuda and _same(got, R.sum(h))


@pytest.mark.gpu
def test_geometry_and_partition_independence():
    torch = _device()
    rng = np.random.default_rng(23)
    shape = (257, 33, 40)
    for dtype in (np.float64, np.float32):
        ha, hb = _data(rng, shape, dtype), _data(rng, shape, dtype)
        da = storage.from_array(ha, dtype, backend=BE, aligned_index=(3, 3, 0))
        db = storage.from_array(hb, dtype, backend=BE, aligned_index=(3, 3, 0))
        want_sum, want_dot = R.sum(ha), R.dot(ha, hb)
        for blocks in (1, 7, None):
            assert _same(R.sum(da, _blocks=blocks), want_sum), blocks
            assert _same(R.dot(da, db, _blocks=blocks), want_dot), blocks
            assert _same(R.sum(da, origin=(1, 2, 0), _blocks=blocks), R.sum(ha, origin=(1, 2, 0))), blocks
            assert _same(R.scan(da, _blocks=blocks), R.scan(ha)), blocks
        # three uneven J strips against the whole domain's (M, N): the distributed path in one process
        sc = R.scan(da)
        whole = R.fold_sums(da, sc[0], sc[6])
        assert _same(whole, R.fold_sums(ha, R.scan(ha)[0], ha.size))
        acc = None
        raws = []
        for j0, j1 in ((0, 5), (5, 19), (19, 33)):
            box = dict(origin=(0, j0, 0), domain=(shape[0], j1 - j0, shape[2]))
            part = R.fold_sums(da, sc[0], sc[6], **box)  # M stays on the device
            assert _same(part, R.fold_sums(ha, R.scan(ha)[0], ha.size, **box))
            acc = part if acc is None else tuple(a + p for a, p in zip(acc, part))
            p = R._DevicePass(R._box(da, box["origin"], box["domain"]), None, np.dtype(dtype), None, None)
            raws.append(p.scan())
        assert _same(acc, whole)
        # the strips' scans combined are the whole domain's scan
        p = R._DevicePass(da, None, np.dtype(dtype), None, None)
        combined = R.combine_scans_device(torch.stack(raws), dtype)
        assert torch.equal(combined, p.scan())


@pytest.mark.gpu
def test_special_values():
    _device()
    rng = np.random.default_rng(24)
    shape = (65, 3, 67)
    base = _wide(rng, shape)
    nan, inf = np.nan, np.inf
    cases = {"wide": {}, "nan": {(5, 1, 7): nan}, "pinf": {(64, 2, 66): inf}, "ninf": {(0, 0, 0): -inf},
             "all": {(5, 1, 7): nan, (64, 2, 66): inf, (0, 0, 0): -inf, (1, 1, 1): inf}}
    for name, cells in cases.items():
        for dtype in (np.float64, np.float32):
            h = base.astype(dtype)
            for idx, v in cells.items():
                h[idx] = v
            d = storage.from_array(h, dtype, backend=BE, aligned_index=(1, 1, 0))
            _check_every_function(d, d, h, h, name)
    # a NaN that lies only in the halo does not show
    h = np.full((71, 9, 67), np.nan)
    h[3:68, 3:6, :] = base
    d = storage.from_array(h, backend=BE, aligned_index=(3, 3, 0))
    kw = dict(origin=(3, 3, 0), domain=shape)
    assert _same(R.sum(d, **kw), R.sum(base)) and _same(R.absmax(d, **kw), R.absmax(base))
    assert int(R.count_nonfinite(d, **kw)) == 0 and _same(R.min(d, **kw), R.min(base))
    assert _same(R.dot(d, d, **kw), R.dot(base, base))
    # subnormal inputs are not flushed
    sub64 = rng.integers(-(2**20), 2**20, shape).astype(np.float64) * 2.0**-1074
    sub32 = (rng.integers(-(2**10), 2**10, shape) * 2.0**-149).astype(np.float32)
    mixed = np.where(rng.random(shape) < 0.1, base * 2.0**-990, sub64)
    for h in (sub64, sub32, mixed):
        d = storage.from_array(h, h.dtype, backend=BE)
        assert float(R.sum(h)) != 0.0
        _check_every_function(d, d, h, h, "subnormal")
    # the huge-M edge (dot: the products overflow)
    huge = base * 2.0**990
    d = storage.from_array(huge, backend=BE)
    assert R.fold_plan(np.abs(huge).max(), huge.size).scale < 1.0 and np.isfinite(R.sum(huge))
    _check_every_function(d, d, huge, huge, "huge")
    # all zeros, of both signs
    z = np.where(rng.random(shape) < 0.5, 0.0, -0.0)
    d = storage.from_array(z, backend=BE)
    _check_every_function(d, d, z, z, "zeros")


@pytest.mark.gpu
def test_identities_shapes_and_streams():
    torch = _device()
    rng = np.random.default_rng(25)
    h = _wide(rng, (65, 3, 67))
    d = storage.from_array(h, backend=BE, aligned_index=(1, 1, 0))
    n2, dd = R.norm2(d), R.dot(d, d)
    assert n2.is_cuda and n2.dim() == 0 and n2.dtype == torch.float64
    assert float(n2) == math.sqrt(float(dd))
    # a one-cell box and an empty one
    one = dict(origin=(7, 1, 13), domain=(1, 1, 1))
    for fn in (R.sum, R.min, R.max):
        assert float(fn(d, **one)) == h[7, 1, 13]
    assert float(R.absmax(d, **one)) == abs(h[7, 1, 13]) and _same(R.norm2(d, **one), R.norm2(h, **one))
    empty = dict(origin=(7, 1, 13), domain=(0, 2, 5))
    for fn in (R.sum, R.count_nonfinite):
        got = fn(d, **empty)
        assert got.is_cuda and _same(got, fn(h, **empty))
    assert _same(R.dot(d, d, **empty), R.dot(h, h, **empty))
    for fn in (R.min, R.max, R.absmax):
        with pytest.raises(ValueError):
            fn(d, **empty)
    with pytest.raises(ValueError, match="dtype"):
        R.sum(d.to(torch.float16))
    # results stay on the device, in the documented types
    for fn, dt in ((R.sum, torch.float64), (R.min, torch.float64), (R.count_nonfinite, torch.int64)):
        got = fn(d)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dim() == 0 and got.dtype == dt
    d32 = storage.from_array(h.astype(np.float32), np.float32, backend=BE)
    assert R.max(d32).dtype == torch.float32 and R.sum(d32).dtype == torch.float64
    di = storage.from_array(np.arange(-50, 50, dtype=np.int32).reshape(10, 10), np.int32, backend=BE, dimensions=("I", "J"))
    assert R.min(di).dtype == torch.int32 and R.absmax(di).dtype == torch.int64 and R.sum(di).dtype == torch.int64
    # a side stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = R.sum(d, stream=s)
    got_dot = R.dot(d, d, origin=(1, 1, 0), stream=s)
    s.synchronize()
    assert _same(got, R.sum(h)) and _same(got_dot, R.dot(h, h, origin=(1, 1, 0)))


@pytest.mark.gpu
def test_no_host_synchronisation(monkeypatch):
    torch = _device()
    h = _wide(np.random.default_rng(26), (65, 3, 67))
    d = storage.from_array(h, backend=BE)
    R.sum(d)  # library loaded

    def no_sync(*a, **k):
        raise AssertionError("device->host transfer or synchronisation in a reduction")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, no_sync)
        m.setattr(torch.cuda, "synchronize", no_sync)
        results = [R.sum(d), R.dot(d, d), R.absmax(d), R.count_nonfinite(d, origin=(1, 1, 1)), R.norm2(d)]
        sc = R.scan(d)
        results += list(R.fold_sums(d, sc[0], sc[6]))
    assert _same(results[0], R.sum(h)) and _same(results[5], R.fold_sums(h, R.scan(h)[0], h.size)[0])


@pytest.mark.gpu
def test_library_reports_its_abi_version():
    _device()
    assert R.abi_version() == 1
    # planner and library agree on the path
    import ctypes

    for shape, sa, sb in (((65, 3, 67), (1, 72, 216), None), ((5, 64), (128, 2), None), ((4, 64), (64, 1), (1, 4)),
                          ((4, 6), (6, 1), (8, 1)), ((40,), (1,), None)):
        extent, a, b, path = R.plan(shape, sa, sb)
        desc = R.GtmiReduceDesc()
        desc.a, desc.b = 64, (64 if sb is not None else None)
        desc.extent[: len(extent)], desc.a_stride[: len(extent)], desc.b_stride[: len(extent)] = extent, a, b
        desc.ndim, desc.dtype = len(extent), 1
        assert R._PATH_CODES[R._library().gtmi_reduce_path(ctypes.byref(desc))] == path


@pytest.mark.gpu
def test_global_reductions_on_device_tensors_over_rccl():
    """The device path of ``distributed.reduce`` (gather, record kernel, all-reduce of the folds)
    in a world of one rank: the bits of ``storage.reduce`` and of the restatement."""
    import socket

    torch = _device()
    import torch.distributed as dist

    from gt4py_amd.distributed import reduce as G
    from gt4py_amd.distributed.halo import rccl_options

    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0), pg_options=rccl_options())
    try:
        rng = np.random.default_rng(27)
        box = dict(origin=(1, 2, 0), domain=(63, 1, 67))
        for dtype in (np.float64, np.float32, np.int64):
            ha, hb = _data(rng, (65, 3, 67), dtype), _data(rng, (65, 3, 67), dtype)
            if np.dtype(dtype).kind == "f":
                ha[0, 0, 0] = np.nan  # outside the box below
            da = storage.from_array(ha, dtype, backend=BE, aligned_index=(1, 2, 0))
            db = storage.from_array(hb, dtype, backend=BE, aligned_index=(1, 2, 0))
            for kw in (box, dict(box, global_count=63 * 67)):
                local = {k: v for k, v in kw.items() if k != "global_count"}
                got = G.global_sum(da, **kw)
                assert got.is_cuda and _same(got, R.sum(ha, **local)) and _same(got, R.sum(da, **local))
                assert _same(G.global_dot(da, db, **kw), R.dot(ha, hb, **local))
                assert _same(G.global_norm2(da, **kw), R.norm2(ha, **local))
                assert _same(G.global_min(da, **kw), R.min(ha, **local))
                assert _same(G.global_max(da, **kw), R.max(ha, **local))
                assert _same(G.global_absmax(da, **kw), R.absmax(ha, **local))
                assert _same(G.global_count_nonfinite(da, **kw), R.count_nonfinite(ha, **local))
            if np.dtype(dtype).kind == "f":
                assert np.isnan(float(G.global_sum(da))) and int(G.global_count_nonfinite(da)) == 1
            # a rank whose part is empty contributes the identities
            none = dict(origin=(1, 2, 0), domain=(63, 0, 67))
            assert float(G.global_sum(da, **none)) == 0 and int(G.global_count_nonfinite(da, **none)) == 0
            with pytest.raises(ValueError):
                G.global_min(da, **none)
    finally:
        dist.destroy_process_group()
