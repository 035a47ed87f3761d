"""``storage.reduce`` with ``axis=``: the vectorised restatement against the scalar functions on
every kept cell's sub-box (CPU), and the axis reduction library against the restatement (GPU).
Every comparison is bitwise (all NaNs count as one value).
"""

import itertools
import math

import numpy as np
import pytest

import gt4py_amd  # noqa: F401
from gt4py_amd import storage
from gt4py_amd.storage import reduce as R
from gt4py_amd.storage import reduce_axis as RA

BE = "gt:mi355x"
DTYPES = [np.float64, np.float32, np.int32, np.int64]
FUNCTIONS = ("sum", "min", "max", "absmax", "count_nonfinite", "norm2", "dot")


def _wide(rng, shape, binades=30, dtype=np.float64):
    n = int(np.prod(shape))
    x = rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-binades, binades + 1, n))
    x[rng.integers(0, n, max(1, n // 50))] = 0.0
    x[rng.integers(0, n, max(1, n // 50))] = -0.0
    return x.astype(dtype).reshape(shape)


def _data(rng, shape, dtype, special=False):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        x = _wide(rng, shape, dtype=dtype)
        if special:  # a few non-finite cells: some sub-boxes get them, most do not
            flat = x.reshape(-1)
            for v in (np.nan, np.inf, -np.inf, np.inf):
                flat[rng.integers(0, flat.size)] = v
        return x
    i = np.iinfo(dtype)
    return rng.integers(i.min, i.max, shape, dtype=dtype, endpoint=True)


def _np(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def _same(got, want):
    """Same shape, dtype and bits; every NaN is one value. Tuples element-wise, Python ints by value."""
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if isinstance(want, int) and not isinstance(want, np.generic):
        return int(got) == want
    g, w = _np(got), _np(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    if g.dtype.kind == "f":
        nan_g, nan_w = np.isnan(g), np.isnan(w)
        if not np.array_equal(nan_g, nan_w):
            return False
        g, w = np.where(nan_g, 0, g), np.where(nan_w, 0, w)
    view = f"i{g.dtype.itemsize}"
    return bool(np.array_equal(g.view(view), w.view(view)))


def _call(name, a, b, **kw):
    return R.dot(a, b, **kw) if name == "dot" else getattr(R, name)(a, **kw)


def _subsets(ndim):
    for k in range(1, ndim):
        yield from itertools.combinations(range(ndim), k)


def _by_sub_boxes(name, a, b, red, origin=None, domain=None):
    """The definition: the scalar function on the sub-box of every kept cell."""
    shape = a.shape
    origin = tuple(origin) if origin is not None else (0,) * len(shape)
    domain = tuple(domain) if domain is not None else tuple(s - o for s, o in zip(shape, origin))
    kept = [d for d in range(len(shape)) if d not in red]
    out = []
    for idx in np.ndindex(*[domain[d] for d in kept]):
        o, dm = list(origin), list(domain)
        for d, i in zip(kept, idx):
            o[d], dm[d] = origin[d] + i, 1
        out.append(_call(name, a, b, origin=tuple(o), domain=tuple(dm)))
    return np.array(out).reshape([domain[d] for d in kept])


# ---------------------------------------------------------------------------------------------
# CPU: the vectorised restatement is the scalar functions, cell by cell
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape,box", [((5, 4, 3), ((1, 0, 1), (3, 4, 2))), ((33, 7, 9), ((2, 1, 0), (29, 5, 8))),
                                       ((3, 2, 4, 2, 2), ((1, 0, 1, 0, 0), (2, 2, 3, 2, 1)))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "box")
def test_every_cell_is_the_scalar_function_on_its_sub_box(shape, box, dtype):
    rng = np.random.default_rng(len(shape) * 100 + shape[0])
    a, b = _data(rng, shape, dtype, special=True), _data(rng, shape, dtype)
    for red in _subsets(len(shape)):
        for kw in ({}, dict(origin=box[0], domain=box[1])):
            for name in FUNCTIONS:
                got = _call(name, a, b, axis=red, **kw)
                assert isinstance(got, np.ndarray)
                assert _same(got, _by_sub_boxes(name, a, b, red, **kw)), (name, red, kw)
    # scan and fold_sums: per-cell arrays of the same values
    red = (0, 2)
    sc = R.scan(a, axis=red)
    assert sc[6] == shape[0] * shape[2] and isinstance(sc[6], int)
    kshape = tuple(s for d, s in enumerate(shape) if d not in red)
    for idx in np.ndindex(*kshape):
        sl = [slice(None)] * len(shape)
        for d, i in zip([d for d in range(len(shape)) if d not in red], idx):
            sl[d] = slice(i, i + 1)
        one = R.scan(a[tuple(sl)])
        assert _same(tuple(v[idx] for v in sc[:6]), one[:6]) and one[6] == sc[6], idx
        M = np.abs(np.nan_to_num(a.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)).max() if a.dtype.kind == "f" else 0
        want = R.fold_sums(a[tuple(sl)], M, a.size)
        got = R.fold_sums(a, np.full(kshape, M, dtype=np.float64), a.size, axis=red)
        assert _same(tuple(v[idx] for v in got), want), idx


KINDS = ("nan", "pinf", "both_inf", "zeros", "huge", "overflow", "subnormal", "cancel", "wide", "wide", "wide", "wide")


def _mixed(cells, n, seed=7):
    """``[cells, n]`` f64: row ``c`` is of kind ``KINDS[c % 12]``, so neighbouring cells of one call
    need different rules and fold plans."""
    rng = np.random.default_rng(seed)
    out = np.empty((cells, n))
    for c in range(cells):
        kind = KINDS[c % len(KINDS)]
        row = _wide(rng, (n,)) * 2.0 ** float(rng.integers(-200, 200))
        if kind == "nan":
            row[rng.integers(0, n)] = np.nan
        elif kind == "pinf":
            row[rng.integers(0, n)] = np.inf
        elif kind == "both_inf":
            row[0], row[n - 1] = np.inf, -np.inf
        elif kind == "zeros":
            row = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        elif kind == "huge":  # M near 2**1023: E0 > 1022, the summands are scaled; the sum is finite
            row = _wide(rng, (n,), binades=10) * 2.0**1010
            row[0], row[1] = 1.7e308, -1.6e308
        elif kind == "overflow":
            row = np.abs(_wide(rng, (n,), binades=10)) * 2.0**1000
            row[0], row[1] = 1.7e308, 1.0e308
        elif kind == "subnormal":
            row = rng.integers(-(2**20), 2**20, n).astype(np.float64) * 2.0**-1074
        elif kind == "cancel":
            row = np.zeros(n)
            row[0], row[n // 2], row[n - 1] = 1e16, 3 * 2.0**-60, -1e16  # a plain sum in this order gives 0
        out[c] = row
    return out


def _check_mixed_columns(got, cols):
    for c in range(cols.shape[0]):
        kind, v = KINDS[c % len(KINDS)], got[c]
        if kind in ("nan", "both_inf"):
            assert np.isnan(v), (c, kind)
        elif kind in ("pinf", "overflow"):
            assert v == np.inf, (c, kind)
        elif kind == "zeros":
            assert v == 0 and not np.signbit(v), c
        elif kind == "cancel":
            assert v == 3 * 2.0**-60, c
        else:  # within the rule's bound of the exact sum (test_reduce.py test_accuracy_bound)
            p = R.fold_plan(np.abs(cols[c]).max(), cols.shape[1])
            bound = cols.shape[1] * 2.0 ** (p.E[2] - 52) / p.scale
            assert np.isfinite(v) and abs(v - math.fsum(cols[c])) <= bound, (c, kind, v)
    assert R.fold_plan(np.abs(cols[4]).max(), cols.shape[1]).scale < 1.0  # "huge" is scaled
    assert all(R.fold_plan(np.abs(cols[6]).max(), cols.shape[1]).ident)  # "subnormal" takes q = r


def test_cells_with_different_plans_in_one_call():
    cols = _mixed(24, 40)
    for arr, ax in ((cols.reshape(4, 6, 40), 2), (np.ascontiguousarray(cols.T).reshape(8, 5, 24), (0, 1))):
        got = R.sum(arr, axis=ax).reshape(-1)
        _check_mixed_columns(got, cols)
        red = RA.normalize_axis(ax, 3)
        for name in FUNCTIONS:
            assert _same(_call(name, arr, arr, axis=ax), _by_sub_boxes(name, arr, arr, red)), name
    zeros = cols[3].reshape(1, 40)
    assert np.signbit(R.min(zeros, axis=1)[0]) and not np.signbit(R.max(zeros, axis=1)[0])


def test_order_independence_along_reduced_axes():
    rng = np.random.default_rng(11)
    a, b = _wide(rng, (33, 7, 9)), _wide(rng, (33, 7, 9))
    for ax in ((0,), (0, 2), (1,)):
        want_sum, want_dot = R.sum(a, axis=ax), R.dot(a, b, axis=ax)
        for d in ax:
            perm = rng.permutation(a.shape[d])
            pa, pb = np.take(a, perm, axis=d), np.take(b, perm, axis=d)
            assert _same(R.sum(pa, axis=ax), want_sum) and _same(R.dot(pa, pb, axis=ax), want_dot), (ax, d)
    assert not _same(np.sum(a, axis=0), np.sum(np.take(a, rng.permutation(33), axis=0), axis=0))  # a plain sum is not


def test_axis_arguments():
    rng = np.random.default_rng(12)
    a = _wide(rng, (5, 4, 3))
    # negative values count from the end; an int is a one-element tuple; order does not matter
    assert _same(R.sum(a, axis=-1), R.sum(a, axis=(2,))) and _same(R.sum(a, axis=(-1, 0)), R.sum(a, axis=(0, 2)))
    assert _same(R.max(a, axis=(2, 0)), R.max(a, axis=(0, 2))) and R.sum(a, axis=1).shape == (5, 3)
    for bad in ((0, 0), (1, -2), 3, -4, (0, 5), 1.5, "x"):
        with pytest.raises(ValueError):
            R.sum(a, axis=bad)
        with pytest.raises(ValueError):
            R.min(a, axis=bad)
    # every axis listed: the 0-d result of axis=None, same bits
    for name in FUNCTIONS:
        got = _call(name, a, a, axis=(0, 1, 2))
        assert np.ndim(got) == 0 and _same(got, _call(name, a, a)), name
        assert _same(_call(name, a, a, axis=(2, -3, 1), origin=(1, 1, 0)), _call(name, a, a, origin=(1, 1, 0)))
    # axis=() reduces nothing: every cell is its own sub-box
    m = np.array([[1.5, -0.0], [np.nan, -np.inf]], dtype=np.float32)
    got = R.sum(m, axis=())
    assert got.dtype == np.float64 and got.shape == (2, 2) and _same(got, np.array([[1.5, 0.0], [np.nan, -np.inf]]))
    assert _same(R.min(m, axis=()), m) and _same(R.count_nonfinite(m, axis=()), np.array([[0, 0], [1, 1]]))
    # dtypes
    a32, ai = a.astype(np.float32), _data(rng, (5, 4, 3), np.int32)
    assert R.sum(a32, axis=0).dtype == np.float64 and R.norm2(a32, axis=0).dtype == np.float64
    assert R.min(a32, axis=0).dtype == np.float32 and R.absmax(a32, axis=0).dtype == np.float32
    assert R.sum(ai, axis=0).dtype == np.int64 and R.dot(ai, ai, axis=0).dtype == np.int64
    assert R.max(ai, axis=0).dtype == np.int32 and R.absmax(ai, axis=0).dtype == np.int64
    assert R.count_nonfinite(ai, axis=0).dtype == np.int64 and not R.count_nonfinite(ai, axis=0).any()


def test_empty_extents():
    a = np.ones((5, 4, 3))
    # an empty reduced extent: 0 for the sums and counts, an error for the extrema
    kw = dict(origin=(0, 1, 0), domain=(5, 0, 3))
    for name, dt in (("sum", np.float64), ("dot", np.float64), ("norm2", np.float64), ("count_nonfinite", np.int64)):
        got = _call(name, a, a, axis=1, **kw)
        assert got.shape == (5, 3) and got.dtype == dt and not got.any(), name
    assert R.sum(a.astype(np.int32), axis=(1, 2), **kw).dtype == np.int64
    for fn in (R.min, R.max, R.absmax):
        with pytest.raises(ValueError, match="zero-size"):
            fn(a, axis=1, **kw)
    # an empty kept extent: an empty array of the right shape and dtype
    for name in FUNCTIONS:
        got = _call(name, a, a, axis=(0, 2), **kw)
        assert got.shape == (0,), name
        assert _call(name, a, a, axis=0, **kw).shape == (0, 3)
    assert R.min(a.astype(np.float32), axis=0, **kw).dtype == np.float32
    assert R.absmax(a.astype(np.int32), axis=0, **kw).dtype == np.int64


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_integer_wrap_around_per_cell(dtype):
    rng = np.random.default_rng(13)
    i = np.iinfo(dtype)
    x = rng.integers(i.max - 1000, i.max, (7, 33, 3), dtype=dtype, endpoint=True)
    x[:, :, 1] = rng.integers(i.min, i.min + 1000, (7, 33), dtype=dtype)
    for ax in ((1,), (0, 1), (2,)):
        assert _same(R.sum(x, axis=ax), np.sum(x, axis=ax, dtype=np.int64)), ax
        with np.errstate(over="ignore"):
            want = np.sum(x.astype(np.int64) * x.astype(np.int64), axis=ax, dtype=np.int64)
        assert _same(R.dot(x, x, axis=ax), want), ax
    if dtype == np.int64:
        assert (np.sum(x.astype(object), axis=(0, 1)) != R.sum(x, axis=(0, 1))).all()  # every level wrapped
    y = np.array([[i.min, 5], [3, -4]], dtype=dtype)
    assert _same(R.absmax(y, axis=1), np.array([5 if dtype == np.int64 else 2**31, 4], dtype=np.int64))  # |INT64_MIN| wraps, as in numpy


def test_plan_axis_canonical_forms():
    S, L, G = RA.SEGMENT, RA.LANE, RA.GENERIC
    shape, st = (65, 3, 67), (1, 72, 300)  # an I-first storage box with a halo: padded J and K strides
    assert R.plan_axis(shape, (0, 1), st) == (((67,), (300,), (0,)), ((3, 65), (72, 1), (0, 0)), S)
    assert R.plan_axis(shape, (2,), st) == (((3, 65), (72, 1), (0, 0)), ((67,), (300,), (0,)), L)
    assert R.plan_axis(shape, (0,), st) == (((67, 3), (300, 72), (0, 0)), ((65,), (1,), (0,)), S)
    assert R.plan_axis(shape, (1, 2), st) == (((65,), (1,), (0,)), ((67, 3), (300, 72), (0, 0)), L)
    assert R.plan_axis(shape, (0, 2), st)[2] == S
    # merging inside a group: K continues the J rows
    assert R.plan_axis(shape, (0,), (1, 72, 216)) == (((201,), (72,), (0,)), ((65,), (1,), (0,)), S)
    assert R.plan_axis((4, 5, 6), (1, 2), (30, 6, 1)) == (((4,), (30,), (0,)), ((30,), (1,), (0,)), G)  # a row of 30
    assert R.plan_axis((4, 5, 8), (1, 2), (40, 8, 1))[1:] == (((40,), (1,), (0,)), S)
    # ... and never across the groups: dense C order, the middle axis reduced
    assert R.plan_axis((4, 5, 64), (1,), (320, 64, 1)) == (((4, 64), (320, 1), (0, 0)), ((5,), (64,), (0,)), L)
    assert R.plan_axis((4, 5, 64), (0, 1), (320, 64, 1)) == (((64,), (1,), (0,)), ((20,), (64,), (0,)), L)
    # the second source keeps dimensions apart and decides the path with the first
    assert R.plan_axis((4, 5, 64), (1, 2), (320, 64, 1), (400, 80, 1))[1] == ((5, 64), (64, 1), (80, 1))
    assert R.plan_axis((4, 64), (1,), (64, 1), (0, 0))[2] == G  # a broadcast second source
    assert R.plan_axis((4, 64), (1,), (64, 1), (64, 1))[2] == S
    # stride 2, and rows of 31
    assert R.plan_axis((5, 64), (1,), (128, 2))[2] == G and R.plan_axis((5, 64), (0,), (128, 2))[2] == G
    assert R.plan_axis((40, 31), (0,), (31, 1))[2] == G and R.plan_axis((40, 31), (1,), (31, 1))[2] == G
    assert R.plan_axis((40, 32), (0,), (32, 1))[2] == L and R.plan_axis((40, 32), (1,), (32, 1))[2] == S
    # extent-1 dimensions are dropped; an empty group; an empty box
    assert R.plan_axis((40, 1, 3), (1,), (1, 40, 48)) == (((3, 40), (48, 1), (0, 0)), ((), (), ()), L)
    assert R.plan_axis((40, 1, 3), (1,), (1, 40, 40)) == (((120,), (1,), (0,)), ((), (), ()), L)
    assert R.plan_axis((257, 33, 1), (0, 1), (1, 264, 8712)) == (((), (), ()), ((33, 257), (264, 1), (0, 0)), S)
    assert R.plan_axis((3, 0), (1,), (1, 1))[2] is None
    with pytest.raises(ValueError):
        R.plan_axis((3, 4), (0,), (-4, 1))
    with pytest.raises(ValueError):
        R.plan_axis((3, 4), (2,), (4, 1))


def test_host_column_sum_of_a_model_sized_field_is_usable():
    import time

    x = _wide(np.random.default_rng(14), (256, 256, 80))
    t0 = time.perf_counter()
    got = R.sum(x, axis=2)
    assert time.perf_counter() - t0 < 20.0  # vectorised: a loop of 65536 scalar calls takes minutes
    assert got.shape == (256, 256) and _same(got[17, 200], R.sum(x[17, 200])) and _same(got[255, 0], R.sum(x[255, 0]))


# ---------------------------------------------------------------------------------------------
# GPU: the library against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------
AXES = [(0, 1), (2,), (0,), (1, 2), (0, 2)]


def _device():
    import torch

    torch.empty(1, device="cuda")
    return torch


def _check_every_function(dev_a, dev_b, host_a, host_b, what, axis, host_cache=None, **kw):
    """Every public function on device views against the restatement on their host copies."""
    host_cache = host_cache if host_cache is not None else {}

    def host(key, fn):
        if key not in host_cache:
            host_cache[key] = fn()
        return host_cache[key]

    def finite_max(h):
        h = np.abs(np.asarray(h, dtype=np.float64))
        return float(np.max(h[np.isfinite(h)], initial=1.0))

    for name in FUNCTIONS:
        got = _call(name, dev_a, dev_b, axis=axis, **kw)
        assert got.is_cuda and got.is_contiguous(), (what, name)
        ok = _same(got, host(name, lambda: _call(name, host_a, host_b, axis=axis, **kw)))
        assert ok, (what, name, axis, kw)
    for two in (False, True):
        args_d, args_h = ((dev_a, dev_b), (host_a, host_b)) if two else ((dev_a,), (host_a,))
        sc = host(("scan", two), lambda: R.scan(*args_h, axis=axis, **kw))
        ok = _same(R.scan(*args_d, axis=axis, **kw), sc)
        assert ok, (what, "scan", two, axis, kw)
        # folds against the (M, N) of a larger reduction: per cell twice its own maximum (where that is
        # not finite, a bound of every finite summand), three times the count
        if sc[0].dtype.kind == "f":
            bound = finite_max(host_a) * (finite_max(host_b) if two else 1.0)
            with np.errstate(over="ignore"):  # a cell near the top of the range: M = inf, every fold sum is 0
                M = np.where(np.isfinite(sc[0]), sc[0], bound) * 2.0
        else:
            M = np.zeros(sc[0].shape)
        want = host(("folds", two), lambda: R.fold_sums(*args_h, M, 3 * sc[6], axis=axis, **kw))
        ok = _same(R.fold_sums(*args_d, M, 3 * sc[6], axis=axis, **kw), want)
        assert ok, (what, "folds", two, axis, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("axis", AXES, ids=lambda a: "axis" + "".join(map(str, a)))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(65, 3, 67), (257, 33, 40)], ids=lambda s: "x".join(map(str, s)))
def test_storages_match_the_restatement(shape, dtype, axis):
    _device()
    rng = np.random.default_rng(31)
    ha, hb = _data(rng, shape, dtype, special=True), _data(rng, shape, dtype)
    box = dict(origin=(1, 2, 0), domain=(shape[0] - 2, shape[1] - 2, shape[2]))
    caches = ({}, {})
    for ai in ((0, 0, 0), (1, 2, 0)):
        da = storage.from_array(ha, dtype, backend=BE, aligned_index=ai)
        db = storage.from_array(hb, dtype, backend=BE, aligned_index=ai)
        _check_every_function(da, db, ha, hb, ai, axis, caches[0])
        _check_every_function(da, db, ha, hb, ai, axis, caches[1], **box)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda d: np.dtype(d).name)
def test_cells_with_different_plans_on_the_device(dtype):
    _device()
    cols = _mixed(96, 80)
    if dtype == np.float32:  # the f32 range: no huge / overflow / f64-subnormal rows, the rest as they are
        cols = np.where(np.isfinite(cols), np.clip(cols, -3e38, 3e38), cols).astype(np.float32)
    for arr, ax in ((np.ascontiguousarray(cols.T).reshape(40, 2, 96), (0, 1)), (cols.reshape(48, 2, 80), 2)):
        arr = arr.astype(dtype)
        d = storage.from_array(arr, dtype, backend=BE, aligned_index=(1, 1, 0))
        assert RA._AxisPass(R._box(d, None, None), None, np.dtype(dtype), RA.normalize_axis(ax, 3), None, None).path == (
            RA.SEGMENT if ax == (0, 1) else RA.LANE)
        got = R.sum(d, axis=ax)
        if dtype == np.float64:
            _check_mixed_columns(_np(got).reshape(-1), cols)
        _check_every_function(d, d, arr, arr, "mixed", ax)


@pytest.mark.gpu
def test_part_count_independence():
    _device()
    rng = np.random.default_rng(33)
    shape = (257, 33, 40)
    for dtype in (np.float64, np.float32):
        ha, hb = _data(rng, shape, dtype), _data(rng, shape, dtype)
        da = storage.from_array(ha, dtype, backend=BE, aligned_index=(3, 3, 0))
        db = storage.from_array(hb, dtype, backend=BE, aligned_index=(3, 3, 0))
        for ax, path in (((0, 1), RA.SEGMENT), ((2,), RA.LANE), ((0,), RA.SEGMENT), ((1, 2), RA.LANE)):
            p = RA._AxisPass(R._box(da, None, None), None, np.dtype(dtype), ax, None, None)
            assert p.path == path
            want = {n: _call(n, ha, hb, axis=ax) for n in ("sum", "dot", "min", "count_nonfinite")}
            box = dict(origin=(1, 2, 3))
            want_box, want_scan = R.sum(ha, axis=ax, **box), R.scan(ha, axis=ax)
            for parts in (1, 3, 7, None):
                for n, w in want.items():
                    assert _same(_call(n, da, db, axis=ax, _parts=parts), w), (ax, n, parts)
                assert _same(R.sum(da, axis=ax, _parts=parts, **box), want_box), (ax, parts)
                assert _same(R.scan(da, axis=ax, _parts=parts), want_scan), (ax, parts)
                assert RA._AxisPass(R._box(da, None, None), None, np.dtype(dtype), ax, None, parts).parts == (parts or p.parts)
        # few kept cells are split into parts by default, many are not
        assert RA._AxisPass(R._box(da, None, None), None, np.dtype(dtype), (0, 1), None, None).parts > 1
        big = storage.empty((1024, 512, 1), dtype, backend=BE)
        assert RA._AxisPass(R._box(big, None, None), None, np.dtype(dtype), (2,), None, None).parts == 1


@pytest.mark.gpu
def test_one_kept_cell_one_reduced_element_and_short_rows():
    _device()
    rng = np.random.default_rng(34)
    for dtype in (np.float64, np.int32):
        h = _data(rng, (257, 33, 1), dtype)
        d = storage.from_array(h, dtype, backend=BE, aligned_index=(1, 1, 0))
        _check_every_function(d, d, h, h, "one cell", (0, 1))  # one kept cell
        assert R.sum(d, axis=(0, 1)).shape == (1,) and _same(R.sum(d, axis=(0, 1))[0], R.sum(h))
        _check_every_function(d, d, h, h, "one element", (2,))  # one reduced element per cell
        _check_every_function(d, d, h, h, "axis ()", ())
        h = _data(rng, (31, 5, 7), dtype)  # rows of 31: GENERIC whatever the axis
        d = storage.from_array(h, dtype, backend=BE)
        for ax in ((0,), (1, 2), (0, 2)):
            _check_every_function(d, d, h, h, "short rows", ax, origin=(0, 1, 1))
        # data dimensions count as axes
        h = _data(rng, (40, 6, 5, 2, 3), dtype)
        d = storage.from_array(h, np.dtype((dtype, (2, 3))), backend=BE)
        for ax in ((0, 1, 2), (3, 4), (0, -1)):
            _check_every_function(d, d, h, h, "data dims", ax)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32], ids=lambda d: np.dtype(d).name)
def test_phases_broadcast_generic_views_and_foreign_objects(dtype):
    torch = _device()
    rng = np.random.default_rng(35)
    shape = (65, 3, 67)
    ha, hb = _data(rng, shape, dtype), _data(rng, shape, dtype)
    da = storage.from_array(ha, dtype, backend=BE, aligned_index=(1, 2, 0))
    db = storage.from_array(hb, dtype, backend=BE, aligned_index=(0, 0, 0))  # another 16-B phase: element per lane
    for ax in AXES:
        assert _same(R.dot(da, db, axis=ax), R.dot(ha, hb, axis=ax)), ax
        assert _same(R.dot(da, db, axis=ax, origin=(3, 0, 0)), R.dot(ha, hb, axis=ax, origin=(3, 0, 0))), ax
    # a broadcast (stride 0) second source
    h = _data(rng, (9, 70, 6), dtype)
    wide = torch.from_numpy(h).cuda()
    hb = _data(rng, (9, 1, 6), dtype)
    vb = torch.from_numpy(hb).cuda().expand(9, 70, 6)
    for ax in ((1,), (0, 2), (2,)):
        assert _same(R.dot(wide, vb, axis=ax), R.dot(h, np.broadcast_to(hb, h.shape), axis=ax)), ax
        _check_every_function(wide, wide, h, h, "c order", ax)
    # a view with innermost stride 2 (not a storage): the generic path
    va, hv = wide[:, ::2, 1], np.ascontiguousarray(h[:, ::2, 1])
    for ax in ((0,), (1,)):
        assert R.plan_axis(va.shape, ax, va.stride())[2] == RA.GENERIC
        _check_every_function(va, va, hv, hv, "stride 2", ax)

    class Foreign:  # any object with __cuda_array_interface__ takes the device path
        __cuda_array_interface__ = wide.__cuda_array_interface__

    got = R.sum(Foreign(), axis=(0, 2))
    assert got.is_cuda and _same(got, R.sum(h, axis=(0, 2)))


@pytest.mark.gpu
def test_nothing_outside_the_box_is_read():
    torch = _device()
    rng = np.random.default_rng(36)
    shape, halo = (65, 5, 41), 3
    inner = _wide(rng, shape)
    for dtype in (np.float64, np.float32):
        d = storage.empty((shape[0] + 2 * halo, shape[1] + 2 * halo, shape[2]), dtype, backend=BE, aligned_index=(halo, halo, 0))
        t = storage._as_device_tensor(d)
        flat = torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
        flat.fill_(float("nan"))  # the whole flat buffer, padding included
        t[halo:-halo, halo:-halo, :] = torch.from_numpy(inner.astype(dtype)).cuda()
        kw = dict(origin=(halo, halo, 0), domain=shape)
        for ax in AXES:
            for name in ("sum", "min", "max", "absmax", "norm2", "dot"):
                got = _np(_call(name, d, d, axis=ax, **kw))
                assert not np.isnan(got).any(), (name, ax)
                assert _same(got, _call(name, inner.astype(dtype), inner.astype(dtype), axis=ax)), (name, ax)
            assert not _np(R.count_nonfinite(d, axis=ax, **kw)).any(), ax
            assert int(_np(R.count_nonfinite(d, axis=ax)).sum()) == t.numel() - inner.size, ax


@pytest.mark.gpu
def test_no_host_synchronisation_and_streams(monkeypatch):
    torch = _device()
    h = _wide(np.random.default_rng(37), (65, 3, 67))
    d = storage.from_array(h, backend=BE)
    R.sum(d, axis=2)  # library loaded
    m_dev = torch.from_numpy(np.abs(h).max(axis=(0, 1))).cuda()

    def no_sync(*a, **k):
        raise AssertionError("device->host transfer or synchronisation in a reduction")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, no_sync)
        m.setattr(torch.cuda, "synchronize", no_sync)
        results = [R.sum(d, axis=(0, 1)), R.sum(d, axis=2), R.dot(d, d, axis=0), R.absmax(d, axis=(1, 2)),
                   R.count_nonfinite(d, axis=2, origin=(1, 1, 1)), R.norm2(d, axis=(0, 2))]
        sc = R.scan(d, axis=(0, 1))
        results += list(R.fold_sums(d, sc[0], sc[6], axis=(0, 1))) + list(R.fold_sums(d, m_dev, h.size, axis=(0, 1)))
    assert _same(results[0], R.sum(h, axis=(0, 1))) and _same(results[1], R.sum(h, axis=2))
    assert _same(results[3], R.absmax(h, axis=(1, 2))) and _same(results[5], R.norm2(h, axis=(0, 2)))
    hs = R.scan(h, axis=(0, 1))
    assert _same(tuple(results[6:9]), R.fold_sums(h, hs[0], hs[6], axis=(0, 1)))
    assert _same(tuple(results[9:12]), R.fold_sums(h, np.abs(h).max(axis=(0, 1)), h.size, axis=(0, 1)))
    # a side stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = R.sum(d, axis=(0, 1), stream=s)
    got_dot = R.dot(d, d, axis=2, origin=(1, 1, 0), stream=s)
    s.synchronize()
    assert _same(got, R.sum(h, axis=(0, 1))) and _same(got_dot, R.dot(h, h, axis=2, origin=(1, 1, 0)))
    # empty extents: no launch, results on the device
    e = R.sum(d, axis=2, origin=(0, 0, 0), domain=(65, 3, 0))
    assert e.is_cuda and e.shape == (65, 3) and e.dtype == torch.float64 and not _np(e).any()
    e = R.min(d, axis=2, origin=(0, 0, 0), domain=(65, 0, 5))
    assert e.is_cuda and e.shape == (65, 0)
    with pytest.raises(ValueError, match="zero-size"):
        R.max(d, axis=2, origin=(0, 0, 0), domain=(65, 3, 0))
    # all axes listed: the scalar library's 0-d result
    assert _same(R.sum(d, axis=(0, 1, 2)), R.sum(h)) and R.sum(d, axis=(0, 1, 2)).dim() == 0


@pytest.mark.gpu
def test_library_reports_its_abi_version_and_path():
    _device()
    assert RA.abi_version() == 1
    cases = [((65, 3, 67), ax, (1, 72, 300), None) for ax in AXES + [(1,)]]
    cases += [((5, 64), (1,), (128, 2), None), ((5, 64), (0,), (128, 2), None), ((40, 31), (0,), (31, 1), None),
              ((40, 32), (0,), (32, 1), None), ((4, 64), (1,), (64, 1), (0, 0)), ((4, 64), (1,), (64, 1), (64, 1)),
              ((4, 5, 64), (1,), (320, 64, 1), (320, 64, 1)), ((257, 33, 1), (0, 1), (1, 264, 8712), None),
              ((40, 1, 3), (1,), (1, 40, 48), None)]
    for shape, ax, sa, sb in cases:
        red = RA.normalize_axis(ax, len(shape))
        kept, reduced, _, path = RA._plan(shape, red, sa, sb)
        desc = RA.descriptor(kept, reduced, np.float64, 64, 64 if sb is not None else None)
        assert RA.library_path_name(desc) == path == R.plan_axis(shape, ax, sa, sb)[2], (shape, ax, sa, sb)


@pytest.mark.gpu
def test_level_sums_are_the_scalar_library_on_each_plane():
    _device()
    h = _wide(np.random.default_rng(38), (257, 33, 40))
    d = storage.from_array(h, backend=BE, aligned_index=(1, 1, 0))
    prof, mx = R.sum(d, axis=(0, 1)), R.max(d, axis=(0, 1))
    for k in (0, 17, 39):
        plane = dict(origin=(0, 0, k), domain=(257, 33, 1))
        assert _same(prof[k], R.sum(d, **plane)) and _same(mx[k], R.max(d, **plane)), k


@pytest.mark.gpu
def test_global_axis_reductions_on_device_tensors_over_rccl():
    """The device path of ``distributed.reduce`` with ``axis=`` in a world of one rank."""
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
        rng = np.random.default_rng(39)
        box = dict(origin=(1, 1, 0), domain=(63, 2, 67))
        for dtype in (np.float64, np.float32, np.int64):
            ha, hb = _data(rng, (65, 3, 67), dtype, special=True), _data(rng, (65, 3, 67), dtype)
            da = storage.from_array(ha, dtype, backend=BE, aligned_index=(1, 1, 0))
            db = storage.from_array(hb, dtype, backend=BE, aligned_index=(1, 1, 0))
            for ax in ((0, 1), (1,)):
                for kw in (box, dict(box, global_count=63 * 2 if ax == (0, 1) else 2)):
                    local = {k: v for k, v in kw.items() if k != "global_count"}
                    got = G.global_sum(da, axis=ax, **kw)
                    assert got.is_cuda and _same(got, R.sum(da, axis=ax, **local)) and _same(got, R.sum(ha, axis=ax, **local))
                    assert _same(G.global_dot(da, db, axis=ax, **kw), R.dot(ha, hb, axis=ax, **local))
                    assert _same(G.global_norm2(da, axis=ax, **kw), R.norm2(ha, axis=ax, **local))
                    assert _same(G.global_min(da, axis=ax, **kw), R.min(ha, axis=ax, **local))
                    assert _same(G.global_max(da, axis=ax, **kw), R.max(ha, axis=ax, **local))
                    assert _same(G.global_absmax(da, axis=ax, **kw), R.absmax(ha, axis=ax, **local))
                    assert _same(G.global_count_nonfinite(da, axis=ax, **kw), R.count_nonfinite(ha, axis=ax, **local))
            # a rank whose part is empty along a reduced axis contributes the identities
            none = dict(origin=(1, 1, 0), domain=(63, 0, 67))
            assert not _np(G.global_sum(da, axis=(0, 1), **none)).any()
            with pytest.raises(ValueError):
                G.global_min(da, axis=(0, 1), **none)
    finally:
        dist.destroy_process_group()
