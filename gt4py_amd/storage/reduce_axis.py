"""Axis reductions of ``storage.reduce``: level profiles, column sums (``include/gtmi_reduce_axis.h``,
``csrc/gtmi_reduce_axis.hip``). ``storage.reduce.sum(arr, axis=...)`` and its siblings end here.

**Definition.** The axes listed in ``axis`` are reduced, the others kept in their order (no
``keepdims``). Element ``idx`` of a result has the bits the scalar function of ``storage.reduce``
returns for the sub-box of ``idx``: the box with every kept dimension narrowed to the one index. So
every kept cell has its own absolute maximum ``M`` and its own fold plan; the non-finite rules, the
``+0.0`` rule for ``M == 0``, the scaling at ``E0 > 1022`` and the ``q = r`` folds apply per cell.
``N``, the reduced count, is the same for every cell. ``axis=()`` reduces nothing: every cell is its
own sub-box (``sum`` then gives the cell as f64, ``-0.0`` as ``+0.0``). An empty reduced extent
gives 0 for the sums and counts and ``ValueError`` for the extrema; an empty kept extent gives an
empty array.

The numpy code here is that definition, vectorised over the kept cells, and the execution path of
host arrays. Device tensors go through the axis reduction library, which writes its results in
the order of the canonical kept group (``plan_axis``); a strided view puts them back into the order
of the array's dimensions.
"""

from __future__ import annotations

import builtins
import ctypes
import hashlib
import operator
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from gt4py_amd.runtime import jit
from gt4py_amd.storage import reduce as _r

_SRC = os.path.join(jit.CSRC_DIR, "gtmi_reduce_axis.hip")
_HEADERS = (os.path.join(jit.INCLUDE_DIR, "gtmi_reduce_axis.h"), os.path.join(jit.INCLUDE_DIR, "gtmi_reduce.h"),
            os.path.join(jit.CSRC_DIR, "gtmi_reduce_rules.h"))
_lock = threading.Lock()
_lib = None

MAX_DIMS = _r.MAX_DIMS
MAX_PARTS = 4096  # GTMI_REDUCE_AXIS_MAX_PARTS
SEGMENT, LANE, GENERIC = "SEGMENT", "LANE", "GENERIC"
_PATH_CODES = {0: SEGMENT, 1: LANE, 2: GENERIC}
# slot masks of the scan (gtmi_reduce.h slot numbering)
MASK_BASE = 0x03F  # absmax, min, max and the three counts
MASK_SUM = 0x039  # what the finish reads: absmax and the three counts
MASK_NONFINITE = 1 << 6
MASK_ALL = 0x77F


class GtmiReduceAxisDesc(ctypes.Structure):
    _fields_ = [
        ("a", ctypes.c_void_p),
        ("b", ctypes.c_void_p),
        ("k_extent", ctypes.c_int64 * MAX_DIMS),
        ("k_a_stride", ctypes.c_int64 * MAX_DIMS),
        ("k_b_stride", ctypes.c_int64 * MAX_DIMS),
        ("r_extent", ctypes.c_int64 * MAX_DIMS),
        ("r_a_stride", ctypes.c_int64 * MAX_DIMS),
        ("r_b_stride", ctypes.c_int64 * MAX_DIMS),
        ("k_ndim", ctypes.c_int32),
        ("r_ndim", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


# ---------------------------------------------------------------------------------------------
# axes
# ---------------------------------------------------------------------------------------------
def normalize_axis(axis, ndim: int) -> Tuple[int, ...]:
    """``axis`` (an int or a tuple of ints, negative values counting from the end) as the sorted
    tuple of reduced dimensions; ``ValueError`` for duplicates and values out of range."""
    if isinstance(axis, (tuple, list)):
        items = list(axis)
    else:
        items = [axis]
    out: List[int] = []
    for v in items:
        try:
            i = operator.index(v)
        except TypeError:
            raise ValueError(f"reduce: invalid axis {v!r}") from None
        if not -ndim <= i < ndim:
            raise ValueError(f"reduce: axis {i} is out of range for an array of {ndim} dimensions")
        i %= ndim
        if i in out:
            raise ValueError(f"reduce: duplicate axis {i} in {tuple(items)}")
        out.append(i)
    return tuple(sorted(out))


def _ndim(arr) -> int:
    if hasattr(arr, "shape"):
        return len(arr.shape)
    if hasattr(arr, "__cuda_array_interface__"):
        return len(arr.__cuda_array_interface__["shape"])
    return np.ndim(arr)


def reduced_axes(arr, axis) -> Optional[Tuple[int, ...]]:
    """The reduced dimensions of ``arr`` for ``axis``; None when every dimension is listed (the
    scalar path of ``storage.reduce`` then gives the 0-d result)."""
    ndim = _ndim(arr)
    red = normalize_axis(axis, ndim)
    return None if len(red) == ndim else red


# ---------------------------------------------------------------------------------------------
# the restatement, vectorised over the kept cells (host arrays)
# ---------------------------------------------------------------------------------------------
def _split(shape: Sequence[int], red: Sequence[int]):
    kept = [d for d in range(len(shape)) if d not in red]
    kshape = tuple(int(shape[d]) for d in kept)
    cells = int(np.prod(kshape, dtype=object)) if kshape else 1
    nred = int(np.prod([int(shape[d]) for d in red], dtype=object)) if len(red) else 1
    return kept, kshape, cells, nred


def _summands_host(va: np.ndarray, vb: Optional[np.ndarray], dt: np.dtype, red):
    """``(kept shape, summands[cells, N])``: f64 / int64, a copy (only the box's cells are read)."""
    st = np.float64 if _r._floating(dt) else np.int64
    if vb is not None and tuple(vb.shape) != tuple(va.shape):
        raise ValueError(f"reduce: boxes differ in shape ({tuple(va.shape)}, {tuple(vb.shape)})")
    kept, kshape, cells, nred = _split(va.shape, red)
    perm = kept + list(red)
    x = np.array(np.transpose(va, perm), dtype=st, order="C").reshape((cells, nred))
    if vb is not None:
        with np.errstate(all="ignore"):
            x = x * np.array(np.transpose(vb, perm), dtype=st, order="C").reshape((cells, nred))  # int64 wraps
    return kshape, x


def _min_rule(v: np.ndarray, skip: Optional[np.ndarray]) -> np.ndarray:
    """Row minima of ``v`` without the entries of ``skip``; -0.0 orders below +0.0; +inf where nothing is left."""
    mn = np.where(skip, np.inf, v).min(axis=1, initial=np.inf) if skip is not None else v.min(axis=1, initial=np.inf)
    negz = ((v == 0) & np.signbit(v)).any(axis=1)
    return np.where(mn == 0, np.where(negz, -0.0, 0.0), mn)


def _max_rule(v: np.ndarray, skip: Optional[np.ndarray]) -> np.ndarray:
    mx = np.where(skip, -np.inf, v).max(axis=1, initial=-np.inf) if skip is not None else v.max(axis=1, initial=-np.inf)
    posz = ((v == 0) & ~np.signbit(v)).any(axis=1)
    return np.where(mx == 0, np.where(posz, 0.0, -0.0), mx)


def _scan_host(x: np.ndarray):
    """``(absmax, min, max, n_nan, n_pinf, n_ninf)`` per row of ``x[cells, N]`` by the rules of
    ``storage.reduce.scan``, each an array over the cells."""
    cells = x.shape[0]
    z = np.zeros(cells, dtype=np.int64)
    if x.dtype.kind == "f":
        nan = np.isnan(x)
        with np.errstate(all="ignore"):
            absmax = np.where(nan, 0.0, np.abs(x)).max(axis=1, initial=0.0)
        return (absmax, _min_rule(x, nan), _max_rule(x, nan), np.count_nonzero(nan, axis=1).astype(np.int64),
                np.count_nonzero(x == np.inf, axis=1).astype(np.int64), np.count_nonzero(x == -np.inf, axis=1).astype(np.int64))
    i = np.iinfo(np.int64)
    return (np.abs(x).max(axis=1, initial=i.min), x.min(axis=1, initial=i.max), x.max(axis=1, initial=i.min), z, z.copy(), z.copy())


def _combine_scans_host(parts, floating: bool):
    """Per-cell scans of the parts of a domain partitioned along reduced axes into one."""
    stack = [np.stack([p[k] for p in parts], axis=1) for k in range(6)]  # [cells, parts]
    if floating:
        absmax, mn, mx = stack[0].max(axis=1), _min_rule(stack[1], None), _max_rule(stack[2], None)
    else:
        absmax, mn, mx = stack[0].max(axis=1), stack[1].min(axis=1), stack[2].max(axis=1)
    return (absmax, mn, mx, *(stack[k].sum(axis=1, dtype=np.int64) for k in (3, 4, 5)))


class FoldPlans:
    """``storage.reduce.fold_plan`` for an array of absolute maxima ``M`` and one ``N``."""

    def __init__(self, M, N: int):
        M = np.asarray(M, dtype=np.float64)
        self.L = L = _r.ceil_log2(N)
        with np.errstate(all="ignore"):
            self.zero = ~(M > 0.0) | np.isinf(M)
            e = np.frexp(np.where(self.zero, 1.0, M))[1].astype(np.int64)  # M = m * 2**e, m in [0.5, 1)
            E = e + L
            big = E > 1022  # huge M: scale the summands by 2**(1022 - E0), exactly
            self.scale = np.ldexp(1.0, np.where(big, 1022 - E, 0))
            self.unscale = np.ldexp(1.0, np.where(big, E - 1022, 0))
            E = np.minimum(E, 1022)
            self.c, self.ident = [], []
            for _ in range(3):
                ident = E < -1022
                self.ident.append(ident)
                self.c.append(np.where(ident, 0.0, np.ldexp(1.5, np.maximum(E, -1022))))
                E = E - 52 + L


def _fold_sums_host(x: np.ndarray, M, N: int):
    """The three fold sums per row of ``x[cells, N']`` against ``(M[cells], N)``."""
    cells = x.shape[0]
    if x.dtype.kind != "f":
        z = np.zeros(cells, dtype=np.int64)
        return np.sum(x, axis=1, dtype=np.int64), z, z.copy()
    p = FoldPlans(np.broadcast_to(np.asarray(M, dtype=np.float64).reshape(-1), (cells,)), N)
    out = []
    with np.errstate(all="ignore"):
        r = np.where(np.isfinite(x), x, 0.0) * p.scale[:, None]
        for f in range(3):
            c = p.c[f][:, None]
            q = np.where(p.ident[f][:, None], r, (r + c) - c)
            s = np.sum(q, axis=1) + 0.0  # exact in any order; + 0.0: never -0.0
            out.append(np.where(p.zero, 0.0, s))
            r = r - q
    return tuple(out)


def _finish_sum_host(sc, folds, N: int, floating: bool):
    if not floating:
        return np.asarray(folds[0], dtype=np.int64)
    absmax, _, _, n_nan, n_pinf, n_ninf = sc[:6]
    with np.errstate(all="ignore"):
        s = (folds[0] + (folds[1] + folds[2])) * FoldPlans(absmax, N).unscale
    return np.select([(n_nan > 0) | ((n_pinf > 0) & (n_ninf > 0)), n_pinf > 0, n_ninf > 0, absmax == 0],
                     [np.nan, np.inf, -np.inf, 0.0], s).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def _canonical_group(dims):
    """``dims``: ``(extent, sa, sb, dim)`` of a group; ordered and merged ``(extent, sa, sb)`` and the
    order of the group's dimensions of extent > 1."""
    dims = sorted((t for t in dims if t[0] != 1), key=lambda t: -t[1])
    merged: List[Tuple[int, int, int]] = []
    for e, sa, sb, _ in dims:
        if merged:
            pe, psa, psb = merged[-1]
            if psa == sa * e and psb == sb * e:
                merged[-1] = (pe * e, sa, sb)
                continue
        merged.append((e, sa, sb))
    return merged, [t[3] for t in dims]


def _plan(shape, red, a_strides, b_strides):
    shape = tuple(int(e) for e in shape)
    a_strides = tuple(int(s) for s in a_strides)
    two = b_strides is not None
    b_strides = tuple(int(s) for s in b_strides) if two else (0,) * len(shape)
    if not (len(shape) == len(a_strides) == len(b_strides)):
        raise ValueError("shape and strides have different lengths")
    if any(e < 0 for e in shape):
        raise ValueError(f"negative extent in {shape}")
    if any(e > 1 and (sa < 0 or sb < 0) for e, sa, sb in zip(shape, a_strides, b_strides)):
        raise ValueError("negative strides are not supported")
    dims = [(e, sa, sb, d) for d, (e, sa, sb) in enumerate(zip(shape, a_strides, b_strides))]
    kept, korder = _canonical_group([t for t in dims if t[3] not in red])
    reduced, _ = _canonical_group([t for t in dims if t[3] in red])
    if any(e == 0 for e in shape):
        return kept, reduced, korder, None
    path = GENERIC
    for group, name in ((reduced, SEGMENT), (kept, LANE)):
        if group and group[-1][1] == 1 and (not two or group[-1][2] == 1) and group[-1][0] >= _r.SHORT_ROW:
            path = name
            break
    return kept, reduced, korder, path


def plan_axis(shape: Sequence[int], axis, a_strides: Sequence[int], b_strides: Optional[Sequence[int]] = None):
    """Canonical ``(kept, reduced, path)`` of a box of ``shape`` reduced over ``axis``, read from one
    or two sources with the given element strides. Each group is ``(extent, a_strides, b_strides)``
    with extent-1 dimensions dropped, dimensions ordered by the first source's stride (slowest
    first) and neighbours that are contiguous in every source merged -- inside the group only.
    ``path`` is SEGMENT (the reduced group ends in every source's stride-1 dimension, rows of at
    least 32), LANE (the kept group does), GENERIC, or None for an empty box. Pure Python."""
    red = normalize_axis(axis, len(tuple(shape)))
    kept, reduced, _, path = _plan(shape, red, a_strides, b_strides)

    def cols(group):
        return tuple(t[0] for t in group), tuple(t[1] for t in group), tuple(t[2] for t in group)

    return cols(kept), cols(reduced), path


# ---------------------------------------------------------------------------------------------
# the library (device tensors)
# ---------------------------------------------------------------------------------------------
def library_path() -> str:
    with open(_SRC) as f:
        source = f.read()
    h = hashlib.sha256()
    for path in _HEADERS:  # not among jit's hashed headers: make them part of this key
        with open(path, "rb") as f:
            h.update(f.read())
    return jit.compile_source(source, extra_flags=[f"-DGTMI_REDUCE_AXIS_HEADER_DIGEST=0x{h.hexdigest()[:16]}"])


def _library():
    global _lib
    with _lock:
        if _lib is None:
            import torch  # noqa: F401  (bind to torch's HIP runtime first)

            lib = ctypes.CDLL(library_path(), mode=ctypes.RTLD_LOCAL)
            desc_p, vp, i64, u32 = ctypes.POINTER(GtmiReduceAxisDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32
            lib.gtmi_reduce_axis_parts.restype = ctypes.c_int
            lib.gtmi_reduce_axis_parts.argtypes = [desc_p, ctypes.c_int]
            lib.gtmi_reduce_axis_scan.restype = ctypes.c_int
            lib.gtmi_reduce_axis_scan.argtypes = [desc_p, u32, vp, vp, ctypes.c_int, vp]
            lib.gtmi_reduce_axis_folds.restype = ctypes.c_int
            lib.gtmi_reduce_axis_folds.argtypes = [desc_p, vp, i64, vp, vp, ctypes.c_int, vp]
            lib.gtmi_reduce_axis_finish_sum.restype = ctypes.c_int
            lib.gtmi_reduce_axis_finish_sum.argtypes = [vp, vp, i64, i64, ctypes.c_int, vp, vp]
            lib.gtmi_reduce_axis_combine.restype = ctypes.c_int
            lib.gtmi_reduce_axis_combine.argtypes = [vp, ctypes.c_int, i64, ctypes.c_int, u32, vp, vp]
            lib.gtmi_reduce_axis_path.restype = ctypes.c_int
            lib.gtmi_reduce_axis_path.argtypes = [desc_p]
            lib.gtmi_reduce_axis_last_error.restype = ctypes.c_char_p
            lib.gtmi_reduce_axis_abi_version.restype = ctypes.c_int
            if lib.gtmi_reduce_axis_abi_version() != 1:
                raise RuntimeError("gtmi_reduce_axis ABI mismatch")
            _lib = lib
        return _lib


def abi_version() -> int:
    """The ABI version the loaded axis library reports."""
    return int(_library().gtmi_reduce_axis_abi_version())


def _check(lib, rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib.gtmi_reduce_axis_last_error().decode()}")


def descriptor(kept, reduced, dt, a_ptr: int, b_ptr: Optional[int]) -> GtmiReduceAxisDesc:
    """The library's descriptor of two canonical groups (lists of ``(extent, sa, sb)``)."""
    if len(kept) > MAX_DIMS or len(reduced) > MAX_DIMS:
        raise ValueError(f"more than {MAX_DIMS} dimensions after merging")
    d = GtmiReduceAxisDesc()
    d.a, d.b = a_ptr, b_ptr
    for i, (e, sa, sb) in enumerate(kept):
        d.k_extent[i], d.k_a_stride[i], d.k_b_stride[i] = e, sa, sb
    for i, (e, sa, sb) in enumerate(reduced):
        d.r_extent[i], d.r_a_stride[i], d.r_b_stride[i] = e, sa, sb
    d.k_ndim, d.r_ndim, d.dtype = len(kept), len(reduced), _r._DTYPE_CODES[np.dtype(dt)]
    return d


def library_path_name(desc: GtmiReduceAxisDesc) -> str:
    """The path the library derives from ``desc`` (the planner's ``path``, from the other side)."""
    lib = _library()
    code = lib.gtmi_reduce_axis_path(ctypes.byref(desc))
    if code < 0:
        raise RuntimeError(f"gtmi_reduce_axis_path failed: {lib.gtmi_reduce_axis_last_error().decode()}")
    return _PATH_CODES[code]


class _AxisPass:
    """One or two device views, the reduced dimensions, the descriptor and the stream."""

    def __init__(self, va, vb, dt, red, stream, parts):
        import torch

        self.torch = torch
        self.va, self.vb, self.dt = va.detach(), (vb.detach() if vb is not None else None), dt
        self.floating = _r._floating(dt)
        self.device = va.device
        self.stream = stream if stream is not None else torch.cuda.current_stream(va.device)
        if vb is not None:
            if tuple(vb.shape) != tuple(va.shape):
                raise ValueError(f"reduce: boxes differ in shape ({tuple(va.shape)}, {tuple(vb.shape)})")
            if vb.device != va.device:
                raise ValueError(f"reduce: tensors on different devices ({va.device}, {vb.device})")
        shape = tuple(va.shape)
        self.kept, self.kshape, self.cells, self.count = _split(shape, red)
        kept, reduced, korder, self.path = _plan(shape, red, va.stride(), vb.stride() if vb is not None else None)
        # cells are numbered in C order over the kept dimensions of extent > 1, slowest stride first
        self._order_shape = [shape[d] for d in korder]
        plain = [d for d in self.kept if shape[d] != 1]
        self._plain_shape = [shape[d] for d in plain]
        self._to_plain = [korder.index(d) for d in plain]
        self._to_order = [plain.index(d) for d in korder]
        self.desc = None
        self.parts = 1
        if self.path is not None:
            self.lib = _library()
            self.desc = descriptor(kept, reduced, dt, self.va.data_ptr(), self.vb.data_ptr() if vb is not None else None)
            with torch.cuda.device(self.device):
                self.parts = int(self.lib.gtmi_reduce_axis_parts(ctypes.byref(self.desc), int(parts or 0)))
            if self.parts < 1:
                raise RuntimeError(f"gtmi_reduce_axis_parts failed: {self.lib.gtmi_reduce_axis_last_error().decode()}")

    def _context(self):
        import contextlib

        stack = contextlib.ExitStack()
        stack.enter_context(self.torch.cuda.device(self.device))
        stack.enter_context(self.torch.cuda.stream(self.stream))  # workspace and results live on the stream
        return stack

    def _empty(self, n):
        return self.torch.empty(n, dtype=self.torch.int64, device=self.device)

    def _workspace(self, slots):
        return self._empty(self.parts * slots * self.cells) if self.parts > 1 else None

    def scan(self, mask: int):
        """The raw scan result: a ``(SCAN_SLOTS, cells)`` int64 tensor; only the slots of ``mask`` are written."""
        with self._context():
            ws, res = self._workspace(_r.SCAN_SLOTS), self._empty(_r.SCAN_SLOTS * self.cells)
            rc = self.lib.gtmi_reduce_axis_scan(ctypes.byref(self.desc), mask, ws.data_ptr() if ws is not None else None,
                                                res.data_ptr(), self.parts, ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_axis_scan")
        return res.view(_r.SCAN_SLOTS, self.cells)

    def folds(self, m, n: int):
        """The raw fold sums, ``(3, cells)`` int64, against the device doubles ``m`` (``cells`` of them, in
        cell order: a raw scan result's first row will do) and ``n``."""
        with self._context():
            ws, res = self._workspace(3), self._empty(3 * self.cells)
            rc = self.lib.gtmi_reduce_axis_folds(ctypes.byref(self.desc), m.data_ptr(), int(n),
                                                 ws.data_ptr() if ws is not None else None, res.data_ptr(), self.parts,
                                                 ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_axis_folds")
        return res.view(3, self.cells)

    def finish(self, scan_raw, folds_raw, n: int):
        """The sums in cell order (f64 / int64)."""
        with self._context():
            out = self._empty(self.cells)
            rc = self.lib.gtmi_reduce_axis_finish_sum(scan_raw.data_ptr(), folds_raw.data_ptr(), self.cells, int(n),
                                                      _r._DTYPE_CODES[self.dt], out.data_ptr(),
                                                      ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_axis_finish_sum")
        return self.values(out)

    def combine(self, records, mask: int):
        """``(nrec, SCAN_SLOTS, cells)`` raw scan results of a partition into one raw scan result."""
        with self._context():
            records = records.contiguous()
            res = self._empty(_r.SCAN_SLOTS * self.cells)
            rc = self.lib.gtmi_reduce_axis_combine(records.data_ptr(), int(records.shape[0]), self.cells,
                                                   _r._DTYPE_CODES[self.dt], mask, res.data_ptr(),
                                                   ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_axis_combine")
        return res.view(_r.SCAN_SLOTS, self.cells)

    def values(self, row):
        """A row of a raw result in the summand type."""
        return row.view(self.torch.float64) if self.floating else row

    def shaped(self, row):
        """Per-cell values in cell order as a dense array of the kept shape."""
        with self._context():
            return row.reshape(self._order_shape).permute(self._to_plain).contiguous().reshape(self.kshape)

    def cell_order(self, arr):
        """An array over the kept shape as a contiguous f64 vector in cell order."""
        torch = self.torch
        with self._context():
            t = torch.as_tensor(arr).to(device=self.device, dtype=torch.float64)
            if tuple(t.shape) != tuple(self.kshape):
                t = t.broadcast_to(self.kshape)
            return t.reshape(self._plain_shape).permute(self._to_order).contiguous().reshape(-1)

    def full(self, value, torch_dtype):
        with self._context():
            return self.torch.full(self.kshape, value, dtype=torch_dtype, device=self.device)


# ---------------------------------------------------------------------------------------------
# what the public functions of storage.reduce call
# ---------------------------------------------------------------------------------------------
class _Prepared:
    """Host summands or a device pass for ``(arr, b, reduced axes, box)``."""

    def __init__(self, arr, b, red, origin, domain, stream, parts):
        va, vb, self.dt = _r._boxes(arr, b, origin, domain)
        self.floating = _r._floating(self.dt)
        self.p = None
        if isinstance(va, np.ndarray):
            self.kshape, self.x = _summands_host(va, vb, self.dt, red)
            self.cells, self.count = self.x.shape
        else:
            self.p = _AxisPass(va, vb, self.dt, red, stream, parts)
            self.kshape, self.cells, self.count = self.p.kshape, self.p.cells, self.p.count

    @property
    def launches(self) -> bool:
        return self.p is not None and self.cells > 0 and self.count > 0

    def constant(self, value, np_dtype):
        """An array of the kept shape filled with ``value`` (no launch)."""
        if self.p is None:
            return np.full(self.kshape, value, dtype=np_dtype)
        from gt4py_amd import storage

        return self.p.full(value, storage.torch_dtype(np.dtype(np_dtype)))


def scan(arr, b, red, origin, domain, stream, parts):
    q = _Prepared(arr, b, red, origin, domain, stream, parts)
    if q.p is None:
        return (*(v.reshape(q.kshape) for v in _scan_host(q.x)), q.count)
    if not q.launches:
        raise ValueError("reduce: scan of an empty box on the device")
    raw = q.p.scan(MASK_BASE)
    return (*(q.p.shaped(q.p.values(raw[k])) for k in range(3)), *(q.p.shaped(raw[k]) for k in (3, 4, 5)), q.count)


def fold_sums(arr, b, M, N, red, origin, domain, stream, parts):
    q = _Prepared(arr, b, red, origin, domain, stream, parts)
    st = np.float64 if q.floating else np.int64
    if q.p is None:
        M = np.broadcast_to(np.asarray(_r._host_array(M), dtype=np.float64), q.kshape).reshape(-1)
        return tuple(v.reshape(q.kshape) for v in _fold_sums_host(q.x, M, int(N)))
    if not q.launches:
        return tuple(q.constant(0, st) for _ in range(3))
    raw = q.p.folds(q.p.cell_order(M), int(N))
    return tuple(q.p.shaped(q.p.values(raw[k])) for k in range(3))


def sum_(arr, b, red, origin, domain, stream, parts):
    q = _Prepared(arr, b, red, origin, domain, stream, parts)
    st = np.float64 if q.floating else np.int64
    if q.cells == 0 or q.count == 0:  # an empty reduced extent: 0; an empty kept extent: an empty array
        return q.constant(0, st)
    if q.p is None:
        sc = _scan_host(q.x)
        return _finish_sum_host(sc, _fold_sums_host(q.x, sc[0], q.count), q.count, q.floating).reshape(q.kshape)
    raw = q.p.scan(MASK_SUM)  # M stays on the device: row 0 of the scan result
    return q.p.shaped(q.p.finish(raw, q.p.folds(raw, q.count), q.count))


def norm2(a, red, origin, domain, stream, parts):
    d = sum_(a, a, red, origin, domain, stream, parts)
    if isinstance(d, np.ndarray):
        with np.errstate(all="ignore"):
            return np.sqrt(d.astype(np.float64))
    import torch

    return torch.sqrt(d.to(torch.float64))


def count_nonfinite(arr, red, origin, domain, stream, parts):
    q = _Prepared(arr, None, red, origin, domain, stream, parts)
    if q.cells == 0 or q.count == 0:
        return q.constant(0, np.int64)
    if q.p is None:
        sc = _scan_host(q.x)
        return (sc[3] + sc[4] + sc[5]).astype(np.int64).reshape(q.kshape)
    return q.p.shaped(q.p.scan(MASK_NONFINITE)[6])


def extremum(arr, which, red, origin, domain, stream, parts):
    q = _Prepared(arr, None, red, origin, domain, stream, parts)
    out_dt = np.dtype(np.int64) if (which == 0 and not q.floating) else q.dt  # absmax of ints: int64
    if q.count == 0:
        raise ValueError(f"zero-size reduced extent to reduction operation {('absmax', 'min', 'max')[which]} which has no identity")
    if q.cells == 0:
        return q.constant(0, out_dt)
    if q.p is None:
        sc = _scan_host(q.x)
        v = sc[which].astype(out_dt)
        if q.floating:
            v = np.where(sc[3] > 0, out_dt.type(np.nan), v)
        return v.reshape(q.kshape)
    from gt4py_amd import storage

    row = q.p.values(q.p.scan(1 << (8 + which))[8 + which])
    return q.p.shaped(row.to(storage.torch_dtype(out_dt)))


__all__ = ["plan_axis", "normalize_axis", "library_path", "abi_version", "SEGMENT", "LANE", "GENERIC"]
