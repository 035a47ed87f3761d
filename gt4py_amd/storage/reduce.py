"""Reductions over the compute domain of a storage, bit-reproducible
(``include/gtmi_reduce.h``, ``csrc/gtmi_reduce.hip``).

Every function takes ``(arr, *, origin=None, domain=None)``: ``arr`` is a storage or any strided
array / tensor of at most 8 dimensions, ``origin`` and ``domain`` select a box as in a stencil
call (default: the whole array); cells outside the box are never read. The numpy code in this
module is the definition of every result and the execution path of host arrays; device tensors
go through the reduction library, which reproduces the same bits whatever its grid size, its
traversal order or the partition of the domain.

Summands are f64 for f32 / f64 arrays (``dot``: one f64 multiply per cell, exact for f32) and
int64 with wrap-around for int32 / int64 arrays.

**Float sum rule.** ``N`` summands with absolute maximum ``M`` (over the non-NaN ones). Any NaN
-> NaN; +Inf and -Inf -> NaN; Inf of one sign -> that Inf; ``M == 0`` -> ``+0.0``. Otherwise
``M = m * 2**e`` with ``m`` in [0.5, 1), ``L = max(1, ceil(log2 N))``, ``E_0 = e + L`` and for
the folds ``f = 0, 1, 2``: ``C = 1.5 * 2**E_f``, ``q = (r + C) - C``, ``S_f += q``, ``r -= q``,
``E_{f+1} = E_f - 52 + L``; the result is ``S_0 + (S_1 + S_2)``. Every ``q`` of a fold is a
multiple of ``2**(E_f - 52)`` and every partial sum stays below ``2**(E_f + 1)``, so each ``S_f``
is exact in f64 in any order: the result depends on the multiset of summands and ``(M, N)`` only.

At the ends of the exponent range (``fold_plan``): with ``E_0 > 1022`` every summand is first
multiplied by ``2**(1022 - E_0)`` (a factor that depends on ``(e, L)`` only; the folds run with
``E_0 = 1022`` and the result is multiplied by ``2**(E_0 - 1022)``, overflowing to Inf where the
sum does); a fold with ``E_f < -1022``, whose grid ``2**(E_f - 52)`` lies below the smallest
subnormal, takes ``q = r``: all its summands are multiples of ``2**-1074`` below ``2**-1022 / N``,
and their sums are exact as well.

The library is built once with hipcc into the in-tree cache and loaded through ctypes after
torch, exactly as ``storage/relayout.py`` does.
"""

from __future__ import annotations

import builtins
import ctypes
import hashlib
import math
import os
import threading
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from gt4py_amd.runtime import jit

_SRC = os.path.join(jit.CSRC_DIR, "gtmi_reduce.hip")
_HEADER = os.path.join(jit.INCLUDE_DIR, "gtmi_reduce.h")
_RULES = os.path.join(jit.CSRC_DIR, "gtmi_reduce_rules.h")  # shared with gtmi_reduce_axis.hip
_lock = threading.Lock()
_lib = None

MAX_DIMS = 8  # GTMI_REDUCE_MAX_DIMS
SHORT_ROW = 32  # GTMI_REDUCE_SHORT_ROW
SCAN_SLOTS, FOLD_SLOTS = 12, 4  # GTMI_REDUCE_SCAN_SLOTS, GTMI_REDUCE_FOLD_SLOTS
ROW, GENERIC = "ROW", "GENERIC"
_PATH_CODES = {0: ROW, 1: GENERIC}
_DTYPE_CODES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}


class GtmiReduceDesc(ctypes.Structure):
    _fields_ = [
        ("a", ctypes.c_void_p),
        ("b", ctypes.c_void_p),
        ("extent", ctypes.c_int64 * MAX_DIMS),
        ("a_stride", ctypes.c_int64 * MAX_DIMS),
        ("b_stride", ctypes.c_int64 * MAX_DIMS),
        ("ndim", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
    ]


# ---------------------------------------------------------------------------------------------
# the box
# ---------------------------------------------------------------------------------------------
def _normalize_box(shape: Sequence[int], origin, domain) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    shape = tuple(int(s) for s in shape)
    ndim = len(shape)
    if ndim > MAX_DIMS:
        raise ValueError(f"reduce: arrays of more than {MAX_DIMS} dimensions are not supported (got {ndim})")
    if origin is None:
        origin = (0,) * ndim
    try:
        origin = tuple(int(o) for o in origin)
    except Exception as ex:
        raise ValueError("Invalid 'origin' value ({})".format(origin)) from ex
    if len(origin) != ndim:
        raise ValueError("Invalid 'origin' value ({})".format(origin))
    if any(o < 0 for o in origin):
        raise ValueError(f"Origin too small. Must be at least {(0,) * ndim}, is {origin}")
    if domain is None:
        domain = tuple(builtins.max(s - o, 0) for s, o in zip(shape, origin))
    try:
        domain = tuple(int(d) for d in domain)
    except Exception as ex:
        raise ValueError("Invalid 'domain' value ({})".format(domain)) from ex
    if len(domain) != ndim or any(d < 0 for d in domain):
        raise ValueError(f"Invalid 'domain' value '{domain}'")
    room = tuple(s - o for s, o in zip(shape, origin))
    if any(d > r for d, r in zip(domain, room)):
        raise ValueError(
            f"Compute domain too large for reduce: \n"
            f"  Domain is {domain} but the array of shape {shape} holds {room} cells from origin {origin}."
        )
    return origin, domain


def _is_device(obj) -> bool:
    from gt4py_amd import storage

    return storage._is_device_data(obj)


def _host_array(obj) -> np.ndarray:
    if isinstance(obj, np.ndarray):
        return obj
    if hasattr(obj, "detach") and hasattr(obj, "numpy"):
        return obj.detach().numpy()
    return np.asarray(obj)


def _box(arr, origin, domain):
    """The box of ``arr`` as a view (numpy for host arrays, torch for device tensors)."""
    if _is_device(arr):
        from gt4py_amd import storage

        arr = storage._as_device_tensor(arr)
    else:
        arr = _host_array(arr)
    origin, domain = _normalize_box(arr.shape, origin, domain)
    return arr[tuple(slice(o, o + d) for o, d in zip(origin, domain))]


def _np_dtype(view) -> np.dtype:
    from gt4py_amd import storage

    try:
        dt = storage.numpy_dtype_of(view)
    except KeyError:
        raise ValueError(f"reduce: unsupported dtype {view.dtype}") from None
    if dt not in _DTYPE_CODES:
        raise ValueError(f"reduce: unsupported dtype {dt} (float32, float64, int32 and int64 are)")
    return dt


def _boxes(a, b, origin, domain):
    va = _box(a, origin, domain)
    dt = _np_dtype(va)
    if b is None:
        return va, None, dt
    vb = _box(b, origin, domain)
    if _np_dtype(vb) != dt:
        raise ValueError(f"reduce: dtypes differ ({dt}, {_np_dtype(vb)})")
    if isinstance(va, np.ndarray) != isinstance(vb, np.ndarray):
        raise ValueError("reduce: one array is on the host and the other on the device")
    return va, vb, dt


def _floating(dt: np.dtype) -> bool:
    return dt.kind == "f"


# ---------------------------------------------------------------------------------------------
# the restatement (host arrays)
# ---------------------------------------------------------------------------------------------
class FoldPlan(NamedTuple):
    """Constants of the three folds for ``(M, N)``; ``E`` are the fold exponents after scaling."""

    zero: bool  # M is 0 or not finite: every fold sum is 0
    scale: float
    unscale: float
    c: Tuple[float, float, float]
    ident: Tuple[bool, bool, bool]  # the fold takes q = r
    E: Tuple[int, int, int]
    L: int


def ceil_log2(n: int) -> int:
    """``L = max(1, ceil(log2 n))``."""
    n = int(n)
    return builtins.max(1, (n - 1).bit_length() if n > 0 else 0)


def fold_plan(M: float, N: int) -> FoldPlan:
    M = float(M)
    L = ceil_log2(N)
    if not (M > 0.0) or math.isinf(M):
        return FoldPlan(True, 1.0, 1.0, (0.0, 0.0, 0.0), (False, False, False), (0, 0, 0), L)
    e = math.frexp(M)[1]  # M = m * 2**e, m in [0.5, 1)
    E = e + L
    scale = unscale = 1.0
    if E > 1022:  # huge M: scale the summands by 2**(1022 - E0), exactly
        scale, unscale = math.ldexp(1.0, 1022 - E), math.ldexp(1.0, E - 1022)
        E = 1022
    c: List[float] = []
    ident: List[bool] = []
    Es: List[int] = []
    for _ in range(3):
        Es.append(E)
        if E < -1022:
            ident.append(True)
            c.append(0.0)
        else:
            ident.append(False)
            c.append(math.ldexp(1.5, E))
        E = E - 52 + L
    return FoldPlan(False, scale, unscale, tuple(c), tuple(ident), tuple(Es), L)


def _summands_host(va: np.ndarray, vb: Optional[np.ndarray], dt: np.dtype) -> np.ndarray:
    """The box's summands as a flat f64 / int64 array (a copy: only the box's cells are read)."""
    st = np.float64 if _floating(dt) else np.int64
    x = np.array(va, dtype=st, order="C").reshape(-1)
    if vb is not None:
        if tuple(vb.shape) != tuple(va.shape):
            raise ValueError(f"reduce: boxes differ in shape ({tuple(va.shape)}, {tuple(vb.shape)})")
        with np.errstate(all="ignore"):
            x = x * np.array(vb, dtype=st, order="C").reshape(-1)  # one multiply per cell; int64 wraps
    return x


def _scan_host(x: np.ndarray):
    """``(absmax, min, max, n_nan, n_pinf, n_ninf, count)`` of flat summands. NaNs are counted and
    otherwise left out; -0.0 orders below +0.0; identities where nothing is left."""
    count = int(x.size)
    if x.dtype.kind == "f":
        nan = np.isnan(x)
        v = x[~nan]
        n_nan = np.int64(np.count_nonzero(nan))
        n_pinf = np.int64(np.count_nonzero(v == np.inf))
        n_ninf = np.int64(np.count_nonzero(v == -np.inf))
        if v.size == 0:
            return np.float64(0.0), np.float64(np.inf), np.float64(-np.inf), n_nan, n_pinf, n_ninf, count
        absmax, mn, mx = np.abs(v).max(), v.min(), v.max()
        zeros = v[v == 0]
        if mn == 0:
            mn = np.float64(-0.0) if np.signbit(zeros).any() else np.float64(0.0)
        if mx == 0:
            mx = np.float64(0.0) if (~np.signbit(zeros)).any() else np.float64(-0.0)
        return np.float64(absmax), np.float64(mn), np.float64(mx), n_nan, n_pinf, n_ninf, count
    z = np.int64(0)
    if count == 0:
        i = np.iinfo(np.int64)
        return np.int64(i.min), np.int64(i.max), np.int64(i.min), z, z, z, count
    return np.int64(np.abs(x).max()), np.int64(x.min()), np.int64(x.max()), z, z, z, count


def _combine_scans_host(parts):
    """Scan results of the parts of a partitioned domain into one, by the rules of the scan."""
    parts = list(parts)
    floating = isinstance(parts[0][0], (float, np.floating))
    vals = np.array([v for p in parts for v in p[:3]], dtype=np.float64 if floating else np.int64).reshape(-1, 3)
    absmax = vals[:, 0].max()
    mn, mx = vals[:, 1].min(), vals[:, 2].max()
    if floating:
        if mn == 0 and np.signbit(vals[:, 1][vals[:, 1] == 0]).any():
            mn = np.float64(-0.0)
        elif mn == 0:
            mn = np.float64(0.0)
        if mx == 0 and (~np.signbit(vals[:, 2][vals[:, 2] == 0])).any():
            mx = np.float64(0.0)
        elif mx == 0:
            mx = np.float64(-0.0)
    cast = np.float64 if floating else np.int64
    counts = [np.int64(builtins.sum(int(p[k]) for p in parts)) for k in (3, 4, 5)]
    return (cast(absmax), cast(mn), cast(mx), *counts, builtins.sum(int(p[6]) for p in parts))


def _fold_sums_host(x: np.ndarray, M, N: int):
    """The three fold sums of flat summands against ``(M, N)``. Non-finite summands count as 0."""
    if x.dtype.kind != "f":
        return np.sum(x, dtype=np.int64), np.int64(0), np.int64(0)
    p = fold_plan(M, N)
    z = np.float64(0.0)
    if p.zero:
        return z, z, z
    with np.errstate(all="ignore"):
        r = np.where(np.isfinite(x), x, 0.0) * p.scale
        out = []
        for f in range(3):
            q = r if p.ident[f] else (r + p.c[f]) - p.c[f]
            out.append(np.float64(np.sum(q) + 0.0))  # exact in any order; + 0.0: never -0.0
            r = r - q
    return tuple(out)


def _finish_sum_host(sc, folds, N: int, floating: bool):
    if not floating:
        return np.int64(folds[0])
    absmax, _, _, n_nan, n_pinf, n_ninf = sc[:6]
    if n_nan > 0 or (n_pinf > 0 and n_ninf > 0):
        return np.float64(np.nan)
    if n_pinf > 0:
        return np.float64(np.inf)
    if n_ninf > 0:
        return np.float64(-np.inf)
    if absmax == 0:
        return np.float64(0.0)
    with np.errstate(all="ignore"):
        return np.float64((folds[0] + (folds[1] + folds[2])) * np.float64(fold_plan(absmax, N).unscale))


# ---------------------------------------------------------------------------------------------
# the library (device tensors)
# ---------------------------------------------------------------------------------------------
def plan(shape: Sequence[int], a_strides: Sequence[int], b_strides: Optional[Sequence[int]] = None):
    """Canonical ``(extent, a_strides, b_strides, path)`` of a box of ``shape`` read from one or two
    sources with the given element strides: extent-1 dimensions dropped, dimensions ordered by the
    first source's stride (slowest first), neighbours that are contiguous in every source merged.
    ``path`` is ROW, GENERIC, or None for an empty box. Pure Python."""
    shape = tuple(int(e) for e in shape)
    a_strides = tuple(int(s) for s in a_strides)
    two = b_strides is not None
    b_strides = tuple(int(s) for s in b_strides) if two else (0,) * len(shape)
    if not (len(shape) == len(a_strides) == len(b_strides)):
        raise ValueError("shape and strides have different lengths")
    if any(e < 0 for e in shape):
        raise ValueError(f"negative extent in {shape}")
    if any(e == 0 for e in shape):
        return (), (), (), None
    dims = [(e, sa, sb) for e, sa, sb in zip(shape, a_strides, b_strides) if e != 1]
    if any(sa < 0 or sb < 0 for _, sa, sb in dims):
        raise ValueError("negative strides are not supported")
    dims.sort(key=lambda t: -t[1])
    merged: List[Tuple[int, int, int]] = []
    for e, sa, sb in dims:
        if merged:
            pe, psa, psb = merged[-1]
            if psa == sa * e and (not two or psb == sb * e):
                merged[-1] = (pe * e, sa, sb)
                continue
        merged.append((e, sa, sb))
    if not merged:
        merged = [(1, 1, 1)]  # a single element
    if len(merged) > MAX_DIMS:
        raise ValueError(f"more than {MAX_DIMS} dimensions after merging")
    extent = tuple(t[0] for t in merged)
    sa = tuple(t[1] for t in merged)
    sb = tuple(t[2] for t in merged)
    row = sa[-1] == 1 and (not two or sb[-1] == 1) and extent[-1] >= SHORT_ROW
    return extent, sa, sb, ROW if row else GENERIC


def library_path() -> str:
    with open(_SRC) as f:
        source = f.read()
    h = hashlib.sha256()
    for path in (_HEADER, _RULES):  # not among jit's hashed headers: make them part of this key
        with open(path, "rb") as f:
            h.update(f.read())
    return jit.compile_source(source, extra_flags=[f"-DGTMI_REDUCE_HEADER_DIGEST=0x{h.hexdigest()[:16]}"])


def _library():
    global _lib
    with _lock:
        if _lib is None:
            import torch  # noqa: F401  (bind to torch's HIP runtime first)

            lib = ctypes.CDLL(library_path(), mode=ctypes.RTLD_LOCAL)
            desc_p, vp = ctypes.POINTER(GtmiReduceDesc), ctypes.c_void_p
            lib.gtmi_reduce_blocks.restype = ctypes.c_int
            lib.gtmi_reduce_blocks.argtypes = [desc_p, ctypes.c_int]
            lib.gtmi_reduce_scan.restype = ctypes.c_int
            lib.gtmi_reduce_scan.argtypes = [desc_p, vp, vp, ctypes.c_int, vp]
            lib.gtmi_reduce_folds.restype = ctypes.c_int
            lib.gtmi_reduce_folds.argtypes = [desc_p, vp, ctypes.c_int64, vp, vp, ctypes.c_int, vp]
            lib.gtmi_reduce_finish_sum.restype = ctypes.c_int
            lib.gtmi_reduce_finish_sum.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp]
            lib.gtmi_reduce_combine.restype = ctypes.c_int
            lib.gtmi_reduce_combine.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp]
            lib.gtmi_reduce_path.restype = ctypes.c_int
            lib.gtmi_reduce_path.argtypes = [desc_p]
            lib.gtmi_reduce_last_error.restype = ctypes.c_char_p
            lib.gtmi_reduce_abi_version.restype = ctypes.c_int
            if lib.gtmi_reduce_abi_version() != 1:
                raise RuntimeError("gtmi_reduce ABI mismatch")
            _lib = lib
        return _lib


def abi_version() -> int:
    """The ABI version the loaded library reports."""
    return int(_library().gtmi_reduce_abi_version())


def _check(lib, rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib.gtmi_reduce_last_error().decode()}")


def _descriptor(va, vb, dt: np.dtype) -> Optional[GtmiReduceDesc]:
    """The canonical descriptor of one or two device views; None for an empty box."""
    if vb is not None:
        if tuple(vb.shape) != tuple(va.shape):
            raise ValueError(f"reduce: boxes differ in shape ({tuple(va.shape)}, {tuple(vb.shape)})")
        if vb.device != va.device:
            raise ValueError(f"reduce: tensors on different devices ({va.device}, {vb.device})")
    extent, sa, sb, path = plan(va.shape, va.stride(), vb.stride() if vb is not None else None)
    if path is None:
        return None
    d = GtmiReduceDesc()
    d.a = va.data_ptr()
    d.b = vb.data_ptr() if vb is not None else None
    n = len(extent)
    d.extent[:n] = extent
    d.a_stride[:n] = sa
    d.b_stride[:n] = sb
    d.ndim, d.dtype = n, _DTYPE_CODES[dt]
    return d


class _DevicePass:
    """One or two device views, their descriptor and the stream the launches go to."""

    def __init__(self, va, vb, dt, stream, blocks):
        import torch

        self.torch = torch
        self.va, self.vb, self.dt = va.detach(), (vb.detach() if vb is not None else None), dt
        self.device = va.device
        self.stream = stream if stream is not None else torch.cuda.current_stream(va.device)
        self.count = int(np.prod(va.shape, dtype=object)) if len(va.shape) else 1
        self.lib = _library()
        self.desc = _descriptor(self.va, self.vb, dt)
        self.blocks = 1
        if self.desc is not None:
            with torch.cuda.device(self.device):
                self.blocks = int(self.lib.gtmi_reduce_blocks(ctypes.byref(self.desc), int(blocks or 0)))
            if self.blocks < 1:
                raise RuntimeError(f"gtmi_reduce_blocks failed: {self.lib.gtmi_reduce_last_error().decode()}")

    def _context(self):
        import contextlib

        stack = contextlib.ExitStack()
        stack.enter_context(self.torch.cuda.device(self.device))
        stack.enter_context(self.torch.cuda.stream(self.stream))  # workspace and results live on the stream
        return stack

    def _empty(self, n):
        return self.torch.empty(n, dtype=self.torch.int64, device=self.device)

    def scan(self):
        """The raw scan result (``SCAN_SLOTS`` int64 slots on the device)."""
        if self.desc is None:
            raise ValueError("reduce: scan of an empty box on the device")
        with self._context():
            ws, res = self._empty(self.blocks * SCAN_SLOTS), self._empty(SCAN_SLOTS)
            rc = self.lib.gtmi_reduce_scan(ctypes.byref(self.desc), ws.data_ptr(), res.data_ptr(), self.blocks,
                                           ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_scan")
        return res

    def folds(self, m, n: int):
        """The raw fold sums (``FOLD_SLOTS`` int64 slots) against the device double ``m`` and ``n``."""
        with self._context():
            res = self._empty(FOLD_SLOTS)
            if self.desc is None:
                return res.zero_()
            ws = self._empty(self.blocks * FOLD_SLOTS)
            rc = self.lib.gtmi_reduce_folds(ctypes.byref(self.desc), m.data_ptr(), int(n), ws.data_ptr(), res.data_ptr(),
                                            self.blocks, ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_folds")
        return res

    def finish(self, scan_raw, folds_raw, n: int):
        """The sum as a 0-d device tensor (f64 / int64)."""
        with self._context():
            out = self._empty(1)
            rc = self.lib.gtmi_reduce_finish_sum(scan_raw.data_ptr(), folds_raw.data_ptr(), int(n), _DTYPE_CODES[self.dt],
                                                 out.data_ptr(), ctypes.c_void_p(self.stream.cuda_stream))
            _check(self.lib, rc, "gtmi_reduce_finish_sum")
        return self.slot(out, 0)

    def slot(self, raw, k: int):
        """Slot ``k`` of a raw result as a 0-d tensor of the summand type."""
        s = raw[k : k + 1]
        if _floating(self.dt):
            s = s.view(self.torch.float64)
        return s.reshape(())

    def count_slot(self, raw, k: int):
        return raw[k : k + 1].reshape(())


def combine_scans_device(records, dt, stream=None):
    """Raw scan results of the parts of a partitioned domain (a ``(parts, SCAN_SLOTS)`` int64 device
    tensor) into one raw scan result, by the rules of the scan."""
    import torch

    records = records.contiguous()
    lib = _library()
    s = stream if stream is not None else torch.cuda.current_stream(records.device)
    with torch.cuda.device(records.device), torch.cuda.stream(s):
        res = torch.empty(SCAN_SLOTS, dtype=torch.int64, device=records.device)
        rc = lib.gtmi_reduce_combine(records.data_ptr(), int(records.shape[0]), _DTYPE_CODES[np.dtype(dt)], res.data_ptr(),
                                     ctypes.c_void_p(s.cuda_stream))
        _check(lib, rc, "gtmi_reduce_combine")
    return res


def _device_m(p: _DevicePass, M):
    """``M`` as one f64 in device memory (unused by the integer folds)."""
    torch = p.torch
    with p._context():
        if hasattr(M, "is_cuda"):
            return M.detach().to(device=p.device, dtype=torch.float64).reshape(1).contiguous()
        return torch.tensor([float(M) if _floating(p.dt) else 0.0], dtype=torch.float64, device=p.device)


# ---------------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------------
def _prepare(arr, b, origin, domain, stream, blocks):
    """``(host summands | None, device pass | None, dtype)``."""
    va, vb, dt = _boxes(arr, b, origin, domain)
    if isinstance(va, np.ndarray):
        return _summands_host(va, vb, dt), None, dt
    return None, _DevicePass(va, vb, dt, stream, blocks), dt


def _axes(arr, axis):
    """The reduced dimensions for ``axis=``; None for the scalar path (``axis=None``, or every
    dimension listed: a 0-d result with the same bits)."""
    if axis is None:
        return None
    from gt4py_amd.storage import reduce_axis

    return reduce_axis.reduced_axes(arr, axis)


def scan(arr, b=None, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """``(absmax, min, max, n_nan, n_pinf, n_ninf, count)`` of the box's summands (the products
    with ``b``'s box when ``b`` is given), in the summand type (f64 / int64). NaNs are counted and
    otherwise left out, -0.0 orders below +0.0; where nothing is left ``absmax`` is 0 (ints:
    INT64_MIN), ``min`` +inf (INT64_MAX) and ``max`` -inf (INT64_MIN). ``count`` is a Python int;
    for device tensors the other six are 0-d device tensors and an empty box raises. With ``axis=``
    the six are arrays over the kept cells and ``count`` is the reduced count of every cell."""
    red = _axes(arr, axis)
    if red is not None:
        from gt4py_amd.storage import reduce_axis

        return reduce_axis.scan(arr, b, red, origin, domain, stream, _parts)
    x, p, _ = _prepare(arr, b, origin, domain, stream, _blocks)
    if p is None:
        return _scan_host(x)
    raw = p.scan()
    return (p.slot(raw, 0), p.slot(raw, 1), p.slot(raw, 2), p.count_slot(raw, 3), p.count_slot(raw, 4),
            p.count_slot(raw, 5), p.count)


def fold_sums(arr, *args, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """``fold_sums(arr[, b], M, N) -> (S0, S1, S2)``: the fold sums of the box's summands against
    the absolute maximum ``M`` and the count ``N`` of a reduction that may cover more than this
    box (a partition: the parts' fold sums add exactly). Non-finite summands count as 0; integer
    arrays give ``(wrap-around sum, 0, 0)``. ``M`` may be a device scalar. With ``axis=`` ``M`` is an
    array over the kept cells (host or device) and so are the three sums."""
    if len(args) == 2:
        b, (M, N) = None, args
    elif len(args) == 3:
        b, M, N = args
    else:
        raise TypeError("fold_sums(arr[, b], M, N)")
    red = _axes(arr, axis)
    if red is not None:
        from gt4py_amd.storage import reduce_axis

        return reduce_axis.fold_sums(arr, b, M, N, red, origin, domain, stream, _parts)
    x, p, _ = _prepare(arr, b, origin, domain, stream, _blocks)
    if p is None:
        return _fold_sums_host(x, M, int(N))
    raw = p.folds(_device_m(p, M), int(N))
    return p.slot(raw, 0), p.slot(raw, 1), p.slot(raw, 2)


def _sum(arr, b, origin, domain, stream, blocks, axis=None, parts=None):
    red = _axes(arr, axis)
    if red is not None:
        from gt4py_amd.storage import reduce_axis

        return reduce_axis.sum_(arr, b, red, origin, domain, stream, parts)
    x, p, dt = _prepare(arr, b, origin, domain, stream, blocks)
    if p is None:
        sc = _scan_host(x)
        return _finish_sum_host(sc, _fold_sums_host(x, sc[0], x.size), x.size, _floating(dt))
    if p.desc is None:  # an empty box: 0
        with p._context():
            return p.torch.zeros((), dtype=p.torch.float64 if _floating(dt) else p.torch.int64, device=p.device)
    raw = p.scan()  # M stays on the device: slot 0 of the scan result
    return p.finish(raw, p.folds(raw, p.count), p.count)


def sum(arr, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):  # noqa: A001
    """Sum of the box: f64 for f32 / f64 arrays (the float sum rule), int64 with wrap-around for
    int32 / int64 arrays; 0 for an empty box. ``axis`` (an int or a tuple of ints, here and in the
    functions below) reduces those dimensions only: one result per cell of the others, each with
    the bits of this function on the cell's sub-box (``storage/reduce_axis.py``)."""
    return _sum(arr, None, origin, domain, stream, _blocks, axis, _parts)


def dot(a, b, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """Sum of ``a[i] * b[i]`` over the same box of two arrays of equal dtype, as ``sum`` of the
    products (one f64 multiply each for f32 / f64, int64 with wrap-around for integers)."""
    return _sum(a, b, origin, domain, stream, _blocks, axis, _parts)


def norm2(a, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """``sqrt(dot(a, a))`` in f64."""
    d = _sum(a, a, origin, domain, stream, _blocks, axis, _parts)
    if isinstance(d, (np.generic, np.ndarray)):
        with np.errstate(all="ignore"):
            return np.sqrt(np.asarray(d, dtype=np.float64))
    import torch

    return torch.sqrt(d.to(torch.float64))


def count_nonfinite(arr, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """int64 count of NaN / +Inf / -Inf cells of the box (0 for integer arrays and empty boxes)."""
    red = _axes(arr, axis)
    if red is not None:
        from gt4py_amd.storage import reduce_axis

        return reduce_axis.count_nonfinite(arr, red, origin, domain, stream, _parts)
    x, p, _ = _prepare(arr, None, origin, domain, stream, _blocks)
    if p is None:
        sc = _scan_host(x)
        return np.int64(sc[3] + sc[4] + sc[5])
    if p.desc is None:
        with p._context():
            return p.torch.zeros((), dtype=p.torch.int64, device=p.device)
    return p.count_slot(p.scan(), 6)


def _extremum(arr, which, origin, domain, stream, blocks, axis=None, parts=None):
    red = _axes(arr, axis)
    if red is not None:
        from gt4py_amd.storage import reduce_axis

        return reduce_axis.extremum(arr, which, red, origin, domain, stream, parts)
    x, p, dt = _prepare(arr, None, origin, domain, stream, blocks)
    out_dt = np.dtype(np.int64) if (which == 0 and not _floating(dt)) else dt  # absmax of ints: int64
    count = x.size if p is None else p.count
    if count == 0:
        raise ValueError(f"zero-size box to reduction operation {('absmax', 'min', 'max')[which]} which has no identity")
    if p is None:
        sc = _scan_host(x)
        if sc[3] > 0:
            return out_dt.type(np.nan)
        return out_dt.type(sc[which])
    from gt4py_amd import storage

    return p.slot(p.scan(), 8 + which).to(storage.torch_dtype(out_dt))


def min(arr, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):  # noqa: A001
    """Minimum of the box in the array's dtype: NaN when any cell is (as ``np.min``), -0.0 below
    +0.0; ``ValueError`` for an empty box."""
    return _extremum(arr, 1, origin, domain, stream, _blocks, axis, _parts)


def max(arr, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):  # noqa: A001
    """Maximum of the box, as ``min``."""
    return _extremum(arr, 2, origin, domain, stream, _blocks, axis, _parts)


def absmax(arr, *, axis=None, origin=None, domain=None, stream=None, _blocks=None, _parts=None):
    """Maximum of ``|x|`` over the box: the array's dtype for floats (NaN when any cell is),
    int64 for integers (computed in int64); ``ValueError`` for an empty box."""
    return _extremum(arr, 0, origin, domain, stream, _blocks, axis, _parts)


def plan_axis(shape, axis, a_strides, b_strides=None):
    """``storage.reduce_axis.plan_axis``: the canonical kept and reduced groups and the path."""
    from gt4py_amd.storage import reduce_axis

    return reduce_axis.plan_axis(shape, axis, a_strides, b_strides)


__all__ = ["count_nonfinite", "min", "max", "absmax", "sum", "dot", "norm2", "scan", "fold_sums", "fold_plan",
           "ceil_log2", "plan", "plan_axis", "library_path", "abi_version", "combine_scans_device"]
