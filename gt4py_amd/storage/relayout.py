"""Device-side relayout of storages (``include/gtmi_relayout.h``, ``csrc/gtmi_relayout.hip``).

``plan`` turns two strided views of one shape into the canonical descriptor the library takes:
extent-1 dimensions dropped, neighbouring dimensions that are contiguous on both sides merged,
dimensions ordered by the destination's stride (slowest first), and names the copy path. It is
pure Python, so it is tested without a device. ``copy`` launches one kernel on a stream.

The library is built once with hipcc into the in-tree cache like the stencil libraries
(``runtime/jit.py``) and loaded through ctypes after torch (same HIP runtime), exactly as
``distributed/halo_copy.py`` does.
"""

from __future__ import annotations

import ctypes
import hashlib
import os
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from gt4py_amd.runtime import jit

_SRC = os.path.join(jit.CSRC_DIR, "gtmi_relayout.hip")
_HEADER = os.path.join(jit.INCLUDE_DIR, "gtmi_relayout.h")
_lock = threading.Lock()
_lib = None

MAX_DIMS = 8  # GTMI_RELAYOUT_MAX_DIMS
TILE_MIN = 16  # GTMI_RELAYOUT_TILE_MIN
ROW, TILE, GENERIC = "ROW", "TILE", "GENERIC"
_PATH_CODES = {0: ROW, 1: TILE, 2: GENERIC}


class GtmiRelayoutDesc(ctypes.Structure):
    _fields_ = [
        ("src", ctypes.c_void_p),
        ("dst", ctypes.c_void_p),
        ("extent", ctypes.c_int64 * MAX_DIMS),
        ("src_stride", ctypes.c_int64 * MAX_DIMS),
        ("dst_stride", ctypes.c_int64 * MAX_DIMS),
        ("ndim", ctypes.c_int32),
        ("itemsize", ctypes.c_int32),
    ]


@dataclass
class RelayoutPlan:
    """Canonical form of one copy. ``path`` is ROW, TILE or GENERIC (None for an empty box);
    ``a`` / ``b`` index the canonical dimensions with source / destination stride 1 on the TILE
    path (``a == b`` on ROW, both None on GENERIC)."""

    extent: Tuple[int, ...]
    src_strides: Tuple[int, ...]
    dst_strides: Tuple[int, ...]
    itemsize: int
    path: Optional[str]
    a: Optional[int]
    b: Optional[int]

    @property
    def empty(self) -> bool:
        return self.path is None

    def descriptor(self, src_ptr: int = 0, dst_ptr: int = 0) -> GtmiRelayoutDesc:
        d = GtmiRelayoutDesc()
        d.src, d.dst = src_ptr, dst_ptr
        n = len(self.extent)
        d.extent[:n] = self.extent
        d.src_stride[:n] = self.src_strides
        d.dst_stride[:n] = self.dst_strides
        d.ndim, d.itemsize = n, self.itemsize
        return d


def plan(shape: Sequence[int], src_strides: Sequence[int], dst_strides: Sequence[int], itemsize: int) -> RelayoutPlan:
    """Canonical descriptor and path of ``dst[...] = src`` for two views of ``shape`` with the
    given element strides. Raises ``ValueError`` for a destination that overlaps itself, for
    negative strides and for more than ``MAX_DIMS`` dimensions after merging."""
    shape = tuple(int(e) for e in shape)
    src_strides = tuple(int(s) for s in src_strides)
    dst_strides = tuple(int(s) for s in dst_strides)
    itemsize = int(itemsize)
    if not (len(shape) == len(src_strides) == len(dst_strides)):
        raise ValueError("shape and strides have different lengths")
    if itemsize not in (1, 2, 4, 8):
        raise ValueError(f"unsupported element size {itemsize}")
    if any(e < 0 for e in shape):
        raise ValueError(f"negative extent in {shape}")
    if any(e == 0 for e in shape):
        return RelayoutPlan((), (), (), itemsize, None, None, None)
    dims = [(e, ss, ds) for e, ss, ds in zip(shape, src_strides, dst_strides) if e != 1]
    if any(ss < 0 or ds < 0 for _, ss, ds in dims):
        raise ValueError("negative strides are not supported")
    # destination's dimensions slowest to fastest; it must not write an element twice
    dims.sort(key=lambda t: -t[2])
    for (_, _, ds_slow), (e, _, ds) in zip(dims, dims[1:]):
        if ds_slow < ds * e:
            raise ValueError("the destination overlaps itself")
    if dims and dims[-1][2] == 0:
        raise ValueError("the destination overlaps itself")
    merged: List[Tuple[int, int, int]] = []
    for e, ss, ds in dims:
        if merged:
            pe, pss, pds = merged[-1]
            if pds == ds * e and pss == ss * e:  # the slower neighbour continues this one on both sides
                merged[-1] = (pe * e, ss, ds)
                continue
        merged.append((e, ss, ds))
    if not merged:
        merged = [(1, 1, 1)]  # a single element
    if len(merged) > MAX_DIMS:
        raise ValueError(f"more than {MAX_DIMS} dimensions after merging")
    extent = tuple(t[0] for t in merged)
    ss = tuple(t[1] for t in merged)
    ds = tuple(t[2] for t in merged)
    last = len(merged) - 1
    path, a, b = GENERIC, None, None
    if ds[last] == 1 and ss[last] == 1:
        path, a, b = ROW, last, last
    elif ds[last] == 1 and extent[last] >= TILE_MIN:
        cand = [i for i in range(last) if ss[i] == 1]
        if cand:
            ia = max(cand, key=lambda i: (extent[i], i))
            if extent[ia] >= TILE_MIN:
                path, a, b = TILE, ia, last
    return RelayoutPlan(extent, ss, ds, itemsize, path, a, b)


def library_path() -> str:
    with open(_SRC) as f:
        source = f.read()
    with open(_HEADER, "rb") as f:  # not among jit's hashed headers: make it part of this key
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    return jit.compile_source(source, extra_flags=[f"-DGTMI_RELAYOUT_HEADER_DIGEST=0x{digest}"])


def _library():
    global _lib
    with _lock:
        if _lib is None:
            import torch  # noqa: F401  (bind to torch's HIP runtime first)

            lib = ctypes.CDLL(library_path(), mode=ctypes.RTLD_LOCAL)
            lib.gtmi_relayout_copy.restype = ctypes.c_int
            lib.gtmi_relayout_copy.argtypes = [ctypes.POINTER(GtmiRelayoutDesc), ctypes.c_void_p]
            lib.gtmi_relayout_path.restype = ctypes.c_int
            lib.gtmi_relayout_path.argtypes = [ctypes.POINTER(GtmiRelayoutDesc)]
            lib.gtmi_relayout_last_error.restype = ctypes.c_char_p
            lib.gtmi_relayout_abi_version.restype = ctypes.c_int
            if lib.gtmi_relayout_abi_version() != 1:
                raise RuntimeError("gtmi_relayout ABI mismatch")
            _lib = lib
        return _lib


def path_in_library(p: RelayoutPlan) -> Optional[str]:
    """The path the library itself picks for ``p`` (host-only call; the planner must agree)."""
    if p.empty:
        return None
    code = _library().gtmi_relayout_path(ctypes.byref(p.descriptor(src_ptr=16, dst_ptr=16)))
    if code < 0:
        raise RuntimeError(f"gtmi_relayout_path: {_library().gtmi_relayout_last_error().decode()}")
    return _PATH_CODES[code]


def _is_device_tensor(t) -> bool:
    return type(t).__module__.startswith("torch") and hasattr(t, "is_cuda") and bool(t.is_cuda)


def _byte_range(t) -> Tuple[int, int]:
    span = sum((e - 1) * s for e, s in zip(t.shape, t.stride()))
    lo = t.data_ptr()
    return lo, lo + (span + 1) * t.element_size()


def copy(dst, src, stream=None) -> None:
    """``dst[...] = src`` for two device tensors of equal shape and dtype, as one relayout kernel
    on ``stream`` (default: the current stream). ``ValueError`` for anything that is not a device
    tensor on both sides and for a destination that overlaps itself; a source whose memory range
    overlaps the destination's is cloned first; an empty shape is a no-op."""
    import torch

    if not (_is_device_tensor(dst) and _is_device_tensor(src)):
        raise ValueError("relayout.copy needs device tensors on both sides")
    if dst.device != src.device:
        raise ValueError(f"relayout.copy: tensors on different devices ({dst.device}, {src.device})")
    if tuple(dst.shape) != tuple(src.shape):
        raise ValueError(f"relayout.copy: shapes differ ({tuple(src.shape)} -> {tuple(dst.shape)})")
    if dst.dtype != src.dtype:
        raise ValueError(f"relayout.copy: dtypes differ ({src.dtype} -> {dst.dtype})")
    p = plan(dst.shape, src.stride(), dst.stride(), dst.element_size())
    if p.empty:
        return
    s = stream if stream is not None else torch.cuda.current_stream(dst.device)
    with torch.cuda.device(dst.device), torch.cuda.stream(s):
        src = src.detach()
        dlo, dhi = _byte_range(dst)
        slo, shi = _byte_range(src)
        if slo < dhi and dlo < shi:
            src = src.clone()  # allocated and filled on `s`
            p = plan(dst.shape, src.stride(), dst.stride(), dst.element_size())
        lib = _library()
        desc = p.descriptor(src.data_ptr(), dst.data_ptr())
        rc = lib.gtmi_relayout_copy(ctypes.byref(desc), ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"gtmi_relayout_copy failed: {lib.gtmi_relayout_last_error().decode()}")


__all__ = ["GtmiRelayoutDesc", "RelayoutPlan", "ROW", "TILE", "GENERIC", "plan", "copy", "library_path"]
