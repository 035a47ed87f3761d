"""Device-side storage relayout: the planner (CPU), the library build, and
``storage.from_array`` / ``assign`` / ``contiguous`` on the device (GPU).

Every comparison is bitwise (``uint8`` views), so NaN payloads and -0.0 count.
"""

import ctypes

import numpy as np
import pytest

import gt4py_amd  # noqa: F401  (registers the backends)
from gt4py_amd import storage
from gt4py_amd.storage import relayout

BE = "gt:mi355x"
ALIGN = 32  # elements, the backend's alignment


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _c_strides(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return tuple(reversed(out))


def _storage_geometry(shape, itemsize, aligned_index=None, dims=None):
    """(element strides, offset of element 0, flat size) of a gt:mi355x storage."""
    dims = dims if dims is not None else ("I", "J", "K")[: len(shape)]
    aligned_index = aligned_index if aligned_index is not None else (0,) * len(shape)
    lm = storage.REGISTRY[BE]["layout_map"](tuple(dims))
    strides, shift, total, _ = storage._allocation_plan(tuple(shape), lm, itemsize, ALIGN * itemsize, aligned_index)
    return tuple(strides), int(shift), int(total)


def _span(shape, strides):
    return sum((e - 1) * s for e, s in zip(shape, strides)) + 1


# ---------------------------------------------------------------------------------------------
# plan() against brute force
# ---------------------------------------------------------------------------------------------


def _row(name, shape, src, dst, path):
    """src / dst: (strides, offset); sizes follow from the spans."""
    return pytest.param(shape, src, dst, path, id=name)


def _plan_table():
    rows = []
    big = (65, 3, 67)
    st, off, _ = _storage_geometry(big, 8)
    st_sh, off_sh, _ = _storage_geometry(big, 8, aligned_index=(2, 3, 0))
    rows.append(_row("c_to_ifirst", big, (_c_strides(big), 0), (st, off), "TILE"))
    rows.append(_row("ifirst_to_c", big, (st, off), (_c_strides(big), 0), "TILE"))
    rows.append(_row("ifirst_padded_shifted_to_ifirst", big, (st_sh, off_sh), (st, off), "ROW"))
    rows.append(_row("c_to_ifirst_shifted", big, (_c_strides(big), 5), (st_sh, off_sh), "TILE"))
    rows.append(_row("c_to_c_merges_to_one_row", big, (_c_strides(big), 0), (_c_strides(big), 3), "ROW"))
    # masks
    for dims, shape, path in ((("I", "J"), (65, 20), "TILE"), (("I", "K"), (20, 33), "TILE"), (("K",), (40,), "ROW"),
                              (("I", "J"), (65, 7), "GENERIC")):
        g, o, _ = _storage_geometry(shape, 4, dims=dims)
        rows.append(_row("mask_" + "".join(dims) + "_" + "x".join(map(str, shape)), shape, (_c_strides(shape), 0), (g, o), path))
    # data dimensions (5, 6, 7) + (2, 3): they are the storage's slowest axes, and the C-order
    # source's stride-1 dimension is the last of them (extent 3): too short for a tile
    shape = (5, 6, 7, 2, 3)
    g, o, _ = _storage_geometry(shape, 8, dims=("I", "J", "K", "0", "1"))
    rows.append(_row("data_dims", shape, (_c_strides(shape), 0), (g, o), "GENERIC"))
    # stepped slices
    shape = (65, 4, 66)
    g, o, _ = _storage_geometry(shape, 2)
    cs = _c_strides((130, 4, 66))
    rows.append(_row("step2_on_I_of_c", shape, ((2 * cs[0], cs[1], cs[2]), 0), (g, o), "TILE"))
    cs = _c_strides((65, 4, 132))
    rows.append(_row("step2_on_K_of_c", shape, ((cs[0], cs[1], 2), 1), (g, o), "GENERIC"))
    rows.append(_row("step2_both_sides", (33, 5), ((2, 80), 0), ((2, 70), 1), "GENERIC"))
    # broadcast sources
    g, o, _ = _storage_geometry(big, 1)
    rows.append(_row("broadcast_K_row", big, ((0, 0, 1), 0), (g, o), "TILE"))
    rows.append(_row("broadcast_I_column", big, ((1, 0, 0), 0), (g, o), "ROW"))
    rows.append(_row("broadcast_scalar", big, ((0, 0, 0), 0), (g, o), "GENERIC"))
    # extents around the tile size on both tiled dimensions (I on the destination, K on the source)
    for ni, nk in ((63, 64), (64, 65), (65, 130), (130, 63), (64, 64), (16, 16)):
        shape = (ni, 2, nk)
        g, o, _ = _storage_geometry(shape, 4)
        rows.append(_row(f"tile_{ni}x{nk}", shape, (_c_strides(shape), 0), (g, o), "TILE"))
    for ni, nk in ((1, 64), (64, 1), (15, 64), (64, 15)):
        shape = (ni, 2, nk)
        g, o, _ = _storage_geometry(shape, 4)
        rows.append(_row(f"short_{ni}x{nk}", shape, (_c_strides(shape), 0), (g, o), "GENERIC"))
    rows.append(_row("single_element", (1, 1, 1), ((1, 1, 1), 0), ((7, 3, 1), 2), "ROW"))
    return rows


def _walk(p, src_flat, dst_flat, src_off, dst_off):
    """dst[...] = src by walking the canonical descriptor."""
    if p.empty:
        return
    idx = np.indices(p.extent).reshape(len(p.extent), -1)
    so = src_off + sum(idx[d] * p.src_strides[d] for d in range(len(p.extent)))
    do = dst_off + sum(idx[d] * p.dst_strides[d] for d in range(len(p.extent)))
    assert len(np.unique(do)) == do.size
    dst_flat[do] = src_flat[so]


@pytest.mark.parametrize("shape, src, dst, path", _plan_table())
def test_plan_equals_brute_force(shape, src, dst, path):
    (ss, so), (ds, do) = src, dst
    src_flat = np.arange(so + _span(shape, ss) + 3, dtype=np.int64) + 1000
    dst_flat = np.full(do + _span(shape, ds) + 3, -1, dtype=np.int64)
    view = lambda flat, off, st: np.lib.stride_tricks.as_strided(  # noqa: E731
        flat[off:], shape=shape, strides=tuple(s * 8 for s in st))
    want = dst_flat.copy()
    view(want, do, ds)[...] = view(src_flat, so, ss)
    p = relayout.plan(shape, ss, ds, 8)
    _walk(p, src_flat, dst_flat, so, do)
    assert np.array_equal(dst_flat, want)
    assert p.path == path
    # canonical: no extent 1 (but a lone one), destination slowest first, nothing left to merge
    assert len(p.extent) <= relayout.MAX_DIMS
    assert all(e > 1 for e in p.extent) or p.extent == (1,)
    assert list(p.dst_strides) == sorted(p.dst_strides, reverse=True)
    for i in range(len(p.extent) - 1):
        e = p.extent[i + 1]
        assert not (p.dst_strides[i] == p.dst_strides[i + 1] * e and p.src_strides[i] == p.src_strides[i + 1] * e)
    if path == "TILE":
        assert p.src_strides[p.a] == 1 and p.dst_strides[p.b] == 1 and p.a != p.b
        assert min(p.extent[p.a], p.extent[p.b]) >= relayout.TILE_MIN
    elif path == "ROW":
        assert p.a == p.b and p.src_strides[p.a] == 1 and p.dst_strides[p.b] == 1


def test_plan_descriptor_fields():
    p = relayout.plan((4, 1, 6), (6, 6, 1), (1, 4, 4), 2)
    d = p.descriptor(src_ptr=4096, dst_ptr=8192)
    assert (d.src, d.dst, d.ndim, d.itemsize) == (4096, 8192, 2, 2)
    assert list(d.extent[:2]) == [6, 4] and list(d.src_stride[:2]) == [1, 6] and list(d.dst_stride[:2]) == [4, 1]
    assert ctypes.sizeof(d) == 2 * 8 + 3 * 8 * relayout.MAX_DIMS + 8


def test_plan_empty_and_errors():
    assert relayout.plan((3, 0, 2), (2, 2, 1), (2, 2, 1), 4).empty
    with pytest.raises(ValueError):  # zero destination stride
        relayout.plan((3, 4), (4, 1), (0, 1), 4)
    with pytest.raises(ValueError):  # aliasing destination strides
        relayout.plan((3, 4), (4, 1), (2, 1), 4)
    with pytest.raises(ValueError):
        relayout.plan((3, 4), (4, 1), (4, 1), 3)
    with pytest.raises(ValueError):  # nine dimensions that do not merge
        relayout.plan((2,) * 9, tuple(3 ** i for i in range(9)), tuple(3 ** (8 - i) for i in range(9)), 1)


def test_library_builds_loads_and_agrees_with_the_planner():
    so = relayout.library_path()
    assert so.endswith("stencil.so")
    lib = relayout._library()
    assert lib.gtmi_relayout_abi_version() == 1
    assert lib.gtmi_relayout_last_error() is not None
    for param in _plan_table():
        shape, (ss, _), (ds, _), path = param.values
        p = relayout.plan(shape, ss, ds, 4)
        assert relayout.path_in_library(p) == p.path == path, param.id
    bad = relayout.plan((3, 4), (8, 1), (8, 1), 4).descriptor(16, 16)
    assert bad.ndim == 2
    bad.dst_stride[0] = 2  # overlapping destination: refused before any launch
    assert lib.gtmi_relayout_copy(ctypes.byref(bad), None) != 0
    assert b"overlap" in lib.gtmi_relayout_last_error()


def test_copy_refuses_host_arrays_and_overlapping_destinations():
    import torch

    a = np.zeros((3, 4))
    with pytest.raises(ValueError):
        relayout.copy(a, a.copy())
    with pytest.raises(ValueError):
        relayout.copy(torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(ValueError):
        relayout.plan((3, 4), (4, 1), (0, 1), 8)


def test_assign_and_contiguous_on_numpy_storages():
    rng = np.random.default_rng(3)
    h = rng.standard_normal((5, 6, 7))
    dst = storage.zeros((5, 6, 7), np.float32, backend="numpy", aligned_index=(1, 1, 0))
    want = dst.copy()
    want[...] = h
    assert storage.assign(dst, h) is dst
    assert _same_bits(dst, want)
    import torch

    storage.assign(dst, torch.from_numpy(h[::-1].copy()))  # a host tensor
    want[...] = h[::-1]
    assert _same_bits(dst, want)
    view = storage.from_array(h, backend="numpy").transpose(2, 0, 1)[:, ::2]
    c = storage.contiguous(view)
    assert isinstance(c, np.ndarray) and c.flags["C_CONTIGUOUS"] and not np.shares_memory(c, view)
    assert _same_bits(c, np.ascontiguousarray(view))
    with pytest.raises(ValueError):
        storage.assign(dst, h[:4])
    with pytest.raises(ValueError):
        storage.assign(dst, h[:, :, :1])  # no broadcasting
    assert "assign" in storage.__all__ and "contiguous" in storage.__all__


# ---------------------------------------------------------------------------------------------
# GPU: every test allocates a device tensor first, inside its body
# ---------------------------------------------------------------------------------------------

SHAPES = [(1, 1, 1), (3, 1, 2), (63, 5, 7), (64, 64, 1), (65, 3, 67), (130, 2, 66)]
DTYPES = [np.bool_, np.int16, np.float32, np.float64]


def _random_bits(rng, shape, dtype):
    """Random bit patterns (NaN payloads, -0.0, denormals included); 0/1 for bool."""
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return rng.integers(0, 2, shape).astype(np.bool_)
    n = int(np.prod(shape))
    return rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype).reshape(shape)


def _device_sources(torch, h):
    """Device views with the values of ``h`` (3-D) in different layouts."""
    ni, nj, nk = h.shape
    dev = torch.device("cuda")
    out = {"c_order": torch.from_numpy(h).to(dev)}
    out["permuted"] = torch.from_numpy(np.ascontiguousarray(h.transpose(2, 1, 0))).to(dev).permute(2, 1, 0)
    wide = torch.zeros((ni, nj, 2 * nk), dtype=out["c_order"].dtype, device=dev)
    wide[:, :, 1::2] = out["c_order"]
    out["step2_K"] = wide[:, :, 1::2]
    tall = torch.zeros((2 * ni, nj, nk), dtype=out["c_order"].dtype, device=dev)
    tall[::2] = out["c_order"]
    out["step2_I"] = tall[::2]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_from_array_device_matrix(shape, dtype):
    import torch

    torch.empty(1, device="cuda")
    rng = np.random.default_rng(11)
    h = _random_bits(rng, shape, dtype)
    sources = _device_sources(torch, h)
    sources["broadcast"] = torch.from_numpy(np.ascontiguousarray(h[:, :1, :])).cuda().expand(*shape)
    for ai in ((0, 0, 0), (2, 3, 0)):
        for name, src_dev in sources.items():
            got = storage.to_numpy(storage.from_array(src_dev, dtype, backend=BE, aligned_index=ai))
            want = storage.to_numpy(storage.from_array(src_dev.cpu().numpy(), dtype, backend=BE, aligned_index=ai))
            assert _same_bits(got, want), (name, ai)
            if name != "broadcast":
                assert _same_bits(want, h)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(65, 3, 67), (63, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_assign_writes_nothing_outside_the_view(shape, dtype):
    import torch

    torch.empty(1, device="cuda")
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(5)
    h = _random_bits(rng, shape, dtype)
    lm = storage.REGISTRY[BE]["layout_map"](("I", "J", "K"))
    sources = _device_sources(torch, h)
    for ai in ((2, 3, 0), (3, 3, 0)):
        # same-layout storages: equal 16-B phase (the 16-B ROW kernel, with a head where the
        # phase is not 0) and a different phase (one element per lane)
        sources["storage_same_phase"] = storage.from_array(h, dtype, backend=BE, aligned_index=ai)
        sources["storage_other_phase"] = storage.from_array(h, dtype, backend=BE, aligned_index=(0, 0, 0))
        for name, src_dev in sources.items():
            buf, arr = storage.allocate_gpu(shape, lm, dtype, ALIGN * dtype.itemsize, ai)
            buf.view(torch.uint8).fill_(0xA5)
            storage.assign(arr, src_dev)
            flat = np.full(buf.numel() * dtype.itemsize, 0xA5, dtype=np.uint8).view(dtype)
            np.lib.stride_tricks.as_strided(
                flat[arr.storage_offset():], shape=shape, strides=tuple(s * dtype.itemsize for s in arr.stride())
            )[...] = h
            assert _same_bits(buf.cpu().numpy(), flat), (name, ai)


@pytest.mark.gpu
def test_masks_and_data_dimensions():
    import torch

    torch.empty(1, device="cuda")
    rng = np.random.default_rng(2)
    for dims, shape in ((("I", "J"), (65, 20)), (("I", "K"), (20, 33)), (("K",), (40,)), (("I", "J"), (65, 7))):
        h = _random_bits(rng, shape, np.float32)
        got = storage.from_array(torch.from_numpy(h).cuda(), np.float32, backend=BE, dimensions=dims)
        want = storage.from_array(h, np.float32, backend=BE, dimensions=dims)
        assert got.stride() == want.stride()
        assert _same_bits(storage.to_numpy(got), storage.to_numpy(want)) and _same_bits(storage.to_numpy(got), h)
    h = _random_bits(rng, (5, 6, 7, 2, 3), np.float64)
    dt = np.dtype((np.float64, (2, 3)))
    got = storage.from_array(torch.from_numpy(h).cuda(), dt, backend=BE, aligned_index=(1, 1, 0))
    want = storage.from_array(h, dt, backend=BE, aligned_index=(1, 1, 0))
    assert tuple(got.shape) == (5, 6, 7, 2, 3) and got.stride() == want.stride()
    assert _same_bits(storage.to_numpy(got), h) and _same_bits(storage.to_numpy(want), h)
    with pytest.raises(ValueError, match="Incompatible data shape"):
        storage.from_array(torch.from_numpy(h).cuda(), np.dtype((np.float64, (3, 2))), backend=BE)
    c = storage.contiguous(got)
    assert c.is_contiguous() and _same_bits(c.cpu().numpy(), h)


@pytest.mark.gpu
def test_cast_on_the_device_equals_host_astype():
    import torch

    torch.empty(1, device="cuda")
    h = np.random.default_rng(9).integers(-2**31, 2**31, (65, 3, 67), dtype=np.int32)
    t = torch.from_numpy(h).cuda()
    got = storage.from_array(t, np.float64, backend=BE, aligned_index=(2, 3, 0))
    assert got.dtype == torch.float64
    assert _same_bits(storage.to_numpy(got), h.astype(np.float64))
    kept = storage.from_array(t, None, backend=BE)
    assert kept.dtype == torch.int32 and _same_bits(storage.to_numpy(kept), h)
    dst = storage.zeros((65, 3, 67), np.float32, backend=BE)
    storage.assign(dst, t)
    assert _same_bits(storage.to_numpy(dst), h.astype(np.float32))
    storage.assign(dst, (h // 3).astype(np.int64))  # a host source goes through the host path
    assert _same_bits(storage.to_numpy(dst), (h // 3).astype(np.float32))
    with pytest.raises(ValueError):
        storage.assign(dst, t[:64])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_contiguous_on_the_device(dtype):
    import torch

    torch.empty(1, device="cuda")
    h = _random_bits(np.random.default_rng(4), (65, 3, 67), dtype)
    arr = storage.from_array(h, dtype, backend=BE, aligned_index=(2, 3, 0))
    for view in (arr, arr[1:, :, ::2], arr.permute(1, 2, 0)):
        c = storage.contiguous(view)
        assert isinstance(c, torch.Tensor) and c.is_cuda and c.is_contiguous() and c.dtype == view.dtype
        lo, hi = relayout._byte_range(view)
        assert not (lo <= c.data_ptr() < hi)
        assert _same_bits(c.cpu().numpy(), storage.to_numpy(view))


@pytest.mark.gpu
def test_assign_from_a_view_of_the_destination_buffer():
    import torch

    torch.empty(1, device="cuda")
    shape = (65, 3, 67)
    lm = storage.REGISTRY[BE]["layout_map"](("I", "J", "K"))
    h = np.random.default_rng(8).standard_normal(int(np.prod(shape)) + 4096)
    buf, arr = storage.allocate_gpu(shape, lm, np.float64, ALIGN * 8, (0, 0, 0))
    buf[: h.size] = torch.from_numpy(h).cuda()[: buf.numel()]
    src = torch.as_strided(buf, shape, _c_strides(shape), arr.storage_offset() + 1)  # C-order over the same memory
    other = storage.zeros(shape, np.float64, backend=BE)
    storage.assign(other, src.clone())
    want = storage.to_numpy(other)
    storage.assign(arr, src)
    assert _same_bits(storage.to_numpy(arr), want)
    same = want.copy()
    storage.assign(arr, arr)  # onto itself
    assert _same_bits(storage.to_numpy(arr), same)
    with pytest.raises(ValueError):  # a destination that overlaps itself
        relayout.copy(buf[:1].expand(8), buf[8:16])
    before = buf.clone()
    relayout.copy(buf[:0].reshape(0, 3), buf[:0].reshape(0, 3))  # an empty box is a no-op
    assert storage.contiguous(arr[:0]).shape == (0, 3, 67)
    assert torch.equal(buf.view(torch.int64), before.view(torch.int64))


@pytest.mark.gpu
def test_assign_on_a_side_stream():
    import torch

    torch.empty(1, device="cuda")
    h = _random_bits(np.random.default_rng(6), (130, 2, 66), np.float32)
    src = torch.from_numpy(h).cuda()
    ints = torch.from_numpy(h.view(np.int32)).cuda()
    dst = storage.zeros(h.shape, np.float32, backend=BE)
    dst64 = storage.zeros(h.shape, np.float64, backend=BE)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    storage.assign(dst, src, stream=s)
    storage.assign(dst64, ints, stream=s)  # with a cast on the side stream
    s.synchronize()
    assert _same_bits(storage.to_numpy(dst), h)
    assert _same_bits(storage.to_numpy(dst64), h.view(np.int32).astype(np.float64))


@pytest.mark.gpu
def test_from_array_makes_no_host_round_trip(monkeypatch):
    import torch

    t = torch.arange(65 * 3 * 67, dtype=torch.float64, device="cuda").reshape(65, 3, 67)

    def no_cpu(self, *a, **k):
        raise AssertionError("device->host transfer in from_array")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", no_cpu)
        arr = storage.from_array(t, backend=BE, aligned_index=(2, 3, 0))
        dense = storage.contiguous(arr)
        storage.assign(arr, dense)

        class Foreign:  # any object with __cuda_array_interface__ takes the same path
            __cuda_array_interface__ = t.__cuda_array_interface__

        other = storage.from_array(Foreign(), backend=BE)
        storage.assign(other, Foreign())
    assert torch.equal(other, arr)
    assert _same_bits(storage.to_numpy(arr), np.arange(65 * 3 * 67, dtype=np.float64).reshape(65, 3, 67))
    assert torch.equal(dense, t)


@pytest.mark.gpu
def test_box_past_two_to_the_31_elements():
    import torch

    torch.empty(1, device="cuda")
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip("needs 6 GB of free device memory")
    ni, nj, nk = 1290, 1290, 1291
    assert ni * nj * nk > 2**31
    iv, jv, kv = (np.arange(n).astype(np.int8) * np.int8(m) for n, m in ((ni, 7), (nj, 13), (nk, 31)))
    src = torch.zeros((ni, nj, nk), dtype=torch.int8, device="cuda")
    src.add_(torch.from_numpy(iv).cuda()[:, None, None])  # int8 arithmetic wraps, as numpy's below
    src.add_(torch.from_numpy(jv).cuda()[None, :, None])
    src.add_(torch.from_numpy(kv).cuda()[None, None, :])
    arr = storage.from_array(src, np.int8, backend=BE)
    assert arr.stride(0) == 1 and tuple(arr.shape) == (ni, nj, nk)
    for k in (0, nk // 2, nk - 1):
        want = (iv[:, None] + jv[None, :] + kv[k]).astype(np.int8)
        assert np.array_equal(arr[:, :, k].cpu().numpy(), want), k
    for i in (0, ni - 1):
        for j in (0, nj - 1):
            for k in (0, nk - 1):
                assert int(arr[i, j, k]) == (int(iv[i]) + int(jv[j]) + int(kv[k]) + 128) % 256 - 128
