"""``distributed.reduce`` with ``axis=`` over gloo: worlds of 2 and 3 ranks hold uneven J strips of
one field; every level profile (``axis=(0, 1)``) on every rank has the bits of ``storage.reduce``
with the same ``axis`` on the undivided field. Mismatched kept extents raise on every rank.
"""

import os
import pickle
import socket
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (33, 29, 11)
HALO = 2
STRIPS = {2: (0, 9, 29), 3: (0, 4, 17, 29)}  # uneven J bounds per world size
AXIS = (0, 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _fields(which):
    rng = np.random.default_rng(45)
    n = int(np.prod(SHAPE))

    def wide():
        return (rng.uniform(-1, 1, n) * np.exp2(rng.integers(-30, 31, n))).reshape(SHAPE)

    a, b = wide(), wide()
    if which == "special":
        a[5, 20, 3] = np.nan  # a NaN on one rank only (the last strip of both partitions)
        a[7, 2, 5] = 2.0**40  # level 5's maximum lies on the first rank only
        a[0, 0, 7] = np.inf
        a[32, 28, 8] = np.inf
        a[32, 28, 9], a[1, 1, 9] = np.inf, -np.inf
        a[:, :10, 10] = 0.0
        a[:, 10:, 10] = -0.0
    elif which == "int64":
        i = np.iinfo(np.int64)
        a = rng.integers(i.min, i.max, SHAPE, dtype=np.int64)
        b = rng.integers(i.min, i.max, SHAPE, dtype=np.int64)
    return a, b


def _single_domain(a, b):
    from gt4py_amd.storage import reduce as R

    return {"sum": R.sum(a, axis=AXIS), "dot": R.dot(a, b, axis=AXIS), "norm2": R.norm2(a, axis=AXIS),
            "min": R.min(a, axis=AXIS), "max": R.max(a, axis=AXIS), "absmax": R.absmax(a, axis=AXIS),
            "count_nonfinite": R.count_nonfinite(a, axis=AXIS), "sum_j": R.sum(a, axis=1)}


def _worker(rank, world, port, outdir, which):
    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    from gt4py_amd.distributed import reduce as G

    dist.init_process_group("gloo", rank=rank, world_size=world)
    a, b = _fields(which)
    j0, j1 = STRIPS[world][rank], STRIPS[world][rank + 1]
    # the rank's strip inside a NaN halo: only the compute domain may be read
    h = HALO
    la = np.full((SHAPE[0] + 2 * h, j1 - j0 + 2 * h, SHAPE[2]), np.nan if a.dtype.kind == "f" else 7, dtype=a.dtype)
    lb = la.copy()
    la[h:-h, h:-h, :] = a[:, j0:j1, :]
    lb[h:-h, h:-h, :] = b[:, j0:j1, :]
    kw = dict(axis=AXIS, origin=(h, h, 0), domain=(SHAPE[0], j1 - j0, SHAPE[2]))
    out = {"sum": G.global_sum(la, **kw), "dot": G.global_dot(la, lb, **kw), "norm2": G.global_norm2(la, **kw),
           "min": G.global_min(la, **kw), "max": G.global_max(la, **kw), "absmax": G.global_absmax(la, **kw),
           "count_nonfinite": G.global_count_nonfinite(la, **kw),
           "sum_j": G.global_sum(la, **dict(kw, axis=1, global_count=SHAPE[1]))}
    if a.dtype.kind == "f":
        import torch

        t = torch.from_numpy(np.sum(a[:, j0:j1, :], axis=AXIS))  # a per-rank sum followed by an all-reduce
        dist.all_reduce(t)
        out["naive"] = t.numpy().copy()
    # the kept extents differ between the ranks (the strips are uneven and J is kept): every rank raises
    try:
        G.global_sum(la, **dict(kw, axis=(0, 2)))
        out["mismatch"] = None
    except ValueError as e:
        out["mismatch"] = str(e)
    with open(os.path.join(outdir, f"out_{rank}.pkl"), "wb") as f:
        pickle.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


def _same(g, w):
    g, w = np.asarray(g), np.asarray(w)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind == "f":
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            return False
        g, w = np.where(np.isnan(g), 0, g), np.where(np.isnan(w), 0, w)
    return bool(np.array_equal(g.view(np.int64), w.view(np.int64)))


@pytest.mark.parametrize("world,which", [(2, "wide"), (3, "wide"), (2, "special"), (3, "special"), (2, "int64")])
def test_global_level_profiles_match_single_domain(tmp_path, world, which):
    import torch.multiprocessing as mp

    sys.path.insert(0, REPO)
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), which), nprocs=world, join=True)
    a, b = _fields(which)
    want = _single_domain(a, b)
    assert want["sum"].shape == (SHAPE[2],) and want["sum_j"].shape == (SHAPE[0], SHAPE[2])
    if which == "special":
        assert np.isnan(want["sum"][3]) and want["count_nonfinite"][3] == 1 and np.isnan(want["max"][3])
        assert want["absmax"][5] == 2.0**40 and want["sum"][7] == np.inf and np.isnan(want["sum"][9])
        assert want["sum"][10] == 0 and not np.signbit(want["sum"][10]) and np.signbit(want["min"][10])
    for r in range(world):
        with open(tmp_path / f"out_{r}.pkl", "rb") as f:
            got = pickle.load(f)
        for name, w in want.items():
            assert _same(got[name], w), (r, name, got[name], w)
        assert got["mismatch"] is not None and "kept extents differ" in got["mismatch"], r
        if which == "wide":
            # the test can tell a reproducible profile from per-rank sums and an all-reduce
            assert not _same(got["naive"], want["sum"]), "the seed no longer separates the two sums"
