"""Reductions over a domain that is split over the ranks of a process group.

Every rank passes its own part of the field (``origin`` / ``domain`` select the part's compute
domain, as in ``storage.reduce``) and every rank gets the same bits back: those a single rank
gets from ``storage.reduce`` on the undivided domain, whatever the number of ranks and the shape
of the parts. The steps are the two passes of ``storage.reduce`` with one collective after each:

1. local ``scan``; the ranks' scan results are gathered and combined by the scan's own rules
   (maximum of absmax / max, minimum of min with -0.0 below +0.0, counts added);
2. local ``fold_sums`` against the global ``(M, N)``; one all-reduce (SUM) of the three fold sums.
   Every partial sum of a fold is exact in f64, so the all-reduce gives the same bits in any order.

Host arrays go over any backend that takes CPU tensors (gloo), device tensors over RCCL; device
results stay on the device. ``N`` is a kernel argument, so the device path reads the gathered
cell counts back to the host once per call unless ``global_count`` is given (the decomposition
of a model is static: count once, pass it on).

With ``axis=`` every function returns one result per kept cell (``storage.reduce`` with ``axis=``):
the partition must cut reduced axes only, so the kept extents are the same on every rank (level
profiles over J strips or a 2-D grid). An all-gather of the kept shape checks that and a mismatch
raises ``ValueError`` on every rank; the steps are the ones above with per-cell arrays in place
of scalars (one all-reduce of the ``3 x cells`` fold sums). A partition that cuts only kept axes
needs no collective: the caller concatenates.
"""

from __future__ import annotations

import numpy as np

from gt4py_amd.storage import reduce as _reduce


def _dist():
    import torch.distributed as dist

    return dist


class _GlobalScan:
    """The combined scan of every rank's part, and what the second pass needs."""

    def __init__(self, a, b, origin, domain, group, stream, global_count):
        import torch

        dist = _dist()
        self.group = group
        self.world = dist.get_world_size(group)
        self.x, self.p, self.dt = _reduce._prepare(a, b, origin, domain, stream, None)
        self.floating = _reduce._floating(self.dt)
        if self.p is None:
            sc = _reduce._scan_host(self.x)
            vals = np.array(sc[:3], dtype=np.float64 if self.floating else np.int64).view(np.int64)
            rec = torch.from_numpy(np.concatenate([vals, np.array(sc[3:7], dtype=np.int64)]))
            parts = [torch.empty_like(rec) for _ in range(self.world)]
            dist.all_gather(parts, rec, group=group)
            vt = np.float64 if self.floating else np.int64
            tuples = []
            for t in parts:
                r = t.numpy()
                tuples.append((*(vt(v) for v in r[:3].view(vt)), *(np.int64(c) for c in r[3:6]), int(r[6])))
            self.scan = _reduce._combine_scans_host(tuples)
            self.count = int(self.scan[6]) if global_count is None else int(global_count)
            return
        p = self.p
        with p._context():
            rec = torch.empty(_reduce.SCAN_SLOTS + 1, dtype=torch.int64, device=p.device)
            if p.desc is None:  # this rank's part is empty: the identities
                i = np.iinfo(np.int64)
                ident = (np.array([0.0, np.inf, -np.inf]).view(np.int64) if self.floating
                         else np.array([i.min, i.max, i.min], dtype=np.int64))
                rec.zero_()
                rec[:3] = torch.from_numpy(ident.copy()).to(p.device)
            else:
                rec[: _reduce.SCAN_SLOTS] = p.scan()
            rec[_reduce.SCAN_SLOTS] = p.count
            parts = [torch.empty_like(rec) for _ in range(self.world)]
            dist.all_gather(parts, rec, group=group)
            recs = torch.stack(parts)
            self.raw = _reduce.combine_scans_device(recs[:, : _reduce.SCAN_SLOTS], self.dt, stream=p.stream)
            if global_count is None:
                global_count = int(recs[:, _reduce.SCAN_SLOTS].sum().item())
        self.count = int(global_count)

    def sum(self):
        import torch

        dist = _dist()
        if self.p is None:
            folds = _reduce._fold_sums_host(self.x, self.scan[0], self.count)
            t = torch.from_numpy(np.array(folds, dtype=np.float64 if self.floating else np.int64))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            return _reduce._finish_sum_host(self.scan, tuple(t.numpy()), self.count, self.floating)
        p = self.p
        folds = p.folds(self.raw, self.count)
        with p._context():
            t = folds.view(torch.float64) if self.floating else folds
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return p.finish(self.raw, folds, self.count)

    def extremum(self, which):
        name = ("absmax", "min", "max")[which]
        if self.count == 0:
            raise ValueError(f"zero-size domain to reduction operation {name} which has no identity")
        out_dt = np.dtype(np.int64) if (which == 0 and not self.floating) else self.dt
        if self.p is None:
            return out_dt.type(np.nan) if self.scan[3] > 0 else out_dt.type(self.scan[which])
        from gt4py_amd import storage

        return self.p.slot(self.raw, 8 + which).to(storage.torch_dtype(out_dt))

    def count_nonfinite(self):
        if self.p is None:
            return np.int64(self.scan[3] + self.scan[4] + self.scan[5])
        return self.p.count_slot(self.raw, 6)


class _GlobalAxisScan:
    """The combined per-cell scans of every rank's part (``axis=``), and what the second pass needs."""

    def __init__(self, a, b, axis, origin, domain, group, stream, global_count):
        import torch

        from gt4py_amd.storage import reduce_axis as _axis

        dist = _dist()
        self.group = group
        self.world = dist.get_world_size(group)
        red = _axis.normalize_axis(axis, _axis._ndim(a))
        q = self.q = _axis._Prepared(a, b, red, origin, domain, stream, None)
        self.floating = q.floating
        vt = np.float64 if self.floating else np.int64
        # the kept shape and the reduced count of every rank
        meta = np.full(_reduce.MAX_DIMS + 2, -1, dtype=np.int64)
        meta[0], meta[1], meta[2 : 2 + len(q.kshape)] = len(q.kshape), q.count, q.kshape
        if q.p is None:
            t = torch.from_numpy(meta)
            metas = [torch.empty_like(t) for _ in range(self.world)]
            dist.all_gather(metas, t, group=group)
            metas = np.stack([m.numpy() for m in metas])
        else:
            with q.p._context():
                t = torch.from_numpy(meta).to(q.p.device)
                metas = [torch.empty_like(t) for _ in range(self.world)]
                dist.all_gather(metas, t, group=group)
                metas = torch.stack(metas).cpu().numpy()  # the one read-back of a call
        shapes = [tuple(int(v) for v in m[2 : 2 + int(m[0])]) for m in metas]
        if any(sh != shapes[0] for sh in shapes):
            raise ValueError(f"global reduction with axis={axis}: the kept extents differ between the ranks ({shapes}); "
                             f"the partition may cut reduced axes only")
        self.count = int(metas[:, 1].sum()) if global_count is None else int(global_count)
        if q.cells == 0:
            return
        if q.p is None:
            sc = _axis._scan_host(q.x)
            rec = torch.from_numpy(np.stack([np.asarray(v, dtype=vt).view(np.int64) for v in sc[:3]] + list(sc[3:6])))
            parts = [torch.empty_like(rec) for _ in range(self.world)]
            dist.all_gather(parts, rec, group=group)
            tuples = [(*(t.numpy()[k].view(vt) for k in range(3)), *(t.numpy()[k] for k in (3, 4, 5))) for t in parts]
            self.scan = _axis._combine_scans_host(tuples, self.floating)
            return
        p = q.p
        with p._context():
            if q.count == 0:  # this rank's part is empty: the identities
                i = np.iinfo(np.int64)
                ident = (np.array([0.0, np.inf, -np.inf]).view(np.int64) if self.floating
                         else np.array([i.min, i.max, i.min], dtype=np.int64))
                rec = torch.zeros((_reduce.SCAN_SLOTS, q.cells), dtype=torch.int64, device=p.device)
                rec[:3] = torch.from_numpy(ident.copy()).to(p.device)[:, None]
            else:
                rec = p.scan(_axis.MASK_ALL)
            parts = [torch.empty_like(rec) for _ in range(self.world)]
            dist.all_gather(parts, rec, group=group)
            if p.desc is None:  # combine needs no descriptor, only the library
                p.lib = _axis._library()
            self.raw = p.combine(torch.stack(parts), _axis.MASK_ALL)

    def _constant(self, value, dt):
        return self.q.constant(value, dt)

    def sum(self):
        import torch

        from gt4py_amd.storage import reduce_axis as _axis

        dist = _dist()
        q = self.q
        st = np.float64 if self.floating else np.int64
        if q.cells == 0:
            return self._constant(0, st)
        if q.p is None:
            folds = np.stack(_axis._fold_sums_host(q.x, self.scan[0], self.count)).astype(st)
            t = torch.from_numpy(folds)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            return _axis._finish_sum_host(self.scan, tuple(t.numpy()), self.count, self.floating).reshape(q.kshape)
        p = q.p
        if q.count == 0:
            with p._context():
                folds = torch.zeros((3, q.cells), dtype=torch.int64, device=p.device)
        else:
            folds = p.folds(self.raw, self.count)
        with p._context():
            t = folds.view(torch.float64) if self.floating else folds
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return p.shaped(p.finish(self.raw, folds, self.count))

    def extremum(self, which):
        name = ("absmax", "min", "max")[which]
        if self.count == 0:
            raise ValueError(f"zero-size reduced extent to reduction operation {name} which has no identity")
        q = self.q
        out_dt = np.dtype(np.int64) if (which == 0 and not self.floating) else q.dt
        if q.cells == 0:
            return self._constant(0, out_dt)
        if q.p is None:
            v = self.scan[which].astype(out_dt)
            if self.floating:
                v = np.where(self.scan[3] > 0, out_dt.type(np.nan), v)
            return v.reshape(q.kshape)
        from gt4py_amd import storage

        return q.p.shaped(q.p.values(self.raw[8 + which]).to(storage.torch_dtype(out_dt)))

    def count_nonfinite(self):
        q = self.q
        if q.cells == 0:
            return self._constant(0, np.int64)
        if q.p is None:
            return (self.scan[3] + self.scan[4] + self.scan[5]).astype(np.int64).reshape(q.kshape)
        return q.p.shaped(self.raw[6])


def _scan_of(a, b, axis, origin, domain, group, stream, global_count):
    if axis is not None:
        return _GlobalAxisScan(a, b, axis, origin, domain, group, stream, global_count)
    return _GlobalScan(a, b, origin, domain, group, stream, global_count)


def global_sum(field, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``storage.reduce.sum`` of the undivided domain, the same bits on every rank."""
    return _scan_of(field, None, axis, origin, domain, group, stream, global_count).sum()


def global_dot(a, b, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``storage.reduce.dot`` of the undivided domain."""
    return _scan_of(a, b, axis, origin, domain, group, stream, global_count).sum()


def global_norm2(a, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``sqrt(global_dot(a, a))`` in f64."""
    d = _scan_of(a, a, axis, origin, domain, group, stream, global_count).sum()
    if isinstance(d, (np.generic, np.ndarray)):
        with np.errstate(all="ignore"):
            return np.sqrt(np.asarray(d, dtype=np.float64))
    import torch

    return torch.sqrt(d.to(torch.float64))


def global_min(field, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _scan_of(field, None, axis, origin, domain, group, stream, global_count).extremum(1)


def global_max(field, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _scan_of(field, None, axis, origin, domain, group, stream, global_count).extremum(2)


def global_absmax(field, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _scan_of(field, None, axis, origin, domain, group, stream, global_count).extremum(0)


def global_count_nonfinite(field, *, axis=None, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _scan_of(field, None, axis, origin, domain, group, stream, global_count).count_nonfinite()


__all__ = ["global_sum", "global_dot", "global_norm2", "global_min", "global_max", "global_absmax",
           "global_count_nonfinite"]
