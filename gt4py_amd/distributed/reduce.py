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


def global_sum(field, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``storage.reduce.sum`` of the undivided domain, the same bits on every rank."""
    return _GlobalScan(field, None, origin, domain, group, stream, global_count).sum()


def global_dot(a, b, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``storage.reduce.dot`` of the undivided domain."""
    return _GlobalScan(a, b, origin, domain, group, stream, global_count).sum()


def global_norm2(a, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    """``sqrt(global_dot(a, a))`` in f64."""
    d = _GlobalScan(a, a, origin, domain, group, stream, global_count).sum()
    if isinstance(d, np.generic):
        with np.errstate(all="ignore"):
            return np.sqrt(np.float64(d))
    import torch

    return torch.sqrt(d.to(torch.float64))


def global_min(field, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _GlobalScan(field, None, origin, domain, group, stream, global_count).extremum(1)


def global_max(field, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _GlobalScan(field, None, origin, domain, group, stream, global_count).extremum(2)


def global_absmax(field, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _GlobalScan(field, None, origin, domain, group, stream, global_count).extremum(0)


def global_count_nonfinite(field, *, origin=None, domain=None, group=None, stream=None, global_count=None):
    return _GlobalScan(field, None, origin, domain, group, stream, global_count).count_nonfinite()


__all__ = ["global_sum", "global_dot", "global_norm2", "global_min", "global_max", "global_absmax",
           "global_count_nonfinite"]
