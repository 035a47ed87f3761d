#!/usr/bin/env python3
"""Relayout kernel against torch's ``copy_`` on the device, case by case.

    python scripts/relayout_bench.py [--shape 1024 1024 160] [--out profiles/relayout_bench.json]

Cases (f64 and f32): C-order tensor -> storage; storage -> ``contiguous``; storage with
``aligned_index=(3, 3, 0)`` -> storage of the same layout (ROW); a stepped slice -> storage
(GENERIC). Per case the relayout kernel and ``dst.copy_(src)`` -- the only device-side route
without the kernel -- alternate in one process after a warm-up, each call timed with device
events, with enough repeats for about a second per method. The host round trip
(device -> numpy -> ``from_array``) is timed a few times for the record. Needs a GPU; there is
no fallback.

Recorded per case and method: median milliseconds, the spread over the repeats (10th to 90th
percentile), and 2 x bytes / time as a share of 8 TB/s. ``kernel_not_slower`` is
``median(kernel) <= median(copy_) + max(spread(kernel), spread(copy_))``.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_BYTES_PER_S = 8e12
BE = "gt:mi355x"


def _stats(ms, nbytes):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    p10, p90 = (float(x) for x in np.percentile(ms, [10, 90]))
    return {"ms": med, "spread_ms": p90 - p10, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "repeats": int(ms.size),
            "share_of_8TBs": 2 * nbytes / (med * 1e-3) / PEAK_BYTES_PER_S}


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _interleaved(torch, methods, seconds):
    """Alternate the methods; repeats sized from the warm-up so each gets about ``seconds``."""
    for fn in methods.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    est = max(max(_timed(torch, fn) for fn in methods.values()), 1e-3)
    repeats = int(min(400, max(10, seconds * 1e3 / est)))
    out = {name: [] for name in methods}
    for _ in range(repeats):
        for name, fn in methods.items():
            out[name].append(_timed(torch, fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 160))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relayout_bench.json"))
    args = ap.parse_args()
    import torch

    import gt4py_amd  # noqa: F401
    from gt4py_amd import storage
    from gt4py_amd.storage import relayout

    if not torch.cuda.is_available():
        raise SystemExit("relayout_bench needs a GPU")
    shape = tuple(args.shape)
    ni, nj, nk = shape
    result = {"shape": list(shape), "device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "cases": []}
    for dtype in (np.float64, np.float32):
        dtype = np.dtype(dtype)
        tdt = storage.torch_dtype(dtype)
        nbytes = ni * nj * nk * dtype.itemsize

        def cases():
            src = torch.rand(shape, dtype=tdt, device="cuda")
            yield "c_order_to_storage", src, storage.empty(shape, dtype, backend=BE)
            del src
            st = storage.from_array(torch.rand(shape, dtype=tdt, device="cuda"), dtype, backend=BE)
            yield "storage_to_contiguous", st, torch.empty(shape, dtype=tdt, device="cuda")
            del st
            st = storage.from_array(torch.rand(shape, dtype=tdt, device="cuda"), dtype, backend=BE, aligned_index=(3, 3, 0))
            yield "storage_to_storage_row", st, storage.empty(shape, dtype, backend=BE, aligned_index=(3, 3, 0))
            del st
            wide = torch.rand((ni, nj, 2 * nk), dtype=tdt, device="cuda")
            yield "stepped_slice_to_storage", wide[:, :, ::2], storage.empty(shape, dtype, backend=BE)

        for name, src, dst in cases():
            p = relayout.plan(dst.shape, src.stride(), dst.stride(), dtype.itemsize)
            check = torch.empty_like(dst)
            relayout.copy(dst, src)
            check.copy_(src)
            if not torch.equal(dst, check):
                raise SystemExit(f"{name} {dtype.name}: kernel and copy_ disagree")
            del check
            ms = _interleaved(torch, {"kernel": lambda: relayout.copy(dst, src), "torch_copy_": lambda: dst.copy_(src)},
                              args.seconds)
            rec = {"case": name, "dtype": dtype.name, "path": p.path, "bytes": nbytes,
                   "kernel": _stats(ms["kernel"], nbytes), "torch_copy_": _stats(ms["torch_copy_"], nbytes)}
            spread = max(rec["kernel"]["spread_ms"], rec["torch_copy_"]["spread_ms"])
            rec["kernel_not_slower"] = bool(rec["kernel"]["ms"] <= rec["torch_copy_"]["ms"] + spread)
            if name == "c_order_to_storage" and args.host_repeats > 0:
                host = []
                for _ in range(args.host_repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arr = storage.from_array(src.detach().cpu().numpy(), dtype, backend=BE)
                    torch.cuda.synchronize()
                    host.append((time.perf_counter() - t0) * 1e3)
                    del arr
                rec["host_round_trip"] = _stats(host, nbytes)
            result["cases"].append(rec)
            print(json.dumps(rec), flush=True)
            del src, dst
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
