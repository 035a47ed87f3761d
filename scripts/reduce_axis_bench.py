#!/usr/bin/env python3
"""Axis reductions (level profiles, column sums) against what a user has today, on the device.

    python scripts/reduce_axis_bench.py [--shape 1024 1024 160] [--halo 3] [--out profiles/reduce_axis_bench.json]

Per dtype (f64, f32) one storage of ``shape`` plus ``halo`` cells on every side of I and J;
everything runs over the compute domain. Timed with device events after a warm-up, the methods
alternating in one process, with enough repeats for about a second each; medians and the
10th-90th percentile spread are recorded:

- ``storage.reduce.sum`` and ``absmax`` with ``axis=(0, 1)`` (a level profile: SEGMENT path) and
  ``axis=2`` (column values: LANE path);
- the scalar ``storage.reduce.sum`` of the same box, which moves the same bytes (two passes);
- ``view.sum(dim=...)`` and ``view.abs().amax(dim=...)`` on the sliced view;
- for the profile, the loop of one scalar ``sum`` per level.

``bytes`` is what the method has to read (the box once per pass). The ratios of every axis method
to the scalar ``sum`` (for ``absmax``: to half of it, one pass), to torch and to the loop are
recorded, and whether ``sum(axis=(0, 1))`` and ``sum(axis=2)`` agree bit for bit with the host
restatement on the same field. Needs a GPU; there is no fallback.
"""

import argparse
import json
import os
import sys

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
            "bytes": int(nbytes), "share_of_8TBs": nbytes / (med * 1e-3) / PEAK_BYTES_PER_S}


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


def _bitwise(got, want):
    g, w = got.detach().cpu().numpy(), np.asarray(want)
    return bool(g.shape == w.shape and np.array_equal(g.view(np.int64), w.view(np.int64)))


def run(torch, storage, R, shape, h, dtype, seconds, host_check):
    ni, nj, nk = shape
    full = (ni + 2 * h, nj + 2 * h, nk)
    box = dict(origin=(h, h, 0), domain=(ni, nj, nk))
    gen = torch.Generator(device="cuda").manual_seed(7)
    tdt = storage.torch_dtype(np.dtype(dtype))
    # uniform mantissas over 40 binades, NaN in the halo: a reduction that touches it shows
    a = storage.empty(full, dtype, backend=BE, aligned_index=(h, h, 0))
    a.fill_(float("nan"))
    vals = torch.rand((ni, nj, nk), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    vals *= torch.exp2(torch.randint(-20, 21, (ni, nj, nk), device="cuda", generator=gen).to(torch.float64))
    storage.assign(a[h:h + ni, h:h + nj, :], vals.to(tdt))
    del vals
    va = a[h:h + ni, h:h + nj, :]
    nbytes = ni * nj * nk * np.dtype(dtype).itemsize

    def loop():
        for k in range(nk):
            R.sum(a, origin=(h, h, k), domain=(ni, nj, 1))

    methods = {
        "sum_axis01": (lambda: R.sum(a, axis=(0, 1), **box), 2 * nbytes),
        "absmax_axis01": (lambda: R.absmax(a, axis=(0, 1), **box), nbytes),
        "sum_axis2": (lambda: R.sum(a, axis=2, **box), 2 * nbytes),
        "absmax_axis2": (lambda: R.absmax(a, axis=2, **box), nbytes),
        "scalar_sum": (lambda: R.sum(a, **box), 2 * nbytes),
        "scalar_absmax": (lambda: R.absmax(a, **box), nbytes),
        "torch_sum_dim01": (lambda: va.sum(dim=(0, 1)), nbytes),
        "torch_abs_amax_dim01": (lambda: va.abs().amax(dim=(0, 1)), nbytes),
        "torch_sum_dim2": (lambda: va.sum(dim=2), nbytes),
        "torch_abs_amax_dim2": (lambda: va.abs().amax(dim=2), nbytes),
        "loop_of_scalar_sums_per_level": (loop, 2 * nbytes),
    }
    ms = _interleaved(torch, {k: f for k, (f, _) in methods.items()}, seconds)
    res = {"dtype": np.dtype(dtype).name, "box_bytes": nbytes, "methods": {}, "ratios": {}}
    for name, (_, nb) in methods.items():
        res["methods"][name] = _stats(ms[name], nb)
        print(json.dumps({np.dtype(dtype).name + "." + name: res["methods"][name]}), flush=True)
    t = {k: v["ms"] for k, v in res["methods"].items()}
    for ax, dim in (("axis01", "dim01"), ("axis2", "dim2")):
        res["ratios"][f"sum_{ax}/scalar_sum"] = t[f"sum_{ax}"] / t["scalar_sum"]
        res["ratios"][f"absmax_{ax}/scalar_absmax"] = t[f"absmax_{ax}"] / t["scalar_absmax"]
        res["ratios"][f"sum_{ax}/torch_sum_{dim}"] = t[f"sum_{ax}"] / t[f"torch_sum_{dim}"]
        res["ratios"][f"absmax_{ax}/torch_abs_amax_{dim}"] = t[f"absmax_{ax}"] / t[f"torch_abs_amax_{dim}"]
    res["ratios"]["sum_axis01/loop_of_scalar_sums_per_level"] = t["sum_axis01"] / t["loop_of_scalar_sums_per_level"]
    print(json.dumps({np.dtype(dtype).name + ".ratios": res["ratios"]}), flush=True)
    if host_check:
        ha = storage.to_numpy(a)
        for ax, key in (((0, 1), "sum_axis01_bitwise_equal_to_host"), (2, "sum_axis2_bitwise_equal_to_host")):
            res[key] = _bitwise(R.sum(a, axis=ax, **box), R.sum(ha, axis=ax, **box))
            print(f"{np.dtype(dtype).name}: sum(axis={ax}) agrees bitwise with the host restatement: {res[key]}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 160))
    ap.add_argument("--halo", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-host-check", action="store_true", help="skip the comparison with the host restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reduce_axis_bench.json"))
    args = ap.parse_args()
    import torch

    import gt4py_amd  # noqa: F401
    from gt4py_amd import storage
    from gt4py_amd.storage import reduce as R

    if not torch.cuda.is_available():
        raise SystemExit("reduce_axis_bench needs a GPU")
    result = {"shape": list(args.shape), "halo": args.halo, "device": torch.cuda.get_device_name(0),
              "peak_bytes_per_s": PEAK_BYTES_PER_S, "dtypes": {}}
    for dtype in (np.float64, np.float32):
        result["dtypes"][np.dtype(dtype).name] = run(torch, storage, R, tuple(args.shape), args.halo, dtype, args.seconds,
                                                      not args.no_host_check)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
