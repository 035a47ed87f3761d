#!/usr/bin/env python3
"""Reduction kernels against the torch expressions a user writes today, on the device.

    python scripts/reduce_bench.py [--shape 1024 1024 160] [--halo 3] [--out profiles/reduce_bench.json]

One f64 storage pair of ``shape`` plus ``halo`` cells on every side of I and J; everything runs
over the compute domain. Timed with device events after a warm-up, the methods alternating in
one process, with enough repeats for about a second each; medians and the 10th-90th percentile
spread are recorded:

- ``scan``, ``fold_sums`` (the two passes), ``sum`` (both passes and the finish) and ``dot`` of
  ``storage.reduce``;
- ``view.sum()``, ``view.abs().max()``, ``torch.isfinite(view).all()`` and ``(a * b).sum()`` on the
  sliced view.

``bytes`` is what the method has to read (the box once per pass and source), and the share of
8 TB/s is ``bytes / time``. The script also prints, and records, whether ``sum`` and ``dot`` agree
bit for bit with the host restatement on the same fields. Needs a GPU; there is no fallback.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 1024, 160))
    ap.add_argument("--halo", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--no-host-check", action="store_true", help="skip the comparison with the host restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reduce_bench.json"))
    args = ap.parse_args()
    import torch

    import gt4py_amd  # noqa: F401
    from gt4py_amd import storage
    from gt4py_amd.storage import reduce as R

    if not torch.cuda.is_available():
        raise SystemExit("reduce_bench needs a GPU")
    ni, nj, nk = args.shape
    h = args.halo
    full = (ni + 2 * h, nj + 2 * h, nk)
    box = dict(origin=(h, h, 0), domain=(ni, nj, nk))
    gen = torch.Generator(device="cuda").manual_seed(7)

    def field():
        # uniform mantissas over 40 binades, NaN in the halo: a reduction that touches it shows
        st = storage.empty(full, np.float64, backend=BE, aligned_index=(h, h, 0))
        st.fill_(float("nan"))
        vals = torch.rand((ni, nj, nk), dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        vals *= torch.exp2(torch.randint(-20, 21, (ni, nj, nk), device="cuda", generator=gen).to(torch.float64))
        storage.assign(st[h:h + ni, h:h + nj, :], vals)
        return st

    a, b = field(), field()
    va, vb = a[h:h + ni, h:h + nj, :], b[h:h + ni, h:h + nj, :]
    cells = ni * nj * nk
    nbytes = cells * 8
    sc = R.scan(a, **box)
    m, n = sc[0], sc[6]
    methods = {
        "scan": (lambda: R.scan(a, **box), nbytes),
        "fold_sums": (lambda: R.fold_sums(a, m, n, **box), nbytes),
        "sum": (lambda: R.sum(a, **box), 2 * nbytes),
        "dot": (lambda: R.dot(a, b, **box), 4 * nbytes),
        "torch_view_sum": (lambda: va.sum(), nbytes),
        "torch_view_abs_max": (lambda: va.abs().max(), nbytes),
        "torch_isfinite_all": (lambda: torch.isfinite(va).all(), nbytes),
        "torch_mul_sum": (lambda: (va * vb).sum(), 2 * nbytes),
    }
    ms = _interleaved(torch, {k: f for k, (f, _) in methods.items()}, args.seconds)
    result = {"shape": list(args.shape), "halo": h, "dtype": "float64", "device": torch.cuda.get_device_name(0),
              "peak_bytes_per_s": PEAK_BYTES_PER_S, "box_bytes": nbytes, "methods": {}}
    for name, (_, nb) in methods.items():
        result["methods"][name] = _stats(ms[name], nb)
        print(json.dumps({name: result["methods"][name]}), flush=True)
    got_sum, got_dot = float(R.sum(a, **box)), float(R.dot(a, b, **box))
    result["sum"], result["dot"], result["torch_view_sum_value"] = got_sum, got_dot, float(va.sum())
    if not args.no_host_check:
        ha, hb = storage.to_numpy(a), storage.to_numpy(b)
        want_sum, want_dot = float(R.sum(ha, **box)), float(R.dot(ha, hb, **box))
        result["sum_bitwise_equal_to_host"] = bool(np.float64(got_sum).tobytes() == np.float64(want_sum).tobytes())
        result["dot_bitwise_equal_to_host"] = bool(np.float64(got_dot).tobytes() == np.float64(want_dot).tobytes())
        print(f"sum agrees bitwise with the host restatement: {result['sum_bitwise_equal_to_host']} "
              f"({got_sum!r} / {want_sum!r}); dot: {result['dot_bitwise_equal_to_host']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
