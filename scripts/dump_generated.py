#!/usr/bin/env python3
"""Write the HIP text the generator emits for every stencil the tests and the bench build.

    python scripts/dump_generated.py OUTDIR

Pure CPU, no hipcc: each item goes through ``backend.mi355x_backend.generate_source``. Per item and
option set one ``OUTDIR/<item>__<opts>.hip`` (or ``.err`` with the message when generation raises
``UnsupportedStencil`` or ``ValueError``), plus ``OUTDIR/MANIFEST``, the sorted ``sha256  name``
list. Two trees generate the same libraries exactly when ``diff -r`` of their dumps is empty (the
JIT cache key is a hash of the source). Golden cases and bench configs are also dumped under every
non-default value of the versioned backend options.
"""

import hashlib
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

# one file per non-default value (golden cases and bench configs)
OPTION_VALUES = {
    "order": [0, 1, 2, 3, 4, 5], "nt_load": [0, 2], "nt_store": [0], "dpp": [0], "vector": [1, 2, 4],
    "prefetch": [0, 1, 3], "jchunk": [4, 8], "jmirror": [0], "row_unroll": [0, 3, 4], "bufld": [0, 1],
    "strip_align": [0], "min_blocks": [2], "pointwise_plane": [0], "fuse": [0], "exact_fma": [0],
    "kring": [0, 1, 4], "ktail_lds": [0], "ktail_all": [1], "kreg": [0, 40, 96],
    "ktail_head": [0, 1], "col_bx": [128, 256], "col_order": [0], "tile": [0], "tile_order": [1, 2],
    "tile_lblock": [1, 4], "tile_rows": [2],
}
VARIANTS = [{k: v} for k, vs in OPTION_VALUES.items() for v in vs]
REFUSED = [{"tile_rows": 3}, {"tile_ti": 4}, {"tile_by": 32}]  # tile programs: the messages (.err) are compared too
VARIANTS += [{"kreg": r, "kreg_pf": pf} for r in (40, 96) for pf in (0, 6, 50)] + [{"kreg_pf": pf} for pf in (0, 6, 50)]


def items():
    """(item name, definition, externals, [option sets])."""
    import numpy as np

    import bench
    import frontend_cases as fc
    import golden_utils
    import stencil_cases as sc
    import test_fuzz
    import test_fusion as tf
    import test_gpu_parity as tg
    import test_tile as tt

    for name in golden_utils.available():
        case = sc.CASES[name]
        opts = [{}] + VARIANTS
        if name in tg.COLUMN_OPT_CASES:
            opts += tg.COLUMN_OPTS
        if name in tt.GEOM_GOLDEN:
            opts += [tt.geom_opts(g) for g in tt.GEOMS]
        yield f"golden.{name}", case.definition, case.externals, opts
    defs = bench.stencil_defs()
    for cfg in sorted(bench.CONFIGS):
        sname, dtype = bench.CONFIGS[cfg][:2]
        yield f"bench.{cfg}", defs[(sname, dtype)], bench.EXTERNALS.get(sname, {}), [{}] + VARIANTS
    with tempfile.TemporaryDirectory() as d:
        for seed in test_fuzz.SEEDS:
            yield f"fuzz.{seed}", test_fuzz._load(seed, d)[0], {}, [test_fuzz._opts(seed)]
    with open(os.path.join(REPO, "tests", "golden", "frontend", "verdicts.json")) as f:
        accepted = sorted(n for n, v in json.load(f).items() if v["accepted"])
    for name in accepted:
        defn, externals = fc.CASES[name]
        yield f"frontend.{name}", defn, externals, [{}]
    for name, (defn, *_rest) in tf.CASES.items():
        yield f"fusion.{name}", defn, {}, [{}]
    yield "fusion.hdiff_blocks.full", tf.hdiff_blocks, {}, [{}]
    for name in sorted(tt.CASES):
        yield f"tile.{name}", tt.CASES[name][0], {}, [{}] + [tt.geom_opts(g) for g in tt.GEOMS] + REFUSED
    yield "parity.hdiff_ragged", sc.hdiff_f64, {}, tg.RAGGED_CHUNK_OPTS
    for dt, defn in ((np.float64, sc.hdiff_f64), (np.float32, sc.hdiff_f32)):
        yield f"parity.hdiff_bufld_{np.dtype(dt).name}", defn, {}, tg.BUFLD_OPTS


def main():
    from gt4py_amd.backend.base import from_name
    from gt4py_amd.backend.mi355x_backend import generate_source
    from gt4py_amd.codegen.plan import UnsupportedStencil
    from gt4py_amd.definitions import BuildOptions
    from gt4py_amd.loader import StencilBuilder

    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    manifest = {}
    for item, defn, externals, optsets in items():
        b = StencilBuilder(defn, from_name("gt:mi355x"), BuildOptions(name=f"dump.{item}", module="dump"), externals, {})
        for opts in optsets:
            tag = "_".join(f"{k}{v}" for k, v in opts.items()) or "default"
            try:
                text, ext = generate_source(b.analysis, dict(opts))[1], "hip"
            except (UnsupportedStencil, ValueError) as e:
                text, ext = f"{type(e).__name__}: {e}\n", "err"
            fname = f"{item}__{tag}.{ext}"
            if fname in manifest:
                continue  # an option set listed twice
            with open(os.path.join(out, fname), "w") as f:
                f.write(text)
            manifest[fname] = hashlib.sha256(text.encode()).hexdigest()
    with open(os.path.join(out, "MANIFEST"), "w") as f:
        f.writelines(f"{h}  {n}\n" for n, h in sorted(manifest.items()))
    print(f"{len(manifest)} files ({sum(n.endswith('.err') for n in manifest)} .err) in {out}")


if __name__ == "__main__":
    main()
