#!/usr/bin/env python3
"""Times `Context.isosurface` (whole call and `device_ms`) beside the vectorised numpy reference of
tests/_isosurface_ref.py, on a 256^3 sphere distance field and a 512 x 512 x 200 mask; one JSON line per case
(`profiles/isosurface.md`).

    python tools/bench_isosurface.py [--small] [--reps 5]

The reference runs on a grid coarser by 4 per axis (64 times fewer samples) and its time is reported as measured, with
the factor beside it: it is not scaled.  `--small` runs both on the coarse grids only (a check of the tool itself)."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _isosurface_ref as ref  # noqa: E402
from pyfocusr_amd import _hip  # noqa: E402


def sphere(n):
    ax = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) + 0.123
    x, y, z = np.meshgrid(ax, ax + 0.2, ax - 0.3, indexing="ij")
    return np.sqrt(x * x + y * y + z * z) - 0.4 * n, 0.0


def mask(nx, ny, nz):
    x, y, z = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), np.linspace(-1, 1, nz), indexing="ij")
    solid = ((x / 0.8) ** 2 + (y / 0.6) ** 2 + (z / 0.9) ** 2 < 1.0) & ~((x - 0.2) ** 2 + y ** 2 < 0.05)
    return -solid.astype(np.float64), -0.5  # `inside="above"` of the mask at 0.5, as mask_to_mesh passes it


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    small = "--small" in sys.argv
    ctx = _hip.default_context()
    cases = [("sphere", sphere, (256,), (64,)), ("mask", mask, (512, 512, 200), (128, 128, 50))]
    for name, make, full, coarse in cases:
        values, level = make(*(coarse if small else full))
        ctx.isosurface(values, level)  # warm-up: the pool's blocks
        ms, raw = timed(lambda: ctx.isosurface(values, level), reps)
        dev = min(ctx.isosurface(values, level)["device_ms"] for _ in range(reps))
        cvalues, clevel = make(*coarse)
        ref_ms, want = timed(lambda: ref.isosurface_ref(cvalues, clevel), 1)
        craw = raw if small else ctx.isosurface(cvalues, clevel)
        same = all(np.array_equal(craw[k], w) for k, w in zip(("points", "faces", "vertex_key", "face_cell"), want))
        print(json.dumps({"case": name, "shape": list(values.shape), "vertices": int(raw["report"][0]), "faces": int(raw["report"][1]),
                          "crossing_cells": int(raw["report"][2]), "call_ms": round(ms, 3), "device_ms": round(dev, 4),
                          "volume_bytes": int(values.nbytes), "reference_shape": list(cvalues.shape), "reference_ms": round(ref_ms, 1),
                          "reference_samples_factor": int(values.size // cvalues.size), "coarse_equal_to_reference": bool(same)}))


if __name__ == "__main__":
    main()
