#!/usr/bin/env python3
"""Times mesh smoothing (`pyfocusr_amd.smoothing`, `pf_smoother_*`): 20 Taubin iterations (40 sweeps, uniform weights,
fixed boundary) on the isosurface of the 256^3 sphere distance field of `profiles/isosurface.md` and on a 250k blob; one
JSON line per case (`profiles/smoothing.md`).

    python tools/bench_smoothing.py [--small] [--reps 5]

Per case: the build of the smoother, the whole call of `smooth_points` (with the stats), the device time of the 40 sweeps
alone, the time per sweep against the bytes a sweep must move - 48 B per vertex for reading and writing x, 4 B per entry
for the columns, 4 B + 1 B per vertex for the row starts and kinds; `gather_bytes` is what the gathered rows add when no
cache helps (24 B per entry) - and the same smoothing in scipy.sparse on the same host (a row-normalised CSR matrix, one
product per sweep), whose result is compared with the device's.  `--small` runs a 64^3 field and a 20k blob (a check of the
tool itself)."""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import MeshSmoother, _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402
from pyfocusr_amd.smoothing import taubin_mu  # noqa: E402

ITERATIONS, LAM, PASS_BAND = 20, 0.5, 0.1


def sphere_mesh(ctx, n):
    ax = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) + 0.123
    x, y, z = np.meshgrid(ax, ax + 0.2, ax - 0.3, indexing="ij")
    raw = ctx.isosurface(np.sqrt(x * x + y * y + z * z) - 0.4 * n, 0.0)
    return raw["points"], raw["faces"]


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def host_smoothing(pts, rowptr, col, kind, factors):
    """The same sweeps in scipy.sparse: x <- x + f (A x - x) at the movable rows, A the row-normalised adjacency."""
    n = len(pts)
    length = np.diff(rowptr).astype(np.float64)
    movable = (kind & 4) != 0
    inv = np.where(movable, 1.0 / np.maximum(length, 1.0), 0.0)
    A = sp.csr_matrix((np.repeat(inv, np.diff(rowptr)), col, rowptr), shape=(n, n))
    keep = movable[:, None]
    x = pts.copy()
    for f in factors:
        x = np.where(keep, x + f * (A @ x - x), x)
    return x


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    small = "--small" in sys.argv
    ctx = _hip.default_context()
    factors = np.tile(np.array([LAM, taubin_mu(LAM, PASS_BAND)]), ITERATIONS)
    blob = blob_mesh(20000 if small else 250000, seed=0)
    cases = [("sphere256" if not small else "sphere64", sphere_mesh(ctx, 64 if small else 256)), ("blob", (blob.points, blob.faces))]
    for name, (pts, faces) in cases:
        MeshSmoother((pts, faces), ctx=ctx).close()  # warm-up: the pool's blocks
        build_ms, sm = timed(lambda: MeshSmoother((pts, faces), ctx=ctx), reps)
        call_ms, (out, info) = timed(lambda: sm.smooth_points(ITERATIONS, "taubin", LAM, PASS_BAND, return_info=True), reps)
        sweeps_ms = min(sm._device.run(None, factors, 2, None, False)[2] for _ in range(reps))
        with_stats_ms = min(sm._device.run(None, factors, 2, None, True)[2] for _ in range(reps))
        rowptr, col, _, kind = sm.adjacency()
        counts = sm.info
        sm.close()
        host_ms, host = timed(lambda: host_smoothing(pts, rowptr, col, kind, factors), 1)
        n, nnz = len(pts), int(counts["entries"])
        must, gather = 48 * n + 4 * nnz + 5 * n, 24 * nnz
        per_sweep_us = 1e3 * sweeps_ms / len(factors)
        print(json.dumps({"case": name, "vertices": n, "faces": int(len(faces)), "entries": nnz, "largest_row": int(counts["largest_row"]),
                          "sweeps": len(factors), "build_ms": round(build_ms, 3), "call_ms": round(call_ms, 3),
                          "device_sweeps_ms": round(sweeps_ms, 4), "device_with_stats_ms": round(with_stats_ms, 4),
                          "per_sweep_us": round(per_sweep_us, 2), "must_bytes": must, "gather_bytes": gather,
                          "must_GBps": round(must / per_sweep_us / 1e3, 1), "with_gather_GBps": round((must + gather) / per_sweep_us / 1e3, 1),
                          "volume_ratio": info.volume_out / info.volume_in, "scipy_ms": round(host_ms, 1),
                          "max_abs_difference_to_scipy": float(np.max(np.abs(out - host)))}))


if __name__ == "__main__":
    main()
