#!/usr/bin/env python3
"""Times `Context.connected_components` (whole call and `device_ms`) at connectivities 6 and 26 beside
`scipy.ndimage.label` on the same host: a 256^3 ball mask (one large component), the same ball with 1 % salt noise (many
components), a 512 x 512 x 200 sparse mask and a serpentine at 128^3 (one path through the volume: the longest chains the
unions can meet).  Then the statistics of the one-component case with and without combining within a wave.  One JSON line
per case (`profiles/components.md`).  Medians of `--reps` calls after one warm-up call, with the least and the largest.

    python tools/bench_components.py [--small] [--reps 7]

`--small` divides every extent by 4 (a check of the tool itself)."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import _hip  # noqa: E402

STREAM_BYTES_PER_MS = 5.0e9  # the streaming rate the README quotes: 5.0 TB/s


def ball(n):
    ax = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) + 0.123
    x, y, z = np.meshgrid(ax, ax + 0.2, ax - 0.3, indexing="ij")
    return x * x + y * y + z * z < (0.3 * n) ** 2


def salted(n):
    return ball(n) ^ (np.random.default_rng(1).random((n, n, n)) < 0.01)


def sparse(nx, ny, nz):
    return np.random.default_rng(0).random((nx, ny, nz)) < 1e-3


def serpentine(n):
    """One voxel-wide path: the z-lines with even i and even j in turn, joined at alternating ends."""
    n |= 1  # the last line on the last index
    vol = np.zeros((n, n, n), dtype=bool)
    end, previous = n - 1, None
    for a, i in enumerate(range(0, n, 2)):
        js = list(range(0, n, 2))
        for j in (js if a % 2 == 0 else js[::-1]):
            vol[i, j, :] = True
            if previous is not None:
                vol[(previous[0] + i) // 2, (previous[1] + j) // 2, end] = True
                end = n - 1 - end
            previous = (i, j)
    return vol


def spread(samples):
    s = sorted(samples)
    return {"median": round(s[len(s) // 2], 3), "least": round(s[0], 3), "largest": round(s[-1], 3)}


def timed(fn, reps):
    samples, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        samples.append((time.perf_counter() - t0) * 1e3)
    return spread(samples), out


def main():
    from scipy import ndimage

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    div = 4 if "--small" in sys.argv else 1
    ctx, lib = _hip.default_context(), _hip.load_library()
    cases = [("ball", ball, (256,)), ("ball with 1 % salt noise", salted, (256,)), ("sparse", sparse, (512, 512, 200)),
             ("serpentine", serpentine, (128,))]
    for name, make, extents in cases:
        vol = make(*(e // div for e in extents)).astype(np.int32)
        floor_ms = 8.0 * vol.size / STREAM_BYTES_PER_MS  # the int32 volume read and the int32 labels written once
        for connectivity in (6, 26):
            ctx.connected_components(vol, connectivity)  # warm-up: the pool's blocks
            call, raw = timed(lambda: ctx.connected_components(vol, connectivity), reps)
            quiet = [ctx.connected_components(vol, connectivity, component=False, stats=False) for _ in range(reps)]  # nothing fetched
            device = spread([q["device_ms"] for q in quiet])
            structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
            sci, (want, n) = timed(lambda: ndimage.label(vol, structure), 1 if vol.size > 2 ** 25 else 3)
            print(json.dumps({"case": name, "shape": list(vol.shape), "connectivity": connectivity, "labelled": int(raw["report"][1]),
                              "components": raw["n"], "largest": int(raw["report"][4]), "call_ms": call, "device_ms": device,
                              "retries": sorted(int(q["report"][3]) for q in quiet), "scipy_ms": sci, "floor_ms": round(floor_ms, 4),
                              "device_over_floor": round(device["median"] / floor_ms, 1),
                              "equals_scipy": bool(n == raw["n"] and np.array_equal(want, raw["component"]))}), flush=True)
        if name != "ball":
            continue
        line = {"case": "statistics of the ball, connectivity 6"}
        try:
            for on, tag in ((1, "combined_device_ms"), (0, "separate_device_ms")):
                lib.pf_ccl_combine_stats(on)
                ctx.connected_components(vol, 6, component=False, stats=False)
                line[tag] = spread([ctx.connected_components(vol, 6, component=False, stats=False)["device_ms"] for _ in range(reps)])
        finally:
            lib.pf_ccl_combine_stats(1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
