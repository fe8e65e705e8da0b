#!/usr/bin/env python3
"""Times `Context.distance_transform` (whole call and `device_ms`, unsigned and signed) beside
`scipy.ndimage.distance_transform_edt` on the same host: a 256^3 ball mask, a 512 x 512 x 200 sparse mask and the worst
case of the outward search, a single feature in a corner of 256^3; then the hand-over of the resident field to the
isosurface beside the round trip through the host.  One JSON line per case (`profiles/distance_transform.md`).

    python tools/bench_distance_transform.py [--small] [--reps 5]

`--small` divides every extent by 4 (a check of the tool itself)."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import _hip  # noqa: E402

SPACING = (0.5, 0.5, 1.25)


def ball(n):
    ax = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) + 0.123
    x, y, z = np.meshgrid(ax, ax + 0.2, ax - 0.3, indexing="ij")
    return x * x + y * y + z * z < (0.3 * n) ** 2


def sparse(nx, ny, nz):
    return np.random.default_rng(0).random((nx, ny, nz)) < 1e-3


def corner(n):
    mask = np.zeros((n, n, n), dtype=bool)
    mask[0, 0, 0] = True
    return mask


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    from scipy import ndimage

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    div = 4 if "--small" in sys.argv else 1
    ctx = _hip.default_context()
    cases = [("ball", ball, (256,)), ("sparse", sparse, (512, 512, 200)), ("corner", corner, (256,))]
    for name, make, extents in cases:
        mask = make(*(e // div for e in extents))
        line = {"case": name, "shape": list(mask.shape), "foreground": int(mask.sum()), "spacing": list(SPACING)}
        for signed in (False, True):
            ctx.distance_transform(mask, SPACING, signed=signed)  # warm-up: the pool's blocks
            ms, raw = timed(lambda: ctx.distance_transform(mask, SPACING, signed=signed), reps)
            # the device time alone: nothing fetched
            dev = min(ctx.distance_transform(mask, SPACING, signed=signed, dist=False, dist2=False, nearest=False)["device_ms"]
                      for _ in range(reps))
            tag = "signed" if signed else "unsigned"
            line.update({tag + "_call_ms": round(ms, 2), tag + "_device_ms": round(dev, 3)})
            if not signed:
                scipy_ms, want = timed(lambda: ndimage.distance_transform_edt(~mask, sampling=SPACING), 1)
                line.update(scipy_ms=round(scipy_ms, 1),
                            largest_relative_difference=float(np.max(np.abs(raw["dist"] - want) / np.maximum(want, 1e-300))))
        print(json.dumps(line), flush=True)
        if name != "ball":
            continue
        # the margin at 3 units: the resident field straight into the isosurface, and the same through the host
        origin = np.zeros(3)

        def resident():
            with _hip.DeviceDistanceTransform(mask, SPACING, signed=True, ctx=ctx) as edt:
                with edt.isosurface(3.0, origin) as iso:
                    return iso.fetch()

        def round_trip():
            dist = ctx.distance_transform(mask, SPACING, signed=True, dist2=False, nearest=False)["dist"]
            return ctx.isosurface(dist, 3.0, SPACING, origin)

        resident(), round_trip()
        a_ms, a = timed(resident, reps)
        b_ms, b = timed(round_trip, reps)
        print(json.dumps({"case": "ball margin 3.0", "vertices": int(len(a[0])), "resident_ms": round(a_ms, 2), "round_trip_ms": round(b_ms, 2),
                          "same_bytes": bool(a[0].tobytes() == b["points"].tobytes() and a[1].tobytes() == b["faces"].tobytes())}), flush=True)


if __name__ == "__main__":
    main()
