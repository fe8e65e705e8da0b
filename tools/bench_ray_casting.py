#!/usr/bin/env python3
"""Ray casting timing on a synthetic pair: python tools/bench_ray_casting.py [n_vertices] [--reps R] [--host-rays Q]

A blob_mesh pair (seeds 0 and 1): the rays start at every vertex of mesh 0 and run along its inward unit normals
(`vertex_normals`) against the surface of mesh 1: across the interior to the far side, for the vertices outside mesh 1
through its near side first.  Times `pf_surface_raycast` in first-hit mode and in count mode, and next to them `pf_surface_distance` from the
same origins to the same surface: host clock around calls that end in a device synchronise (each call uploads its
inputs, sorts them, runs the kernel and downloads the outputs), one warm-up call, then R calls: median, minimum and
maximum.  Also the outward rays (from outside mesh 1 a miss, from inside its near side).  Last, the numpy
reference of the tests on the host for the first Q rays (default 64; 0 skips it), compared bit for bit and scaled to the
full ray count.  Prints markdown tables (the record in profiles/ray_casting.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402
from pyfocusr_amd.ray_casting import vertex_normals  # noqa: E402


def option(args, name, default, cast):
    if name in args:
        k = args.index(name)
        value = cast(args[k + 1])
        del args[k:k + 2]
        return value
    return default


args = sys.argv[1:]
reps = option(args, "--reps", 5, int)
host_rays = option(args, "--host-rays", 64, int)
n = int(args[0]) if args else 250000
ctx = _hip.default_context()


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t), 1e3 * max(t)


a, outer = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
origins = a.points
normals = vertex_normals(a, ctx=ctx)
surf = _hip.DeviceSurface(outer.points, outer.faces, ctx=ctx)
print("%d rays against %d triangles; %d timed calls per row\n" % (len(origins), len(outer.faces), reps))
print("| call | ms (median) | min | max | Mrays/s | rays that hit | crossings per ray (mean) |")
print("|---|---|---|---|---|---|---|")
for label, d in (("inward", -normals), ("outward", normals)):
    t, _, _, count = surf.raycast(origins, d, count=True)
    for mode, fn in (("first hit", lambda: surf.raycast(origins, d)), ("first hit + count", lambda: surf.raycast(origins, d, count=True))):
        med, lo, hi = timed(fn)
        print("| raycast %s, %s | %.2f | %.2f | %.2f | %.1f | %d | %.3f |"
              % (label, mode, med, lo, hi, 1e-3 * len(origins) / med, int(np.isfinite(t).sum()), float(count.mean())), flush=True)
med, lo, hi = timed(lambda: surf.distance(origins))
print("| pf_surface_distance, same origins | %.2f | %.2f | %.2f | %.1f | | |" % (med, lo, hi, 1e-3 * len(origins) / med), flush=True)
t_dev = timed(lambda: surf.raycast(origins, -normals, count=True))[0]
got = surf.raycast(origins[:max(host_rays, 1)], -normals[:max(host_rays, 1)], count=True)
surf.close()

if host_rays > 0:
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _ray_ref  # noqa: E402

    t0 = time.perf_counter()
    want = _ray_ref.cast(outer.points, outer.faces, origins[:host_rays], -normals[:host_rays], block=16)
    t_host = time.perf_counter() - t0
    same = all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    print("\nnumpy reference on the host: %d inward rays against the same %d triangles in %.2f s, %s the device's t, face, uv "
          "and count; scaled to %d rays: %.0f s, first hit + count on the device is %.0fx faster"
          % (host_rays, len(outer.faces), t_host, "bit for bit" if same else "DIFFERENT FROM", len(origins),
             t_host * len(origins) / host_rays, t_host * len(origins) / host_rays / (1e-3 * t_dev)))
