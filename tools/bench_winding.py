#!/usr/bin/env python3
"""Winding-number timing on a synthetic pair: python tools/bench_winding.py [n_vertices] [--reps R] [--betas 2,4,8]
[--host-queries Q]

A blob_mesh pair (seeds 0 and 1): every vertex of mesh 0 against the surface of mesh 1.  Times
`pf_surface_prepare_winding` (a fresh surface each time) and `pf_surface_winding` in exact mode and for each beta: host
clock around calls that end in a device synchronise (each call uploads the queries, sorts them, runs the kernel and
downloads w and the bound), one warm-up call, then R calls: median, minimum and maximum.  Per mode also
max |w - w_exact|, the largest returned bound, and how many inside / outside decisions (w > 0.5) differ from exact mode.
Last, the numpy reference of the tests on the host for the first Q queries (default 200; 0 skips it), scaled to the full
query count for comparison.  Prints markdown tables (the record in profiles/winding_number.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402


def option(args, name, default, cast):
    if name in args:
        k = args.index(name)
        value = cast(args[k + 1])
        del args[k:k + 2]
        return value
    return default


args = sys.argv[1:]
reps = option(args, "--reps", 5, int)
betas = option(args, "--betas", [2.0, 4.0, 8.0], lambda s: [float(x) for x in s.split(",")])
host_queries = option(args, "--host-queries", 200, int)
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


def prepare_once(mesh):
    s = _hip.DeviceSurface(mesh.points, mesh.faces, ctx=ctx)
    t0 = time.perf_counter()
    _hip._check(s._lib.pf_surface_prepare_winding(s._h))
    t = time.perf_counter() - t0
    s.close()
    return t


a, b = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
q = a.points
prepare_once(b)  # warm-up
t_prep = 1e3 * float(np.median([prepare_once(b) for _ in range(reps)]))
surf = _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
print("%d queries against %d triangles (%.3g solid angles in exact mode); pf_surface_prepare_winding %.3f ms; %d timed calls "
      "per mode\n" % (len(q), len(b.faces), float(len(q)) * len(b.faces), t_prep, reps))
print("| mode | call ms (median) | min | max | exact / mode | max abs(w - w_exact) | max bound | decisions that differ |")
print("|---|---|---|---|---|---|---|---|")
w_exact, _ = surf.winding_number(q)
t_exact = None
for beta in [0.0] + betas:
    med, lo, hi = timed(lambda: surf.winding_number(q, beta=beta))
    w, bound = surf.winding_number(q, beta=beta)
    if t_exact is None:
        t_exact = med
    print("| %s | %.2f | %.2f | %.2f | %.1fx | %.3e | %.3e | %d |"
          % ("exact" if beta <= 0 else "beta = %g" % beta, med, lo, hi, t_exact / med, np.max(np.abs(w - w_exact)), bound.max(),
             int(np.sum((w > 0.5) != (w_exact > 0.5)))), flush=True)
surf.close()

if host_queries > 0:
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _signed_ref  # noqa: E402

    sub = q[:host_queries]
    t0 = time.perf_counter()
    w_host = _signed_ref.winding_number(b.points, b.faces, sub)
    t_host = time.perf_counter() - t0
    print("\nnumpy reference on the host: %d queries against the same %d triangles in %.2f s (max |w_exact - w_host| = %.2e); "
          "scaled to %d queries: %.0f s, exact mode on the device is %.0fx faster"
          % (len(sub), len(b.faces), t_host, np.max(np.abs(w_exact[:len(sub)] - w_host)), len(q), t_host * len(q) / len(sub),
             t_host * len(q) / len(sub) / (1e-3 * t_exact)))
