#!/usr/bin/env python3
"""Surface-distance timing on synthetic pairs: python tools/bench_surface_distance.py [n_vertices ...] [--reps R] [--signed]

For each size a blob_mesh pair (seeds 0 and 1): the surface build, `pf_surface_distance` in both directions (every
vertex of one mesh against the other's surface; per-point outputs downloaded, and stats only), and
`pf_surface_closest` on the same full query set.  Host clocks around calls that end in a device synchronise, after one
warm-up call of each; the median of R calls.  Prints a markdown table (the record in profiles/surface_distance.md).

--signed instead times the signed structure (`pf_surface_prepare_signed`, on a fresh surface each time) and
`pf_surface_signed_distance` in both directions against the unsigned call, and checks |sd| against sqrt(d2)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyfocusr_amd import _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

args = sys.argv[1:]
reps = 5
if "--reps" in args:
    k = args.index("--reps")
    reps = int(args[k + 1])
    del args[k:k + 2]
signed = "--signed" in args
if signed:
    args.remove("--signed")
sizes = [int(a) for a in args] or [15000, 250000]
ctx = _hip.default_context()


def timed(fn):
    fn()  # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))




def prepare_once(mesh):
    s = _hip.DeviceSurface(mesh.points, mesh.faces, ctx=ctx)
    t0 = time.perf_counter()
    s._prepare_signed()
    t = time.perf_counter() - t0
    s.close()
    return t


if signed:
    print("| vertices | triangles | prepare ms | unsigned a->b ms | signed a->b ms | signed / unsigned | unsigned b->a ms "
          "| signed b->a ms | signed / unsigned | |sd| = sqrt(d2), same faces |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for n in sizes:
        a, b = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
        prepare_once(b)  # warm-up
        t_prep = 1e3 * float(np.median([prepare_once(b) for _ in range(reps)]))
        sa, sb = _hip.DeviceSurface(a.points, a.faces, ctx=ctx), _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
        row = []
        same = True
        for s, q in ((sb, a.points), (sa, b.points)):
            t_u = timed(lambda: s.distance(q))
            t_s = timed(lambda: s.signed_distance(q))
            d2, face, _ = s.distance(q)
            sd, sface, _, _ = s.signed_distance(q)
            same = same and np.array_equal(np.abs(sd), np.sqrt(d2)) and np.array_equal(sface, face)
            row += [t_u, t_s, t_s / t_u]
        sa.close()
        sb.close()
        print("| %d | %d | %.2f | %.3f | %.3f | %.2fx | %.3f | %.3f | %.2fx | %s |"
              % ((n, len(b.faces), t_prep) + tuple(row) + ("yes" if same else "NO",)), flush=True)
    sys.exit(0)

print("| vertices | triangles | build ms | distance a->b ms | distance b->a ms | a->b stats only ms | closest a->b ms "
      "| closest / distance | same d2, faces |")
print("|---|---|---|---|---|---|---|---|---|")
for n in sizes:
    a, b = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
    t_build = timed(lambda: _hip.DeviceSurface(b.points, b.faces, ctx=ctx).close())
    sa, sb = _hip.DeviceSurface(a.points, a.faces, ctx=ctx), _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
    t_ab = timed(lambda: sb.distance(a.points))
    t_ba = timed(lambda: sa.distance(b.points))
    t_stats = timed(lambda: sb.distance(a.points, per_point=False))
    t_closest = timed(lambda: sb.closest(a.points))
    d2, face, _ = sb.distance(a.points)
    _, want_face, want_d2 = sb.closest(a.points)
    same = np.array_equal(d2, want_d2) and np.array_equal(face, want_face)
    sa.close()
    sb.close()
    print("| %d | %d | %.2f | %.3f | %.3f | %.3f | %.3f | %.1fx | %s |"
          % (n, len(b.faces), t_build, t_ab, t_ba, t_stats, t_closest, t_closest / t_ab, "yes" if same else "NO"),
          flush=True)
