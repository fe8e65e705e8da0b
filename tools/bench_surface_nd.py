#!/usr/bin/env python3
"""Closest surface point in spectral coordinates, timed: python tools/bench_surface_nd.py [n_vertices] [--reps R] [--out FILE]

A blob_mesh pair (seeds 0 and 1) goes through `Focusr` (no ICP, no CPD, ten weighted spectral coordinates) once; the
leading d = 3, 5, 10 of those coordinates are the spaces searched.  Every source vertex is a query against the target's
spectral surface: `pf_surface_nd_closest` pruned, the chunks it staged, the exhaustive mode on a subset of the queries
(scaled up to all of them), and for context `pf_surface_distance` at d = 3 and the 1-NN vertex search at the same d.
Host clocks around calls that end in a device synchronise; the first call of each is discarded, then the median of R.
Writes the markdown record (default profiles/spectral_surface.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import Focusr, _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

args = sys.argv[1:]
reps, out_path = 5, os.path.join(REPO, "profiles", "spectral_surface.md")
for flag in ("--reps", "--out"):
    if flag in args:
        k = args.index(flag)
        if flag == "--reps":
            reps = int(args[k + 1])
        else:
            out_path = args[k + 1]
        del args[k:k + 2]
n = int(args[0]) if args else 250000
SUBSET = 2048
ctx = _hip.default_context()


def timed(fn):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


target, source = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
reg = Focusr(target, source, icp_register_first=False, n_spectral_features=10, n_extra_spectral=0,
             n_coords_spectral_ordering=20000, list_features_to_calc=[], return_average_final_points=False,
             smooth_correspondences=False, ctx=ctx, registration=lambda src, tgt, kind: tgt)
reg.align_maps()
tgt_all, src_all = np.asarray(reg.target_spectral_coords), np.asarray(reg.source_spectral_coords)
faces = np.ascontiguousarray(target.faces, dtype=np.int32)

lines = ["# Closest surface point in spectral coordinates (`pf_surface_nd_closest`)", "",
         "`python tools/bench_surface_nd.py %d --reps %d` on one MI355X: blob_mesh pair, %d target vertices, %d triangles "
         "(%d chunks of 64), %d source vertices as queries, the leading d of ten weighted spectral coordinates.  Host "
         "clocks around synchronising calls (uploads and downloads included), first call discarded, median of %d.  "
         "`chunks / packet`: chunks staged per packet of 8 neighbouring queries, the mean over the packets (every query "
         "of a packet sees them).  `exhaustive`: the time of %d queries with pruning off, scaled to all queries."
         % (n, reps, len(tgt_all), len(faces), (len(faces) + 63) // 64, len(src_all), reps, SUBSET), "",
         "| d | build ms | pruned ms | chunks / packet | exhaustive ms (scaled) | exhaustive / pruned | same bits on the subset "
         "| 1-NN vertex search ms | strictly closer than the vertex | `pf_surface_distance` ms | same d2, faces |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
for d in (3, 5, 10):
    tgt, src = np.ascontiguousarray(tgt_all[:, :d]), np.ascontiguousarray(src_all[:, :d])
    t_build = timed(lambda: _hip.DeviceSurfaceND(tgt, faces, ctx=ctx).close())
    with _hip.DeviceSurfaceND(tgt, faces, ctx=ctx) as surface:
        t_pruned = timed(lambda: surface.closest(src))
        face, verts, bary, d2 = surface.closest(src)
        stats = surface.last_search()
        sub = src[:: max(1, len(src) // SUBSET)][:SUBSET]
        t_ex = timed(lambda: surface.closest(sub, exhaustive=True)) * len(src) / len(sub)
        ex, pr = surface.closest(sub, exhaustive=True), surface.closest(sub)
        same = all(a.tobytes() == b.tobytes() for a, b in zip(ex, pr))
    t_knn = timed(lambda: ctx.knn1(tgt, src))
    idx = ctx.knn1(tgt, src)
    diff = src - tgt[idx]
    closer = float(np.mean(d2 < np.sum(diff * diff, axis=1)))
    t_dist, same3 = "", ""
    if d == 3:
        s3 = _hip.DeviceSurface(tgt, faces, ctx=ctx)
        t_dist = "%.2f" % timed(lambda: s3.distance(src))
        d2_3, face_3, _ = s3.distance(src)
        s3.close()
        same3 = "yes" if d2_3.tobytes() == d2.tobytes() and np.array_equal(face_3, face) else "NO"
    lines.append("| %d | %.2f | %.2f | %.1f | %.0f | %.0fx | %s | %.2f | %.1f %% | %s | %s |"
                 % (d, t_build, t_pruned, stats["chunks_opened"] / stats["packets"], t_ex, t_ex / t_pruned,
                    "yes" if same else "NO", t_knn, 100.0 * closer, t_dist, same3))
    print(lines[-1], flush=True)
text = "\n".join(lines) + "\n"
with open(out_path, "w") as fh:
    fh.write(text)
print(text)
