#!/usr/bin/env python3
"""Farthest-point sampling and ZoomOut on sub-samples, timed:
python tools/bench_fast_zoomout.py [n_vertices] [--full N] [--samples Q] [--reps R] [--commit HASH] [--out FILE]

The pair: blob_mesh(n, seed=0) and the same surface renumbered by a random permutation (so the true map is known), with
the stand-in basis of tools/bench_fmap.py: smooth functions of the vertex position, cos(w_k . x + b_k) with |w_k| growing
with k, made M-orthonormal by a QR factorisation (a Laplace-Beltrami basis of a 250k mesh is beyond what the eigensolver
has been verified for; the kernels' work does not depend on which smooth basis it is).  30 basis functions, 30 % of the
initial map random.  Timed:
  * `farthest_point_sampling` of Q (default 1000) of the n (default 250000) points, upload and download included;
  * `zoomout_refine(samples=...)` 4 -> 30 on Q samples a side at n vertices;
  * the full `zoomout_refine` 4 -> 30 beside the sampled one at --full vertices (default 50000: at 250000 a full round
    scans 6 * 10^10 pairs of rows in up to 30 dimensions, 27 times over; pass --full 250000 to wait for it).
Host clocks around calls that end in a device synchronise; the first call of each is discarded, then the median of R -
except the full loop, which is called once: its time includes whatever first-use cost the sampled calls before it left.
Writes the markdown record (default profiles/fast_zoomout.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _fmap_ref as fr  # noqa: E402
from pyfocusr_amd import _hip, farthest_point_sampling, zoomout_refine  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

args = sys.argv[1:]
opts = {"--full": "50000", "--samples": "1000", "--reps": "3", "--commit": "unknown",
        "--out": os.path.join(REPO, "profiles", "fast_zoomout.md")}
for flag in list(opts):
    if flag in args:
        k = args.index(flag)
        opts[flag] = args[k + 1]
        del args[k:k + 2]
n = int(args[0]) if args else 250000
n_full, q, reps = int(opts["--full"]), int(opts["--samples"]), int(opts["--reps"])
K, K_START = 30, 4
ctx = _hip.default_context()


def timed(fn, r=None):
    fn()  # discarded
    t = []
    for _ in range(r or reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def problem(n_vertices):
    """(target points, source points, phi_t, phi_s, mass_s, T_true)."""
    mesh = blob_mesh(n_vertices, seed=0)
    pts, faces = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.faces)
    e1, e2 = pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]]
    mass = np.bincount(faces.ravel(), np.repeat(0.5 * np.linalg.norm(np.cross(e1, e2), axis=1) / 3.0, 3), n_vertices)
    rng = np.random.default_rng(5)
    w = rng.normal(size=(3, K))
    w *= (0.02 + 0.3 * np.sqrt(np.arange(K) / K)) / np.linalg.norm(w, axis=0)
    raw = np.cos(pts @ w + rng.uniform(0, 2 * np.pi, K))
    raw[:, 0] = 1.0
    qr, _ = np.linalg.qr(raw * np.sqrt(mass)[:, None])
    phi_t = np.ascontiguousarray(qr / np.sqrt(mass)[:, None])
    perm = rng.permutation(n_vertices)
    T_true = np.empty(n_vertices, dtype=np.int64)
    T_true[perm] = np.arange(n_vertices)
    return pts, np.ascontiguousarray(pts[T_true]), phi_t, np.ascontiguousarray(phi_t[T_true]), mass[T_true], T_true


def matched(T, T_true):
    return "%.2f %%" % (100.0 * np.mean(T == T_true))


lines = ["# Farthest-point sampling and ZoomOut on sub-samples (`pf_fps.hip`, `pf_fmap.hip`)", "",
         "`python tools/bench_fast_zoomout.py %d --full %d --samples %d --reps %d` on one MI355X, commit %s.  A blob and its "
         "renumbered copy, a stand-in basis of %d smooth M-orthonormal functions (see the tool's header: not the eigensolver's), "
         "30 %% of the initial map random, ZoomOut %d -> %d with step 1.  Host clocks around synchronising calls (uploads and "
         "downloads included), first call discarded, median of %d; the full loop: one call." % (n, n_full, q, reps, opts["--commit"], K, K_START, K, reps),
         "", "| call | vertices | samples a side | ms | vertices at their true match | remark |", "|---|---|---|---|---|---|"]


def row(*cells):
    lines.append("| " + " | ".join(str(c) for c in cells) + " |")
    print(lines[-1], flush=True)


def sampled_rows(n_vertices, with_full):
    pt, ps, phi_t, phi_s, mass_s, T_true = problem(n_vertices)
    T0 = fr.corrupt(T_true, 0.3)
    m = min(q, n_vertices)
    ms = timed(lambda: farthest_point_sampling(pt, m, ctx=ctx))
    S_t, d2 = farthest_point_sampling(pt, m, return_d2=True, ctx=ctx)
    S_s = farthest_point_sampling(ps, m, ctx=ctx)
    row("`farthest_point_sampling`", n_vertices, m, "%.2f" % ms, "", "covering radius %.4g" % np.sqrt(d2.max()))
    ms = timed(lambda: zoomout_refine(phi_t, phi_s, mass_s, T0, K_START, K, samples=(S_t, S_s), ctx=ctx))
    T, C = zoomout_refine(phi_t, phi_s, mass_s, T0, K_START, K, samples=(S_t, S_s), ctx=ctx)
    row("`zoomout_refine(samples=...)`", n_vertices, m, "%.1f" % ms, matched(T, T_true),
        "max \\|\\|C\\| - I\\| = %.2g" % np.max(np.abs(np.abs(C) - np.eye(K))))
    if with_full:
        t0 = time.perf_counter()
        T, C = zoomout_refine(phi_t, phi_s, mass_s, T0, K_START, K, ctx=ctx)
        ms = 1e3 * (time.perf_counter() - t0)
        row("`zoomout_refine`, every vertex", n_vertices, "", "%.1f" % ms, matched(T, T_true),
            "one call; max \\|\\|C\\| - I\\| = %.2g" % np.max(np.abs(np.abs(C) - np.eye(K))))


sampled_rows(n, with_full=(n_full == n))
if n_full != n:
    sampled_rows(n_full, with_full=True)
    lines += ["", "The full loop was not run at %d vertices: it is timed at %d, with the sampled loop at that size beside it." % (n, n_full)]
text = "\n".join(lines) + "\n"
with open(opts["--out"], "w") as fh:
    fh.write(text)
print(text)
