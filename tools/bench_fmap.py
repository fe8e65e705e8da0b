#!/usr/bin/env python3
"""Functional maps and ZoomOut, timed: python tools/bench_fmap.py [n_vertices] [--reps R] [--host N] [--out FILE]

The pair: blob_mesh(n, seed=0) and the same surface renumbered by a random permutation (so the true map is known).  A
Laplace-Beltrami basis of 128 functions of a 250k mesh is beyond what the eigensolver has been verified for, so the basis
here is a stand-in with the same structure: 128 smooth functions of the vertex position, cos(w_k . x + b_k) with |w_k|
growing with k, made M-orthonormal (M = the lumped vertex areas) by a QR factorisation; the source's basis is the
target's at the matching vertices.  Timed: `pf_knn1_wide` at d = 20, 32, 64, 128 (queries = the source's rows, with the
count of coordinate pairs it evaluated, early exit included, and at d = 128 also on unrelated normal clouds, where
nothing can be dropped), one projection at k = 32, ZoomOut 4 -> 32 from a map with 30 % random entries; and the same
calls through tests/_fmap_ref.py on the host at --host vertices (default 1500), with the device at that size beside
them.  Host clocks around calls that end in a device synchronise; the first call of each is discarded, then the median
of R (the host reference: one call).  FP64 rate: 3 floating-point operations per coordinate pair evaluated, against the
78.6 TFLOP/s vector peak (which counts a fused multiply-add as two; the search's separate subtract, multiply and add can
reach half of it).
Writes the markdown record (default profiles/functional_maps.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _fmap_ref as fr  # noqa: E402
from pyfocusr_amd import _hip, zoomout_refine  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

FP64_VALU_PEAK_TFLOPS = 78.6
args = sys.argv[1:]
reps, n_host, out_path = 3, 1500, os.path.join(REPO, "profiles", "functional_maps.md")
for flag in ("--reps", "--host", "--out"):
    if flag in args:
        k = args.index(flag)
        if flag == "--reps":
            reps = int(args[k + 1])
        elif flag == "--host":
            n_host = int(args[k + 1])
        else:
            out_path = args[k + 1]
        del args[k:k + 2]
n = int(args[0]) if args else 250000
K = 128
ctx = _hip.default_context()


def timed(fn, r=None):
    fn()  # discarded
    t = []
    for _ in range(r or reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def once(fn):
    """(ms, result) of a single call: the host reference, whose first call is as good as its second."""
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def problem(n_vertices):
    mesh = blob_mesh(n_vertices, seed=0)
    pts, faces = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.faces)
    e1, e2 = pts[faces[:, 1]] - pts[faces[:, 0]], pts[faces[:, 2]] - pts[faces[:, 0]]
    mass = np.bincount(faces.ravel(), np.repeat(0.5 * np.linalg.norm(np.cross(e1, e2), axis=1) / 3.0, 3), n_vertices)
    rng = np.random.default_rng(5)
    w = rng.normal(size=(3, K))
    w *= (0.02 + 0.3 * np.sqrt(np.arange(K) / K)) / np.linalg.norm(w, axis=0)
    raw = np.cos(pts @ w + rng.uniform(0, 2 * np.pi, K))
    raw[:, 0] = 1.0
    q, _ = np.linalg.qr(raw * np.sqrt(mass)[:, None])
    phi_t = np.ascontiguousarray(q / np.sqrt(mass)[:, None])
    perm = rng.permutation(n_vertices)
    T_true = np.empty(n_vertices, dtype=np.int64)
    T_true[perm] = np.arange(n_vertices)
    return phi_t, np.ascontiguousarray(phi_t[T_true]), mass[T_true], T_true


phi_t, phi_s, mass_s, T_true = problem(n)
T0 = fr.corrupt(T_true, 0.3)
lines = ["# Functional maps and ZoomOut (`pf_fmap.hip`)", "",
         "`python tools/bench_fmap.py %d --reps %d --host %d` on one MI355X.  %d vertices on either side, a stand-in basis of "
         "%d smooth M-orthonormal functions (see the tool's header: not the eigensolver's), the source a renumbered copy.  "
         "Host clocks around synchronising calls (uploads and downloads included), first call discarded, median of %d."
         % (n, reps, n_host, n, K, reps), "",
         "## `pf_knn1_wide`, %d queries against %d references" % (n, n), "",
         "| data | d | ms | map found | coordinate pairs evaluated | share of n^2 d_pad | TFLOP/s (3 per pair) | share of the FP64 vector peak |",
         "|---|---|---|---|---|---|---|---|"]


def wide_row(label, ref, qry, truth, r=None):
    d = ref.shape[1]
    ms = timed(lambda: ctx.knn1_wide(ref, qry), r)
    ctx.knn1_wide_count(True)
    idx = ctx.knn1_wide(ref, qry)
    pairs = ctx.knn1_wide_count(False)
    d_pad = (d + 7) // 8 * 8
    tflops = 3.0 * pairs / (ms * 1e-3) / 1e12
    found = "" if truth is None else "%.2f %%" % (100.0 * np.mean(idx == truth))
    lines.append("| %s | %d | %.1f | %s | %.3g | %.1f %% | %.2f | %.1f %% |"
                 % (label, d, ms, found, pairs, 100.0 * pairs / (float(len(ref)) * len(qry) * d_pad), tflops,
                    100.0 * tflops / FP64_VALU_PEAK_TFLOPS))
    print(lines[-1], flush=True)


for d in (20, 32, 64, 128):
    wide_row("basis rows", np.ascontiguousarray(phi_t[:, :d]), np.ascontiguousarray(phi_s[:, :d]), T_true)
rng = np.random.default_rng(6)
n_rand = min(n, 65536)
wide_row("normal clouds, %d x %d" % (n_rand, n_rand), rng.standard_normal((n_rand, K)), rng.standard_normal((n_rand, K)), None, r=1)
lines += ["", "The time includes the upload of both sets and the transposition of the queries; the rate is over that whole call, so "
          "the kernel's own rate is higher.  `share of n^2 d_pad`: what the early exit left of the exhaustive work.", ""]

with _hip.DeviceFunctionalMap(phi_t[:, :32], phi_s[:, :32], mass_s, ctx=ctx) as h:
    h.set_p2p(T0)
    t_proj = timed(lambda: h.project(32, 32))
    C_dev = h.project(32, 32)
t_proj_host, C_host = once(lambda: fr.project(phi_t, phi_s, mass_s, T0, 32, 32))
t_zo = timed(lambda: zoomout_refine(phi_t[:, :32], phi_s[:, :32], mass_s, T0, 4, 32, ctx=ctx))
T, C = zoomout_refine(phi_t[:, :32], phi_s[:, :32], mass_s, T0, 4, 32, ctx=ctx)
lines += ["## Projection and ZoomOut, %d vertices, 30 %% of the initial map random" % n, "",
          "| call | device ms | numpy ms | result |", "|---|---|---|---|",
          "| one projection, k = 32 (map resident) | %.2f | %.1f | max difference to numpy %.2g |"
          % (t_proj, t_proj_host, np.max(np.abs(C_dev - C_host))),
          "| `zoomout_refine` 4 -> 32, step 1 (29 rounds, uploads and downloads included) | %.1f | | %.2f %% of the vertices at "
          "their true match, max \\|\\|C\\| - I\\| = %.2g |" % (t_zo, 100.0 * np.mean(T == T_true), np.max(np.abs(np.abs(C) - np.eye(32)))), ""]
print("\n".join(lines[-4:]), flush=True)

# ---- the same calls on the host, at a size it can finish
hp_t, hp_s, hm, hT = problem(n_host)
hT0 = fr.corrupt(hT, 0.3)
lines += ["## Host reference (`tests/_fmap_ref.py`, numpy) at %d vertices, the device beside it" % n_host, "",
          "| call | numpy ms | device ms | ratio |", "|---|---|---|---|"]
for d in (32, 128):
    a, b = np.ascontiguousarray(hp_t[:, :d]), np.ascontiguousarray(hp_s[:, :d])
    th, td = once(lambda: fr.brute_force_nn(a, b))[0], timed(lambda: ctx.knn1_wide(a, b))
    lines.append("| 1-NN, d = %d | %.0f | %.2f | %.0fx |" % (d, th, td, th / td))
th, (hT_ref, _) = once(lambda: fr.zoomout(hp_t, hp_s, hm, hT0, 4, 32))
td = timed(lambda: zoomout_refine(hp_t[:, :32], hp_s[:, :32], hm, hT0, 4, 32, ctx=ctx))
same = np.array_equal(hT_ref, zoomout_refine(hp_t[:, :32], hp_s[:, :32], hm, hT0, 4, 32, ctx=ctx)[0])
lines.append("| ZoomOut 4 -> 32 | %.0f | %.1f | %.0fx (same final map: %s) |" % (th, td, th / td, "yes" if same else "NO"))
text = "\n".join(lines) + "\n"
with open(out_path, "w") as fh:
    fh.write(text)
print(text)
