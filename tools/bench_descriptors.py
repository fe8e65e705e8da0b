#!/usr/bin/env python3
"""Spectral descriptors, timed: python tools/bench_descriptors.py [n_vertices] [--reps R] [--out FILE]

`pf_spectral_descriptors` and `pf_descriptor_coefficients` at n x 128 x 200 (default n = 250000; k_out = 20 and 128 for
the coefficients).  A Laplace-Beltrami basis of 128 functions of a 250k mesh is beyond what the eigensolver has been
verified for, and the kernels' time does not depend on the values: phi is a normal random block scaled like an
M-orthonormal basis, the eigenvalues grow linearly (Weyl), G is the library's own HKS table beside its WKS table, 100
samples each.  Host clocks around the calls, which end in a device synchronise and INCLUDE the upload of phi (n x 128
doubles) and, for the descriptors, the download of F (n x 200 doubles); the first call is discarded, then the median of
R.  The kernels' own times come from a kernel trace of this tool (`rocprofv3 --kernel-trace --stats -- python
tools/bench_descriptors.py --reps 1`), not from here.  Operation counts: 1 + 2 T per (row, basis function) for F, 2 more
per (row, output basis function, sample) plus one per (row, sample) for the coefficients; rates against the 78.6 TFLOP/s
FP64 vector peak, which counts a fused multiply-add as two: separate multiplies and adds can reach half of it.
The first rows of F are compared with the numpy loop bit for bit, the coefficients with numpy's matrix product.
Writes the markdown record (default profiles/spectral_descriptors.md)."""
import importlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _descriptor_ref as dr  # noqa: E402
from pyfocusr_amd import _hip  # noqa: E402

sd = importlib.import_module("pyfocusr_amd.spectral_descriptors")

FP64_VALU_PEAK_TFLOPS = 78.6
args = sys.argv[1:]
reps, out_path = 3, os.path.join(REPO, "profiles", "spectral_descriptors.md")
for flag in ("--reps", "--out"):
    if flag in args:
        k = args.index(flag)
        if flag == "--reps":
            reps = int(args[k + 1])
        else:
            out_path = args[k + 1]
        del args[k:k + 2]
n = int(args[0]) if args else 250000
K, T_HALF, CHECK_ROWS = 128, 100, 2048
ctx = _hip.default_context()


def timed(fn):
    fn()  # discarded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


rng = np.random.default_rng(11)
mass = rng.uniform(0.5, 1.5, n) / n
phi = rng.standard_normal((n, K)) / np.sqrt(mass.sum())
vals = 10.0 * np.arange(1, K + 1)
G = np.concatenate([sd.hks_table(vals, n_times=T_HALF)[0], sd.wks_table(vals, n_energies=T_HALF)[0]], axis=1)
T = G.shape[1]

lines = ["# Spectral descriptors (`pf_descriptors.hip`)", "",
         "`python tools/bench_descriptors.py %d --reps %d` on one MI355X.  phi %d x %d (a random stand-in: see the tool's header), "
         "G %d x %d (HKS beside WKS).  Host clocks around whole calls - the upload of phi (%.0f MB) and, for the descriptors, the "
         "download of F (%.0f MB) included - first call discarded, median of %d." % (n, reps, n, K, K, T, 8e-6 * n * K, 8e-6 * n * T, reps),
         "", "| call | ms (whole call) | GFLOP | TFLOP/s over the whole call | share of the FP64 vector peak | check |", "|---|---|---|---|---|---|"]


def row(label, ms, flop, check):
    tflops = flop / (ms * 1e-3) / 1e12
    lines.append("| %s | %.1f | %.1f | %.2f | %.1f %% | %s |" % (label, ms, 1e-9 * flop, tflops, 100.0 * tflops / FP64_VALU_PEAK_TFLOPS, check))
    print(lines[-1], flush=True)


ms = timed(lambda: ctx.spectral_descriptors(phi, G))
F = ctx.spectral_descriptors(phi, G)
same = F[:CHECK_ROWS].tobytes() == dr.descriptors(phi[:CHECK_ROWS], G).tobytes()
row("`pf_spectral_descriptors`", ms, float(n) * K * (1 + 2 * T), "first %d rows equal the numpy loop's bits: %s" % (CHECK_ROWS, "yes" if same else "NO"))
A_host = None
for k_out in (20, 128):
    ms = timed(lambda: ctx.descriptor_coefficients(phi, mass, G, k_out))
    A = ctx.descriptor_coefficients(phi, mass, G, k_out)
    if A_host is None:
        A_host = (phi * mass[:, None]).T @ F
    scale = np.abs(phi * mass[:, None]).T @ np.abs(F)
    row("`pf_descriptor_coefficients`, k_out = %d" % k_out, ms, float(n) * (K * (1 + 2 * T) + T + 2.0 * k_out * T),
        "max |A - numpy| / sum |terms| = %.2g" % np.max(np.abs(A - A_host[:k_out]) / scale[:k_out]))
text = "\n".join(lines) + "\n"
with open(out_path, "w") as fh:
    fh.write(text)
print(text)
