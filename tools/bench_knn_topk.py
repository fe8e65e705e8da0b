#!/usr/bin/env python3
"""The k-nearest-neighbour search (`pf_knn_topk`), timed:
python tools/bench_knn_topk.py [n_points] [--wide N] [--reps R] [--commit HASH] [--out FILE]

References: the points of blob_mesh(n, seed=0); queries: those of blob_mesh(n, seed=1) - two different surfaces of the
same size, so the clouds overlap without being registered.  Depth 3 is the points themselves; deeper coordinates append
smooth functions of the position, cos(w_c . x + b_c) with |w_c| growing with c (a stand-in for a spectral embedding: a
2-manifold in d dimensions; the same functions for both clouds).  Timed, n = 250000 by default:
  * `knn_topk` at d = 3, 5, 10 with k = 4, 8, 16, 64 (the box hierarchy);
  * `knn_topk` at d = 30 with k = 8 on --wide (default 20000) points a side (the exhaustive scan);
  * for comparison only, the existing `knn` (k <= 4, d <= 4: the grid search) at d = 3, k = 4 on the same input.
Per row: the whole call on the host's clock (upload, hierarchy, search, download; ends in a device synchronise) and the
device time between the upload and the download as `pf_timing_get` reports it (knn_ms).  The first call is discarded, then
the median of R.  Writes the markdown record (default profiles/knn_topk.md)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyfocusr_amd import _hip  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

args = sys.argv[1:]
opts = {"--wide": "20000", "--reps": "3", "--commit": "unknown", "--out": os.path.join(REPO, "profiles", "knn_topk.md")}
for flag in list(opts):
    if flag in args:
        j = args.index(flag)
        opts[flag] = args[j + 1]
        del args[j:j + 2]
n = int(args[0]) if args else 250000
n_wide, reps = int(opts["--wide"]), int(opts["--reps"])
ctx = _hip.default_context()


def embed(points, d):
    """(n, d): the points, then d - 3 smooth functions of them."""
    rng = np.random.default_rng(5)
    w = rng.normal(size=(3, max(d - 3, 1)))
    w *= (1.0 + 3.0 * np.sqrt(np.arange(w.shape[1]) / w.shape[1])) / np.linalg.norm(w, axis=0)
    extra = np.cos(points @ w + rng.uniform(0, 2 * np.pi, w.shape[1]))
    return np.ascontiguousarray(np.concatenate([points, extra], axis=1)[:, :d])


def timed(fn):
    """(median host ms, median device ms) of `reps` calls after one that is discarded."""
    fn()
    host, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        host.append(time.perf_counter() - t0)
        dev.append(ctx.timing()["knn_ms"])
    return 1e3 * float(np.median(host)), float(np.median(dev))


lines = ["# k nearest neighbours (`pf_knn_topk`, `pf_knn_tree.hip`)", "",
         "`python tools/bench_knn_topk.py %d --wide %d --reps %d` on one MI355X, commit %s: every figure below comes from that "
         "run.  References and queries: the points of two different blob meshes of the same size; coordinates beyond the "
         "third are smooth functions of the position (see the tool's header).  Whole call: host clock around the call, "
         "upload and download included; device: `pf_timing_get`'s knn_ms, from after the upload to before the download.  "
         "First call discarded, median of %d.  No time here is a pass criterion." % (n, n_wide, reps, opts["--commit"], reps),
         "", "| call | references x queries | d | k | whole call ms | device ms | path |", "|---|---|---|---|---|---|---|"]


def row(*cells):
    lines.append("| " + " | ".join(str(c) for c in cells) + " |")
    print(lines[-1], flush=True)


def clouds(n_points):
    a = np.asarray(blob_mesh(n_points, seed=0).points, dtype=np.float64)
    b = np.asarray(blob_mesh(n_points, seed=1).points, dtype=np.float64)
    return a, b


pa, pb = clouds(n)
print("%d x %d points ready" % (len(pa), len(pb)), flush=True)
for d in (3, 5, 10):
    ref, qry = embed(pa, d), embed(pb, d)
    for k in (4, 8, 16, 64):
        host, dev = timed(lambda: ctx.knn_topk(ref, qry, k))
        row("`knn_topk`", "%d x %d" % (len(ref), len(qry)), d, k, "%.2f" % host, "%.2f" % dev, "box hierarchy")
    if d == 3:
        host, dev = timed(lambda: ctx.knn(ref, qry, 4))
        row("`knn` (comparison)", "%d x %d" % (len(ref), len(qry)), 3, 4, "%.2f" % host, "%.2f" % dev, "grid, k <= 4")
        a, b = ctx.knn_topk(ref, qry, 4), ctx.knn(ref, qry, 4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
pa, pb = clouds(n_wide)
ref, qry = embed(pa, 30), embed(pb, 30)
host, dev = timed(lambda: ctx.knn_topk(ref, qry, 8))
row("`knn_topk`", "%d x %d" % (len(ref), len(qry)), 30, 8, "%.2f" % host, "%.2f" % dev, "exhaustive scan")
text = "\n".join(lines) + "\n"
with open(opts["--out"], "w") as fh:
    fh.write(text)
print(text)
