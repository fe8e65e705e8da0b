"""Assembly and eigensolve time of one blob mesh for either Laplacian (profiles/cotangent.md).

    python tools/bench_cotangent.py --n 250000 --k 5 --laplacian cotangent --repeats 7 --warmup 2

One JSON line: per repeat, the wall time of the device assembly (host clock around a call that ends in a stream
synchronise; the mesh is resident in HBM before the clock starts), the assembler's own device time (`pf_timing.build_ms`,
HIP events), and the wall time of `Graph.get_graph_spectrum()` up to the eigenvectors' arrival on the host; medians and
the spread.  `--laplacian inverse_length` uses only what the package offered before the cotangent option existed, so the
same script times an older checkout (put that checkout first on PYTHONPATH)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (behind PYTHONPATH: an older checkout wins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--laplacian", default="inverse_length", choices=["inverse_length", "cotangent"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from pyfocusr_amd import Graph, _hip
    from pyfocusr_amd.meshgen import blob_mesh

    mesh = blob_mesh(args.n, seed=args.seed)
    ctx = _hip.default_context()
    resident = _hip.DeviceMesh(mesh.points, mesh.faces, ctx=ctx)
    mesh._pf_device_mesh = resident
    kw = {} if args.laplacian == "inverse_length" else {"laplacian": "cotangent"}
    rows = []
    vals = stats = None
    for it in range(args.warmup + args.repeats):
        g = Graph(mesh, n_spectral_features=args.k, n_rand_samples=10, ctx=ctx, verbose=False, **kw)
        ctx.sync()
        t0 = time.perf_counter()
        dev = g.device
        ctx.sync()
        t1 = time.perf_counter()
        build_ms = ctx.timing()["build_ms"]
        t2 = time.perf_counter()
        g.get_graph_spectrum()
        _ = g.eig_vecs  # (collects the download)
        ctx.sync()
        t3 = time.perf_counter()
        vals, stats = np.array(g.eig_vals), g.eigs_stats
        if it >= args.warmup:
            rows.append((1e3 * (t1 - t0), float(build_ms), 1e3 * (t3 - t2)))
        dev.close()
    a = np.array(rows)
    med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
    out = dict(n=args.n, k=args.k, laplacian=args.laplacian, repeats=args.repeats, warmup=args.warmup,
               assembly_wall_ms=dict(median=med[0], min=lo[0], max=hi[0]),
               assembly_device_ms=dict(median=med[1], min=lo[1], max=hi[1]),
               eigensolve_wall_ms=dict(median=med[2], min=lo[2], max=hi[2]),
               eig_vals=[float(v) for v in vals], n_columns=int(len(vals)),
               matvecs=int(getattr(stats, "matvecs", -1)), degree=int(getattr(stats, "degree", -1)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
