"""Time of the discrete curvatures of one blob mesh (profiles/curvature.md).

    python tools/bench_curvature.py --n 250000 --repeats 3

One JSON line: the whole call `discrete_curvatures(points, faces)` (host clock around a call that ends in a stream
synchronise: argument checks, upload, three kernels and two radix sorts, download of every field) and the library's own
device time between upload and download (`device_ms`, HIP events), first call discarded, median and spread of the
repeats; next to them the vectorised numpy reference of the tests (`tests/_curvature_ref.py::curvatures`) on the same
host, and the worst ratio per field between the two (the quantities the GPU tests bound)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)
sys.path.append(os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy reference and the comparison")
    args = ap.parse_args()

    from pyfocusr_amd import _hip, discrete_curvatures
    from pyfocusr_amd.meshgen import blob_mesh

    mesh = blob_mesh(args.n, seed=args.seed)
    pts, faces = mesh.points, mesh.faces
    ctx = _hip.default_context()
    rows, dev = [], None
    for it in range(1 + args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        dev = discrete_curvatures(pts, faces, ctx=ctx)
        t1 = time.perf_counter()
        if it > 0:
            rows.append((1e3 * (t1 - t0), dev["device_ms"]))
    a = np.array(rows)
    out = dict(n=args.n, n_faces=int(len(faces)), repeats=args.repeats,
               call_ms=dict(median=float(np.median(a[:, 0])), min=float(a[:, 0].min()), max=float(a[:, 0].max())),
               device_ms=dict(median=float(np.median(a[:, 1])), min=float(a[:, 1].min()), max=float(a[:, 1].max())),
               topology=[int(v) for v in dev["topology"]])
    if not args.no_reference:
        import _curvature_ref as ref

        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            r = ref.curvatures(pts, faces)
            times.append(1e3 * (time.perf_counter() - t0))
        out.update(numpy_ms=dict(median=float(np.median(times)), min=float(min(times)), max=float(max(times))),
                   topology_equal=bool(np.array_equal(dev["topology"], r["topology"])), worst_ratio=ref.ratios(dev, r))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
