"""Time of the map distortion and coverage metrics of one blob pair under a nearest-vertex map (profiles/map_quality.md).

    python tools/bench_map_quality.py --n 250000 --repeats 5

One JSON line: the whole call `map_distortion(source, target_points, vertex_map=...)` without the flip test (host clock
around a call that ends in a stream synchronise: argument checks, upload, seven kernels and two radix sorts, download of
every field) and the library's own device time between upload and download (`device_ms`, HIP events), first call
discarded, median and spread of the repeats; the same call with the flip test (the target's vertex normals are built on
the device first); next to them what a numpy user would write for the same quantities
(`tests/_map_quality_ref.py::vectorised`) on the same host, and whether every output has the bits of the ordered numpy
reference (`distortion`).  The map itself (the nearest target vertex of every source vertex, `Context.knn1`) is computed
before the clock starts."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)
sys.path.append(os.path.join(REPO, "tests"))


def _stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy timings and the comparison")
    args = ap.parse_args()

    from pyfocusr_amd import _hip, map_distortion
    from pyfocusr_amd.meshgen import blob_mesh

    source, target = blob_mesh(args.n, seed=args.seed), blob_mesh(args.n, seed=args.seed + 1)
    ps, fs, pt, ft = source.points, source.faces, target.points, target.faces
    ctx = _hip.default_context()
    vmap = np.ascontiguousarray(ctx.knn1(pt, ps), dtype=np.int32)
    rows, flip_rows, dev = [], [], None
    for it in range(1 + args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        dev = map_distortion((ps, fs), pt, vertex_map=vmap, ctx=ctx)
        t1 = time.perf_counter()
        with_flips = map_distortion((ps, fs), (pt, ft), vertex_map=vmap, ctx=ctx)
        t2 = time.perf_counter()
        if it > 0:
            rows.append((1e3 * (t1 - t0), dev["device_ms"]))
            flip_rows.append(1e3 * (t2 - t1))
    a = np.array(rows)
    out = dict(n=args.n, n_faces=int(len(fs)), n_target=int(len(pt)), repeats=args.repeats, call_ms=_stats(a[:, 0]),
               device_ms=_stats(a[:, 1]), call_with_flip_test_ms=_stats(flip_rows), report=[int(v) for v in dev["report"]],
               report_with_flip_test=[int(v) for v in with_flips["report"]], dirichlet_energy=dev["dirichlet_energy"],
               area_distortion=dev["area_distortion"], collapsed_area_fraction=dev["collapsed_area_fraction"],
               target_vertices_hit_fraction=dev["target_vertices_hit_fraction"])
    if not args.no_reference:
        import _map_quality_ref as ref

        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ref.vectorised(ps, fs, pt, vmap)
            times.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        r = ref.distortion(ps, fs, pt, vmap)
        ordered_ms = 1e3 * (time.perf_counter() - t0)
        raw = ctx.map_distortion(ps, fs, pt, vmap)
        out.update(numpy_ms=_stats(times), ordered_reference_ms=ordered_ms,
                   same_bits={k: bool(np.array_equal(raw[k], r[k])) for k in ref.FLOAT_FIELDS + ref.INT_FIELDS})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
