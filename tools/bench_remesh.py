"""Time and quality of uniform mesh resampling (profiles/remesh.md).

    python tools/bench_remesh.py --n 250000 --m 15000 1000 --n-iter 20 --repeats 3

One JSON line per target size for `blob_mesh(n)`: the whole call `resample_mesh(mesh, m)` (host clock: argument checks,
vertex areas, farthest-point seeds, `pf_mesh_cluster`, the projection onto the input surface), the seeding alone, the
library's own time of `pf_mesh_cluster` between upload and download (`device_ms`, HIP events: it contains the host's
reads of `changed`), and single steps through the same entry point from the converged state: one assignment (warm start:
the final labels), one update, and the dual as the difference of a call with and without faces.  Distances evaluated per
assignment come from the library's counter, next to the n x m of a brute force.  Quality: candidate and output faces,
mixed votes, `mesh_topology` of the result, two-sided Hausdorff and ASSD between input and output surface.  Then the
numpy reference of the tests (`tests/_remesh_ref.py::cluster`) at `--reference-n` -> `--reference-m` on the same host
beside the device at that size, and whether all outputs are equal."""
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


def _timed(fn, repeats):
    """(result of the last call, wall ms of every call but the first)"""
    out, times = None, []
    for it in range(1 + repeats):
        t0 = time.perf_counter()
        out = fn()
        if it:
            times.append(1e3 * (time.perf_counter() - t0))
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--m", type=int, nargs="*", default=[15000, 1000], help="target sizes; none: the reference part only")
    ap.add_argument("--n-iter", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reference-n", type=int, default=20000, help="0 skips the numpy reference")
    ap.add_argument("--reference-m", type=int, default=2000)
    ap.add_argument("--no-quality", action="store_true", help="skip the topology and the surface distances of the result")
    args = ap.parse_args()

    from pyfocusr_amd import _hip, farthest_point_sampling, mesh_topology, resample_mesh, surface_distance_metrics
    from pyfocusr_amd.meshgen import blob_mesh

    ctx = _hip.default_context()
    mesh = blob_mesh(args.n, seed=args.seed)
    P, F = mesh.points, mesh.faces
    mass = np.ascontiguousarray(ctx.curvatures(P, F)["area"])
    for m in args.m:
        sel, t_seed = _timed(lambda: farthest_point_sampling(P, m, ctx=ctx), args.repeats)
        (new, info), t_call = _timed(lambda: resample_mesh(mesh, m, n_iter=args.n_iter, return_info=True, ctx=ctx), args.repeats)
        rows = [ctx.cluster_mesh(P, F, mass, seeds=sel, n_iter=args.n_iter) for _ in range(1 + args.repeats)][1:]
        raw = rows[-1]
        passes = int(raw["report"][5])
        # single steps from the converged state
        step = {"assign": [], "update": [], "dual": []}
        for _ in range(1 + args.repeats):
            a = ctx.cluster_mesh(P, None, mass, centroids=raw["centroids"], labels=raw["labels"], n_iter=0)
            u = ctx.cluster_mesh(P, None, mass, centroids=raw["centroids"], labels=raw["labels"], n_iter=1, update_only=True)
            d = ctx.cluster_mesh(P, F, mass, centroids=raw["centroids"], labels=raw["labels"], n_iter=1, update_only=True)
            step["assign"].append(a["device_ms"])
            step["update"].append(u["device_ms"])
            step["dual"].append(d["device_ms"] - u["device_ms"])
        out = dict(n=args.n, n_faces=int(len(F)), m=m, n_iter=args.n_iter, repeats=args.repeats, call_ms=_stats(t_call),
                   seeding_ms=_stats(t_seed), cluster_device_ms=_stats([r["device_ms"] for r in rows]),
                   n_iter_run=raw["n_iter_run"], changed=raw["changed"].tolist(),
                   assign_step_device_ms=_stats(step["assign"][1:]), update_step_device_ms=_stats(step["update"][1:]),
                   dual_device_ms=_stats(step["dual"][1:]), assignments=passes, grid_cells=int(raw["report"][3]),
                   distances_per_assignment=float(raw["report"][4]) / passes, brute_force_distances=args.n * m,
                   distances_converged_assignment=int(a["report"][4]), n_candidate_faces=raw["n_candidate_faces"],
                   n_output_faces=int(len(raw["faces"])), n_mixed_votes=int(np.count_nonzero(raw["votes"][:, 1])),
                   n_output_vertices=int(len(new.points)), n_empty_clusters=int(np.count_nonzero(raw["count"] == 0)),
                   cluster_size=dict(min=int(raw["count"].min()), max=int(raw["count"].max())))
        if not args.no_quality:
            topo = mesh_topology(new, ctx=ctx)
            metrics = surface_distance_metrics(mesh, new, ctx=ctx)
            diagonal = float(np.linalg.norm(P.max(axis=0) - P.min(axis=0)))
            out.update(topology=dict(n_patches=topo.n_patches, n_boundary_edges=topo.n_boundary_edges,
                                     n_nonmanifold_edges=topo.n_nonmanifold_edges, n_inconsistent_edges=topo.n_inconsistent_edges),
                       diagonal=diagonal, hausdorff=float(metrics["hausdorff"]), assd=float(metrics["assd"]),
                       max_input_to_output=float(metrics["max_a_to_b"]), max_output_to_input=float(metrics["max_b_to_a"]))
        print(json.dumps(out), flush=True)

    if args.reference_n:
        import _fps_ref
        import _remesh_ref as ref

        small = blob_mesh(args.reference_n, seed=args.seed)
        a = ref.vertex_areas(small.points, small.faces)
        sel = _fps_ref.fps(small.points, args.reference_m)[0]
        t0 = time.perf_counter()
        r = ref.cluster(small.points, small.faces, a, sel, args.n_iter)
        t_ref = 1e3 * (time.perf_counter() - t0)
        rows = [ctx.cluster_mesh(small.points, small.faces, a, seeds=sel, n_iter=args.n_iter) for _ in range(1 + args.repeats)][1:]
        dev = rows[-1]
        equal = all(np.array_equal(dev[k], r[k]) for k in ("labels", "rep", "count", "changed", "faces", "face_src", "votes"))
        equal = equal and dev["centroids"].tobytes() == r["centroids"].tobytes()
        print(json.dumps(dict(reference_n=args.reference_n, reference_m=args.reference_m, n_iter_run=r["n_iter_run"],
                              numpy_reference_ms=t_ref, cluster_device_ms=_stats([x["device_ms"] for x in rows]),
                              outputs_equal=bool(equal))), flush=True)


if __name__ == "__main__":
    main()
