"""Time of the mesh topology of two blob meshes (profiles/topology.md).

    python tools/bench_topology.py --n 250000 --repeats 3

One JSON line per mesh - `blob_mesh(n)` with 1 % of its faces reversed, and `messy_blob_mesh(n)`: the whole call
`mesh_topology(mesh)` (host clock: argument checks, the library's index check, upload, the kernels, sorts and labelling
rounds, download, the per-patch table in numpy), the library's own time between upload and download (`device_ms`, HIP
events: it contains the host's reads of the labelling flag), the labelling rounds, first call discarded, median and
spread of the repeats; next to them the numpy / scipy reference of the tests (`tests/_topology_ref.py::topology`) on the
same host, and whether every integer output equals it."""
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
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy / scipy reference and the comparison")
    args = ap.parse_args()

    from pyfocusr_amd import _hip, mesh_topology
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    clean = blob_mesh(args.n, seed=args.seed)
    faces = clean.faces.copy()
    which = np.random.default_rng(args.seed).choice(len(faces), size=len(faces) // 100, replace=False)
    faces[which] = faces[which][:, [0, 2, 1]]
    messy = messy_blob_mesh(args.n, seed=args.seed)
    ctx = _hip.default_context()
    for name, pts, f in (("blob_1pct_reversed", clean.points, faces), ("messy_blob", messy.points, messy.faces)):
        rows, dev = [], None
        for it in range(1 + args.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            dev = mesh_topology((pts, f), ctx=ctx)
            t1 = time.perf_counter()
            if it > 0:
                rows.append((1e3 * (t1 - t0), dev["device_ms"]))
        a = np.array(rows)
        out = dict(mesh=name, n=args.n, n_faces=int(len(f)), repeats=args.repeats,
                   call_ms=dict(median=float(np.median(a[:, 0])), min=float(a[:, 0].min()), max=float(a[:, 0].max())),
                   device_ms=dict(median=float(np.median(a[:, 1])), min=float(a[:, 1].min()), max=float(a[:, 1].max())),
                   rounds=dev["rounds"], loop_rounds=dev["loop_rounds"], n_patches=dev["n_patches"],
                   n_boundary_loops=dev["n_boundary_loops"], n_flipped=int(dev["flip"].sum()),
                   edges=[dev["n_edges"], dev["n_boundary_edges"], dev["n_nonmanifold_edges"], dev["n_inconsistent_edges"]])
        if name == "blob_1pct_reversed":
            out["flip_is_the_reversed_set"] = bool(np.array_equal(np.flatnonzero(dev["flip"]), np.sort(which)))
        if not args.no_reference:
            import _topology_ref as ref

            times = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                r = ref.topology(len(pts), f, pts)
                times.append(1e3 * (time.perf_counter() - t0))
            equal = all(np.array_equal(dev[k], r[k]) for k in ("face_neighbours", "patch", "flip", "boundary_loop"))
            equal = equal and all(np.array_equal(dev["patches"][k], r["patches"][k]) for k in r["patches"] if k != "signed_volume")
            equal = equal and all(dev[k] == r[k] for k in ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_inconsistent_edges",
                                                           "n_patches", "n_boundary_loops"))
            with np.errstate(invalid="ignore", divide="ignore"):
                vol = np.abs(dev["patches"]["signed_volume"] - r["patches"]["signed_volume"]) / r["volume_terms"]
            out.update(reference_ms=dict(median=float(np.median(times)), min=float(min(times)), max=float(max(times))),
                       integers_equal=bool(equal), worst_volume_ratio=float(np.nanmax(np.r_[0.0, vol])))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
