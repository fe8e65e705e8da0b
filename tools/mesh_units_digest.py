#!/usr/bin/env python3
"""Do two builds of the library give the mesh units' results to the bit?  (profiles/mesh_units_refactor.md)

    PYFOCUSR_HIP_LIB=/path/to/one/libpyfocusr_hip.so python tools/mesh_units_digest.py > a.txt
    PYFOCUSR_HIP_LIB=/path/to/other/libpyfocusr_hip.so python tools/mesh_units_digest.py > b.txt
    diff a.txt b.txt

On the test meshes of tests/test_curvature.py and tests/test_topology.py (blob700, messy700, cone, cylinder, cube,
zero_area) one line per output array, "<mesh> <call>.<array> <shape> <sha256 of its raw bytes>": every array of
`curvatures`, of `mesh_topology` with and without the outward rule, of `cluster_mesh` (fixed seeds, 5 iterations), and of
the signed structure - its counts, the vertex pseudonormals and the signed distances, faces and features of 200 fixed
queries.  Times (`device_ms`) are left out.  A tool, not a test: the bits of libm's functions may move with the
toolchain, so no digest is kept as a golden file."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

MESHES = ("blob700", "messy700", "cone", "cylinder", "cube", "zero_area")


def line(mesh, what, array):
    a = np.ascontiguousarray(array)
    print("%-10s %-32s %-12s %s" % (mesh, what, "x".join(str(s) for s in a.shape) or "scalar", hashlib.sha256(a.tobytes()).hexdigest()))


def lines(mesh, call, fn, keep=lambda out: out):
    """Every array of fn()'s dict but the time; a refusal of the library is a result like any other."""
    from pyfocusr_amd import _hip

    try:
        out = keep(fn())
    except _hip.PfError as e:
        print("%-10s %-32s refused: %s" % (mesh, call, e))
        return
    for key in sorted(out):
        if key != "device_ms":
            line(mesh, "%s.%s" % (call, key), out[key])


def main():
    import test_curvature
    from pyfocusr_amd import _hip

    print("library: %s" % _hip.LIB_PATH, file=sys.stderr)
    ctx = _hip.default_context()
    for name in MESHES:
        pts, faces = test_curvature._MESHES[name]()
        pts, faces = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32)
        n = len(pts)
        lines(name, "curvatures", lambda: ctx.curvatures(pts, faces))
        for outward in (True, False):
            # the report's last two entries count rounds, which depend on the timing of the hooks
            lines(name, "topology[outward=%d]" % outward, lambda: ctx.mesh_topology(n, faces, points=pts, outward=outward),
                  lambda out: dict(out, report=out["report"][:6]))
        rng = np.random.default_rng(5)
        seeds = np.sort(rng.choice(n, size=max(n // 20, 4), replace=False))
        mass = 0.5 + rng.random(n)
        lines(name, "cluster_mesh", lambda: ctx.cluster_mesh(pts, faces, mass, seeds=seeds, n_iter=5))
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        queries = lo - 0.25 * (hi - lo) + 1.5 * (hi - lo) * np.random.default_rng(6).random((200, 3))
        surface = _hip.DeviceSurface(pts, faces, ctx=ctx)
        try:
            line(name, "prepare_signed.counts", surface._prepare_signed())
            line(name, "prepare_signed.vertex_normals", surface.vertex_normals())
            sd, face, feature, ambiguous = surface.signed_distance(queries)
            line(name, "signed_distance.sd", sd)
            line(name, "signed_distance.face", face)
            line(name, "signed_distance.feature", feature)
            line(name, "signed_distance.n_ambiguous", np.int64(ambiguous))
        finally:
            surface.close()


if __name__ == "__main__":
    main()
