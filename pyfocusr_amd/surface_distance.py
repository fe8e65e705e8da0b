"""Exact surface distances between meshes: per-point distances, ASSD, RMS, Hausdorff and its 95th percentile.

The reference sketches a registration check (`pyfocusr/test.py`, `get_all_pairwise_surface_errors`) around a
`get_surface_distance_metrics` it never defines.  Here the distance of every vertex of one mesh to the surface of the
other is the exact minimum over all triangles (polygons fan-triangulated), computed on the MI355X by
`pf_surface_distance` (`_hip.DeviceSurface.distance`): the same arithmetic and tie rule as the ICP search, so the
squared distances equal a brute-force scan bit for bit.  The summary of the downloaded distances is host work
(`summarize_distances`, which needs no device).

Signed distances (`pf_surface_signed_distance`, `_hip.DeviceSurface.signed_distance`) add the side: the sign of
(p - c) . n with n the angle-weighted pseudonormal of the face, edge or vertex the closest point c lies on.  On a
closed, consistently oriented mesh with outward faces, inside is negative (as in VTK's vtkImplicitPolyDataDistance);
the magnitude is the unsigned distance bit for bit.

Generalized winding numbers (`pf_surface_winding`, `_hip.DeviceSurface.winding_number`): w = the signed solid angles
of all triangles seen from the point, over 4 pi.  1 inside and 0 outside a closed outward-oriented mesh, smooth across
holes, no normals or manifoldness needed: `winding_numbers`, `points_inside`, and the signs of `sign="winding"` for
meshes that are open or non-manifold, where the pseudonormal sign flips near every boundary loop.
"""
import contextlib

import numpy as np

from . import _hip
from . import vtk_functions
from ._meshargs import checked_mesh


def _query_array(points):
    return _hip._queries(points, "query points")


def point_to_surface_distances(points, mesh, ctx=None):
    """(d (n,) f64, face (n,) i32): the distance of every point to the surface of `mesh` and the face that attains it
    (lowest face index on exact ties).  A point with a non-finite coordinate gives NaN and -1.  `mesh` may also be a
    `_hip.DeviceSurface` built earlier, which is then reused and left open."""
    q = _query_array(points)
    if hasattr(mesh, "distance"):  # a DeviceSurface
        d2, face, _ = mesh.distance(q)
        return np.sqrt(d2), face
    pts, faces = checked_mesh(mesh)
    with _hip.DeviceSurface(pts, faces, ctx=ctx) as surface:
        d2, face, _ = surface.distance(q)
    return np.sqrt(d2), face


def _direction(d, tag):
    d = np.asarray(d, dtype=np.float64).ravel()
    fin = np.isfinite(d)
    n = int(fin.sum())
    out = {"n_" + tag: n, "n_nan_" + tag: int(d.size - n)}
    if n == 0:
        out.update({"mean_" + tag: np.nan, "rms_" + tag: np.nan, "max_" + tag: np.nan, "max_%s_vertex" % tag: -1,
                    "p95_" + tag: np.nan, "_sum": 0.0})
        return out
    df = d[fin]
    s = float(np.sum(df))
    v = int(np.argmax(np.where(fin, d, -np.inf)))  # lowest index on ties
    out.update({"mean_" + tag: s / n, "rms_" + tag: float(np.sqrt(np.sum(df * df) / n)), "max_" + tag: float(d[v]),
                "max_%s_vertex" % tag: v, "p95_" + tag: float(np.percentile(df, 95)), "_sum": s})
    return out


def summarize_distances(d_a_to_b, d_b_to_a=None):
    """Metrics of per-point distances (pure numpy, no device).  Non-finite distances are counted (`n_nan_*`) and left
    out.  Per direction `t` (`a_to_b`, and `b_to_a` if given): `n_t`, `n_nan_t`, `mean_t`, `rms_t`, `max_t`,
    `max_t_vertex` (the point attaining it, lowest index on ties), `p95_t`.  With both directions also `assd`
    (mean over the points of both meshes), `hausdorff` (max of both maxima) and `hausdorff_95` (max of both 95th
    percentiles)."""
    ab = _direction(d_a_to_b, "a_to_b")
    s_ab = ab.pop("_sum")
    if d_b_to_a is None:
        return ab
    ba = _direction(d_b_to_a, "b_to_a")
    s_ba = ba.pop("_sum")
    out = dict(ab, **ba)
    n = ab["n_a_to_b"] + ba["n_b_to_a"]
    out["assd"] = (s_ab + s_ba) / n if n else np.nan
    out["hausdorff"] = float(np.nanmax([ab["max_a_to_b"], ba["max_b_to_a"]])) if n else np.nan
    out["hausdorff_95"] = float(np.nanmax([ab["p95_a_to_b"], ba["p95_b_to_a"]])) if n else np.nan
    return out


_SIGNS = ("pseudonormal", "winding")


def _check_sign(sign):
    if sign not in _SIGNS:
        raise ValueError("sign must be one of %r, not %r" % (_SIGNS, sign))


def winding_numbers(points, mesh, ctx=None, beta=0.0):
    """w (n,) f64: the generalized winding number of `mesh` at every point: the signed solid angles of all triangles
    (polygons fan-triangulated) seen from the point, over 4 pi.  1 inside and 0 outside a closed mesh with outward faces
    (reversed faces subtract), in between near holes; NaN for a point with a non-finite coordinate.  `beta <= 0`
    evaluates every triangle exactly; `beta > 1` replaces clusters of triangles at least `beta` cluster radii away by
    their dipole (`_hip.DeviceSurface.winding_number` also returns the bound on what that changes).  `mesh` may also be
    a `_hip.DeviceSurface` built earlier, which is then reused and left open."""
    q = _query_array(points)
    beta = float(beta)
    if 0.0 < beta <= 1.0 or beta != beta or beta == np.inf:
        raise ValueError("beta must be <= 0 (exact) or a finite value > 1, not %r" % beta)
    if hasattr(mesh, "winding_number"):  # a DeviceSurface
        return mesh.winding_number(q, beta=beta)[0]
    pts, faces = checked_mesh(mesh)
    with _hip.DeviceSurface(pts, faces, ctx=ctx) as surface:
        return surface.winding_number(q, beta=beta)[0]


def points_inside(points, mesh, ctx=None, threshold=0.5):
    """bool (n,): `winding_numbers(points, mesh) > threshold`; False for a point with a non-finite coordinate.  On an
    open mesh w falls off smoothly across a hole, and 0.5 is the level that closes it the way the surface continues."""
    w = winding_numbers(points, mesh, ctx=ctx)
    with np.errstate(invalid="ignore"):
        return w > threshold


def _signed_on_surface(surface, q, sign):
    """(sd, face) of the queries against an open DeviceSurface."""
    if sign == "pseudonormal":
        sd, face, _, _ = surface.signed_distance(q)
        return sd, face
    d2, face, _ = surface.distance(q)
    w, _ = surface.winding_number(q)
    d = np.sqrt(d2)
    with np.errstate(invalid="ignore"):
        sd = np.where((w > 0.5) & (d > 0.0), -d, d)  # +0.0 at distance 0; NaN stays NaN
    return sd, face


def signed_point_to_surface_distances(points, mesh, ctx=None, check_orientation=True, sign="pseudonormal"):
    """(sd (n,) f64, face (n,) i32): the signed distance of every point to the surface of `mesh` (negative on the side
    opposite to the face normals: inside an outward-oriented closed mesh) and the face that attains it.  |sd| and face
    equal `point_to_surface_distances` bit for bit; NaN and -1 for a point with a non-finite coordinate.  `mesh` may
    also be a `_hip.DeviceSurface`, reused and left open.

    `sign="pseudonormal"`: the side of the angle-weighted pseudonormal at the closest point.  With `check_orientation`
    a mesh whose triangles disagree on their orientation (inconsistent edges) or that has edges in three or more
    triangles raises ValueError: the sign means nothing there (`topology.orient_faces` reverses the faces that
    disagree).  Open boundaries are allowed (the sign then follows the face normals nearby, and flips near every
    boundary loop).

    `sign="winding"`: negative where the generalized winding number (`winding_numbers`, exact mode) exceeds 0.5,
    positive otherwise, +0.0 at distance 0.  Meant for open and non-manifold meshes; with `check_orientation` only
    inconsistent edges raise (a reversed face subtracts its solid angle instead of adding it)."""
    q = _query_array(points)
    _check_sign(sign)
    own = contextlib.nullcontext()
    if hasattr(mesh, "signed_distance"):  # a DeviceSurface
        surface = mesh
    else:
        pts, faces = checked_mesh(mesh)
        surface = own = _hip.DeviceSurface(pts, faces, ctx=ctx)
    with own:
        if check_orientation:
            t = surface.topology()
            if sign == "winding":
                if t["n_inconsistent_edges"]:
                    raise ValueError("winding-number signs need consistently oriented faces: %d inconsistent edges "
                                     "(check_orientation=False to compute them anyway)" % t["n_inconsistent_edges"])
            elif t["n_inconsistent_edges"] or t["n_nonmanifold_edges"]:
                raise ValueError("signed distances need a consistently oriented manifold surface: %d inconsistent and %d "
                                 "non-manifold edges (check_orientation=False to compute them anyway)"
                                 % (t["n_inconsistent_edges"], t["n_nonmanifold_edges"]))
        sd, face = _signed_on_surface(surface, q, sign)
    return sd, face


def summarize_signed_distances(sd):
    """Summary of signed distances (pure numpy, no device): `n` (finite values), `n_nan` (the others, left out),
    `mean_signed` (the bias), `std_signed`, `min_signed` / `min_signed_vertex` (deepest inside), `max_signed` /
    `max_signed_vertex` (farthest outside; lowest index on ties), `n_inside` (sd < 0), `n_outside` (sd > 0), `n_on`
    (sd == 0)."""
    sd = np.asarray(sd, dtype=np.float64).ravel()
    fin = np.isfinite(sd)
    n = int(fin.sum())
    out = {"n": n, "n_nan": int(sd.size - n)}
    if n == 0:
        out.update({"mean_signed": np.nan, "std_signed": np.nan, "min_signed": np.nan, "min_signed_vertex": -1,
                    "max_signed": np.nan, "max_signed_vertex": -1, "n_inside": 0, "n_outside": 0, "n_on": 0})
        return out
    f = sd[fin]
    lo = int(np.argmin(np.where(fin, sd, np.inf)))  # first index on ties
    hi = int(np.argmax(np.where(fin, sd, -np.inf)))
    out.update({"mean_signed": float(np.mean(f)), "std_signed": float(np.std(f)), "min_signed": float(sd[lo]),
                "min_signed_vertex": lo, "max_signed": float(sd[hi]), "max_signed_vertex": hi,
                "n_inside": int(np.sum(f < 0)), "n_outside": int(np.sum(f > 0)), "n_on": int(np.sum(f == 0))})
    return out


def signed_distances_on_mesh(mesh, other, name="signed_distance", ctx=None, sign="pseudonormal"):
    """Signed distances of `mesh`'s vertices to the surface of `other` (`signed_point_to_surface_distances`, orientation
    checked, `sign` as there), stored on `mesh` as the point-data array `name` (`set_mesh_scalars`; written by
    `write_vtk_mesh` with 17 digits, so they read back exactly).  Returns the distances."""
    pts, _ = checked_mesh(mesh)
    _check_sign(sign)
    sd, _ = signed_point_to_surface_distances(pts, other, ctx=ctx, sign=sign)
    vtk_functions.set_mesh_scalars(mesh, sd, name=name)
    return sd


def surface_distance_metrics(mesh_a, mesh_b, symmetric=True, ctx=None, surface_a=None, surface_b=None, signed=False,
                             sign="pseudonormal"):
    """Distances from the vertices of `mesh_a` to the surface of `mesh_b` (and, if `symmetric`, from `mesh_b`'s
    vertices to `mesh_a`'s surface), summarised by `summarize_distances`: `mean_a_to_b`, `rms_a_to_b`, `max_a_to_b`,
    `max_a_to_b_vertex`, `p95_a_to_b`, the same for `b_to_a`, `assd`, `hausdorff`, `hausdorff_95`.

    Meshes: `PolyMesh`, vtkPolyData or `(points, faces)`; quads and larger polygons are fan-triangulated.
    `surface_a` / `surface_b`: `_hip.DeviceSurface` objects already built from the same meshes, reused and left open
    (many pairs over one set of meshes build each surface once).

    `signed=True` adds `summarize_signed_distances` of each direction, its keys suffixed `_a_to_b` / `_b_to_a`
    (`mean_signed_a_to_b` is the bias of `mesh_a` against `mesh_b`'s surface; negative = inside it).  Orientation is
    not checked here; `topology()` of a surface tells whether its signs mean anything.  `sign="winding"` takes the
    signs from the generalized winding number instead (`signed_point_to_surface_distances`): the choice for open or
    non-manifold meshes; the unsigned entries are the same either way."""
    pts_a, faces_a = checked_mesh(mesh_a)
    pts_b, faces_b = checked_mesh(mesh_b)
    _check_sign(sign)
    sd_ab = sd_ba = None
    with contextlib.ExitStack() as built:
        if surface_b is None:
            surface_b = built.enter_context(_hip.DeviceSurface(pts_b, faces_b, ctx=ctx))
        if signed:  # |sd| is the unsigned distance bit for bit: one search per direction
            sd_ab = _signed_on_surface(surface_b, pts_a, sign)[0]
            d_ab = np.abs(sd_ab)
        else:
            d_ab = np.sqrt(surface_b.distance(pts_a)[0])
        d_ba = None
        if symmetric:
            if surface_a is None:
                surface_a = built.enter_context(_hip.DeviceSurface(pts_a, faces_a, ctx=ctx))
            if signed:
                sd_ba = _signed_on_surface(surface_a, pts_b, sign)[0]
                d_ba = np.abs(sd_ba)
            else:
                d_ba = np.sqrt(surface_a.distance(pts_b)[0])
    out = summarize_distances(d_ab, d_ba)
    for tag, sd in (("a_to_b", sd_ab), ("b_to_a", sd_ba)):
        if sd is not None:
            out.update({"%s_%s" % (k, tag): v for k, v in summarize_signed_distances(sd).items()})
    return out
