"""The mesh units at the edges of what they share (pf_halfedge.h, pf_sort_pairs, pf_index_bits): vertex counts at which
the bits of an index change, and the smallest meshes there are.  Each test runs on a context of its own, so no buffer
and no cached block is there before it.

`test_topology.py` and `test_curvature.py` already run a closed mesh of n = 4 (the tetrahedron: two index bits, no
boundary) and meshes of hundreds of vertices; they have no open mesh at 2^k and 2^k + 1 vertices, no mesh of fewer than
four faces, and none whose only shared edge is inconsistent.  Those are here."""
import numpy as np
import pytest

import _curvature_ref as cref
import _remesh_ref as rref
import _signed_ref as sref
import _topology_ref as tref

EPS = np.finfo(np.float64).eps


def strip(n):
    """A consistently oriented triangle strip over n vertices (n - 2 faces), not flat."""
    i = np.arange(n)
    pts = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.1 * np.sin(i)], axis=1)
    t = np.arange(n - 2)
    faces = np.where((t % 2 == 0)[:, None], np.stack([t, t + 1, t + 2], axis=1), np.stack([t + 1, t, t + 2], axis=1))
    return np.ascontiguousarray(pts), np.ascontiguousarray(faces, dtype=np.int32)


_PTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [0.5, 0.5, 1.0]])
_SMALL = {
    "one_triangle": (np.ascontiguousarray(_PTS[:3]), np.array([[0, 1, 2]], dtype=np.int32)),      # n = 3, H = 3
    "same_direction": (_PTS, np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)),  # both faces go 0 -> 1: one inconsistent edge
}
_WANT_COUNTS = {"one_triangle": [3, 3, 0, 0], "same_direction": [5, 4, 0, 1]}  # edges | boundary | non-manifold | inconsistent


@pytest.fixture
def fresh():
    from pyfocusr_amd import _hip

    _hip.load_library()
    ctx = _hip.Context(0)
    yield ctx
    ctx.close()


def _assert_topology(ctx, pts, faces, what):
    r = tref.topology(len(pts), faces, pts, outward=True)
    dev = ctx.mesh_topology(len(pts), faces, points=pts)
    want = [r[k] for k in ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "n_patches", "n_boundary_loops")]
    assert dev["report"][:6].tolist() == want, (what, dev["report"].tolist(), want)
    for key in ("face_neighbours", "patch", "flip", "boundary_loop"):
        assert np.array_equal(dev[key], r[key]), (what, key)
    return dev, r


def _assert_curvature(ctx, pts, faces, what):
    r = cref.curvatures(pts, faces)
    dev = ctx.curvatures(pts, faces)
    assert np.array_equal(dev["topology"], r["topology"]), (what, dev["topology"].tolist(), r["topology"].tolist())
    assert np.array_equal(dev["boundary"], r["boundary"]), what
    return dev, r


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 16, 17])
def test_strips_where_the_index_bits_change(fresh, n):
    """n = 2^k and 2^k + 1: the key of an edge is (min << nb | max) with nb = 2 | 3 and 4 | 5 bits, and the highest vertex
    index is the largest value nb bits hold, or the first that needs one more."""
    pts, faces = strip(n)
    dev, r = _assert_topology(fresh, pts, faces, "strip %d" % n)
    assert dev["report"][:6].tolist() == [2 * n - 3, n, 0, 0, 1, 1]  # an open disc
    _assert_curvature(fresh, pts, faces, "strip %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_SMALL))
def test_smallest_meshes_through_every_unit(fresh, name):
    """Three and six half-edges: every sort of the four units runs on fewer items than one thread block holds."""
    from pyfocusr_amd import _hip

    pts, faces = _SMALL[name]
    counts = _WANT_COUNTS[name]
    assert list(sref.topology_counts(faces)) == counts
    # topology
    dev, _ = _assert_topology(fresh, pts, faces, name)
    assert dev["report"][:4].tolist() == counts
    # curvatures: the reference's counts and masks.  No edge here has two faces that agree, so no edge has a dihedral
    # angle: H and the tensor are exact zeros.  The areas take products, sums, a square root and divisions in the
    # reference's order: its bits.  K = (2 pi - angles) / A: at most two angles of a few ulp each in either libm, then
    # a sum, a difference and a division.
    dev, r = _assert_curvature(fresh, pts, faces, name)
    assert dev["topology"][:4].tolist() == counts and dev["boundary"].all()
    assert np.array_equal(dev["area"], r["area"]) and np.all(dev["area"] > 0.0)
    assert np.all(dev["mean"] == 0.0) and np.all(dev["tensor"] == 0.0)
    assert np.all(np.abs(dev["gaussian"] - r["gaussian"]) <= 16 * EPS * r["mag_gauss"]), name
    # clusters: m = 1, every vertex in the one cluster, no face with three labels
    mass = rref.vertex_areas(pts, faces)
    want = rref.cluster(pts, faces, mass, [1], 2)
    got = fresh.cluster_mesh(pts, faces, mass, seeds=[1], n_iter=2)
    for key in ("labels", "centroids", "rep", "count", "changed", "faces", "face_src", "votes"):
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key], dtype=np.asarray(got[key]).dtype).tobytes(), (name, key)
    assert got["n_iter_run"] == want["n_iter_run"] and got["n_candidate_faces"] == 0 and got["count"].tolist() == [len(pts)]
    # signed distances: the counts, and the vertex pseudonormals sum of angle x unit normal over the corners of a vertex
    surface = _hip.DeviceSurface(pts, faces, ctx=fresh)
    try:
        assert surface._prepare_signed().tolist() == counts
        vn = surface.vertex_normals()
    finally:
        surface.close()
    X = pts[faces]
    cr = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    tn = cr / np.linalg.norm(cr, axis=1)[:, None]
    ref_vn, angsum = np.zeros_like(pts), np.zeros(len(pts))
    for t, f in enumerate(faces):
        for j in range(3):
            e1, e2 = X[t, (j + 1) % 3] - X[t, j], X[t, (j + 2) % 3] - X[t, j]
            ang = np.arctan2(np.linalg.norm(np.cross(e1, e2)), np.dot(e1, e2))
            ref_vn[f[j]] += ang * tn[t]
            angsum[f[j]] += ang
    # an angle and a unit normal of these well-shaped triangles carry a few eps each, their product and the sum one more
    assert np.all(np.abs(vn - ref_vn) <= 16 * EPS * angsum[:, None]), (name, np.abs(vn - ref_vn).max())
