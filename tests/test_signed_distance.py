"""Signed point-to-surface distances (`pf_surface_prepare_signed`, `pf_surface_signed_distance`, the signed functions of
`pyfocusr_amd.surface_distance`).

CPU: the C-ABI declarations, the pure summary helper against plain numpy, argument errors before any device call, and
the numpy edge counts of a defective mesh.  GPU: the magnitude and face bit for bit against the unsigned call, the sign
against an independent ground truth (star-shaped blobs, the generalized winding number), an analytic cube, orientation,
robustness, and point data through the VTK writer and reader."""
import os
import re

import numpy as np
import pytest

import _signed_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_mesh(n, z=0.0):
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], axis=1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)  # normals +z
    return pts, faces


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name,n_args", [("pf_surface_prepare_signed", 4), ("pf_surface_signed_distance", 7)])
def test_signed_entry_points_are_declared_and_bound(name, n_args):
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, "%s is not declared in the header" % name
    assert len(m.group(1).split(",")) == n_args
    _, argtypes = _hip.SIGNATURES[name]
    assert len(argtypes) == n_args


def test_signed_summary_equals_numpy():
    from pyfocusr_amd import summarize_signed_distances

    rng = np.random.default_rng(3)
    sd = rng.normal(size=2001)
    sd[[10, 700]] = sd.min() - 1.0     # a tie for the minimum: the lowest index is reported
    sd[[50, 900]] = sd.max() + 1.0     # and for the maximum
    sd[[3, 4]] = 0.0
    sd[[5, 1500]] = np.nan             # counted and left out
    sd[1600] = np.inf
    s = summarize_signed_distances(sd)
    f = sd[np.isfinite(sd)]
    assert s["n"] == len(f) == 1998 and s["n_nan"] == 3
    np.testing.assert_allclose(s["mean_signed"], np.mean(f), rtol=1e-14)
    np.testing.assert_allclose(s["std_signed"], np.std(f), rtol=1e-14)
    assert s["min_signed"] == f.min() and s["min_signed_vertex"] == 10
    assert s["max_signed"] == f.max() and s["max_signed_vertex"] == 50
    assert s["n_inside"] == np.sum(f < 0) and s["n_outside"] == np.sum(f > 0) and s["n_on"] == 2
    assert s["n_inside"] + s["n_outside"] + s["n_on"] == s["n"]
    none = summarize_signed_distances(np.array([np.nan, np.nan]))
    assert none["n"] == 0 and none["n_nan"] == 2 and none["min_signed_vertex"] == -1 and np.isnan(none["mean_signed"])


def test_signed_argument_errors_before_any_device_call(monkeypatch):
    from pyfocusr_amd import _hip, surface_distance

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceSurface", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    pts, faces = _grid_mesh(4)
    for q, mesh in [(np.zeros((0, 3)), (pts, faces)), (np.zeros((5, 2)), (pts, faces)), (np.zeros(3), (pts, faces)),
                    (pts, (pts, np.zeros((0, 3), dtype=np.int32))), (pts, (pts, faces.ravel())), (pts, (pts[:0], faces))]:
        with pytest.raises(ValueError):
            surface_distance.signed_point_to_surface_distances(q, mesh)
    with pytest.raises(ValueError):
        surface_distance.signed_distances_on_mesh((pts[:0], faces), (pts, faces))
    with pytest.raises(ValueError):
        surface_distance.signed_distances_on_mesh((pts, faces), (pts, faces[:, :2]))
    with pytest.raises(ValueError):
        surface_distance.surface_distance_metrics((pts, faces), (pts, faces[:0]), signed=True)


def test_topology_counts_of_messy_blob():
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    n = 3000
    assert ref.topology_counts(blob_mesh(n).faces) == (3 * n - 6, 0, 0, 0)  # closed genus 0: E = 3V - 6
    e, boundary, nonmanifold, inconsistent = ref.topology_counts(messy_blob_mesh(n).faces)
    # 7 deleted faces (7 x 3 one-triangle edges), 3 stars of 6 faces (3 x 6), 2 fins (2 new edges each, 1 edge in
    # three faces each), 2 flipped faces (3 edges each traversed twice the same way)
    assert (boundary, nonmanifold, inconsistent) == (7 * 3 + 3 * 6 + 2 * 2, 2, 2 * 3)
    assert e == 3 * n - 6 - 3 * 6 + 2 * 2  # the stars' spokes are gone; each fin adds two edges


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


def _signed_and_unsigned(ctx, pts, faces, q):
    from pyfocusr_amd import _hip

    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        d2, face, _ = surf.distance(q)
        sd, sface, feature, amb = surf.signed_distance(q)
    finally:
        surf.close()
    return sd, sface, feature, amb, d2, face


def _assert_magnitude_exact(sd, sface, d2, face):
    assert np.array_equal(np.abs(sd), np.sqrt(d2), equal_nan=True)
    assert np.array_equal(sface, face)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15000, 250000])
def test_magnitude_and_face_bitwise_on_blob_pairs(ctx, n):
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(n, seed=0), blob_mesh(n, seed=1)
    sd, sface, feature, amb, d2, face = _signed_and_unsigned(ctx, b.points, b.faces, a.points)
    _assert_magnitude_exact(sd, sface, d2, face)
    assert amb == 0 and set(np.unique(feature)) <= {0, 1, 2}
    assert np.sum(sd < 0) > 0 and np.sum(sd > 0) > 0  # the two shapes cross each other


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["target_mesh", "source_mesh", "target_mesh_15k", "source_mesh_15k"])
def test_magnitude_and_face_bitwise_on_goldens(ctx, golden, name):
    from pyfocusr_amd import signed_point_to_surface_distances

    g = golden(name)
    pts, faces = g["points"], g["faces"]
    rng = np.random.default_rng(4)
    step = max(1, len(pts) // 1500)
    q = np.concatenate([pts[::step] + rng.normal(size=pts[::step].shape), pts[rng.integers(0, len(pts), 200)],
                        rng.uniform(pts.min(0) - 50, pts.max(0) + 50, size=(200, 3))])
    sd, sface, _, _, d2, face = _signed_and_unsigned(ctx, pts, faces, q)
    _assert_magnitude_exact(sd, sface, d2, face)
    sd2, face2 = signed_point_to_surface_distances(q, (pts, faces), ctx=ctx, check_orientation=False)
    assert np.array_equal(sd2, sd) and np.array_equal(face2, face)


@pytest.mark.gpu
def test_sign_against_star_shape_and_winding_number(ctx):
    from pyfocusr_amd import _hip
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(15000, seed=2)
    surf = _hip.DeviceSurface(m.points, m.faces, ctx=ctx)
    try:
        topo = surf.topology()
        assert topo["closed"] and topo["volume"] > 0 and topo["n_inconsistent_edges"] == 0
        # star-shaped about the origin: t x vertex is inside for t < 1, outside for t > 1
        for t in (0.5, 0.9, 0.999, 1.001, 1.1, 2.0):
            sd, _, _, amb = surf.signed_distance(t * m.points)
            assert amb == 0
            assert np.all(sd < 0) if t < 1 else np.all(sd > 0), t
        # random points of the bounding box, judged by the generalized winding number
        rng = np.random.default_rng(9)
        q = rng.uniform(m.points.min(0), m.points.max(0), size=(600, 3))
        w = ref.winding_number(m.points, m.faces, q)
        assert np.all(np.abs(w - np.round(w)) < 1e-6) and set(np.round(w)) <= {0.0, 1.0}
        sd, _, _, amb = surf.signed_distance(q)
        assert amb == 0
        assert np.array_equal(sd < 0, np.round(w) == 1.0)
    finally:
        surf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["quads", "triangles"])
def test_analytic_cube(ctx, kind):
    from pyfocusr_amd import _hip

    pts, faces = ref.cube_quads() if kind == "quads" else ref.cube_triangles()
    rng = np.random.default_rng(21)
    q = np.concatenate([rng.uniform(-3, 3, size=(4000, 3)), rng.uniform(-0.97, 0.97, size=(1000, 3))])
    want_feature, c = ref.box_feature(q)
    e = np.abs(q) - 1.0
    # keep clear of the region boundaries: the queries' distance to the boundary planes of the cube's regions ...
    keep = np.all(np.abs(e) > 1e-3, axis=1)
    srt = np.sort(np.abs(q), axis=1)
    keep &= ~((want_feature == 0) & np.all(e < 0, axis=1) & (srt[:, 2] - srt[:, 1] < 1e-3))  # inside: a unique face
    # ... and, for the face queries, of the quads' fan diagonals (they are edges of the triangulation)
    quads = ref.cube_quads()[1]
    for f in quads:
        a, b = pts[f[0]], pts[f[2]]
        axis = int(np.flatnonzero(a == b)[0])  # the face's constant coordinate
        on = (want_feature == 0) & (c[:, axis] == a[axis])
        u = (b - a) / np.linalg.norm(b - a)
        r = (c - a) - np.outer((c - a) @ u, u)
        keep &= ~(on & (np.linalg.norm(r, axis=1) < 1e-3))
    q, want_feature = q[keep], want_feature[keep]
    assert all(np.sum(want_feature == k) > 100 for k in (0, 1, 2))
    assert np.sum(np.all(np.abs(q) < 1, axis=1)) > 500

    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        topo = surf.topology()
        sd, _, feature, amb = surf.signed_distance(q)
    finally:
        surf.close()
    assert topo["closed"] and topo["n_inconsistent_edges"] == 0 and topo["volume"] == 8.0
    assert topo["n_edges"] == 18  # 12 cube edges + 6 diagonals
    want = ref.box_signed_distance(q)
    np.testing.assert_allclose(sd, want, rtol=0, atol=1e-12)
    assert np.array_equal(np.sign(sd), np.sign(want))
    assert amb == 0
    assert np.array_equal(feature, want_feature)


@pytest.mark.gpu
def test_orientation_reversal_defects_and_open_grid(ctx):
    from pyfocusr_amd import _hip, signed_point_to_surface_distances
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    # reversing every face flips every sign; each magnitude stays its own mesh's unsigned distance
    m = blob_mesh(5000, seed=3)
    rng = np.random.default_rng(6)
    q = m.points * rng.uniform(0.8, 1.2, size=(len(m.points), 1))
    rev = m.faces[:, ::-1].copy()
    sd, sface, _, amb, d2, face = _signed_and_unsigned(ctx, m.points, m.faces, q)
    sd_r, sface_r, _, amb_r, d2_r, face_r = _signed_and_unsigned(ctx, m.points, rev, q)
    _assert_magnitude_exact(sd_r, sface_r, d2_r, face_r)
    assert amb == amb_r == 0
    assert np.array_equal(np.sign(sd_r), -np.sign(sd)) and np.all(sd != 0)
    # the reversed triangles are other operands of the exact test, so the last bits of d2 may differ
    np.testing.assert_allclose(sd_r, -sd, rtol=1e-12, atol=1e-12)

    # the device's edge counts of a defective mesh are numpy's; the orientation check refuses it
    messy = messy_blob_mesh(3000)
    surf = _hip.DeviceSurface(messy.points, messy.faces, ctx=ctx)
    try:
        t = surf.topology()
    finally:
        surf.close()
    assert (t["n_edges"], t["n_boundary_edges"], t["n_nonmanifold_edges"], t["n_inconsistent_edges"]) \
        == ref.topology_counts(messy.faces)
    assert not t["closed"]
    with pytest.raises(ValueError, match="inconsistent"):
        signed_point_to_surface_distances(messy.points[:10], messy, ctx=ctx)
    surf = _hip.DeviceSurface(m.points, rev, ctx=ctx)
    try:
        assert surf.topology()["volume"] < 0  # inward faces
    finally:
        surf.close()

    # an open, flat grid (normals +z) is accepted; the sign is that of z, also beyond its boundary
    pts, faces = _grid_mesh(12)
    g = np.random.default_rng(10).uniform(-3, 14, size=(3000, 3))
    g[:, 2] = np.where(np.abs(g[:, 2]) < 1e-3, 0.5, g[:, 2])
    sd, face = signed_point_to_surface_distances(g, (pts, faces), ctx=ctx)
    assert np.array_equal(np.sign(sd), np.sign(g[:, 2]))
    inner = np.all((g[:, :2] > 0) & (g[:, :2] < 11), axis=1)
    np.testing.assert_allclose(sd[inner], g[inner, 2], rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_nan_repeat_and_degenerate_triangles(ctx, golden):
    from pyfocusr_amd import _hip

    g = golden("target_mesh")
    rng = np.random.default_rng(2)
    q = g["points"][::7] + rng.normal(size=g["points"][::7].shape)
    q[[3, 100, 101]] = np.nan
    q[200, 1] = np.inf
    surf = _hip.DeviceSurface(g["points"], g["faces"], ctx=ctx)
    try:
        sd, face, feature, amb = surf.signed_distance(q)
        again = surf.signed_distance(q)
        d2, dface, _ = surf.distance(q)
    finally:
        surf.close()
    bad = [3, 100, 101, 200]
    assert np.all(np.isnan(sd[bad])) and np.all(face[bad] == -1) and np.all(feature[bad] == -1)
    assert np.all(np.isfinite(np.delete(sd, bad))) and np.all(np.delete(feature, bad) >= 0)
    _assert_magnitude_exact(sd, face, d2, dface)
    assert np.array_equal(again[0], sd, equal_nan=True) and np.array_equal(again[1], face)
    assert np.array_equal(again[2], feature) and again[3] == amb
    assert np.array_equal(again[0].view(np.int64), sd.view(np.int64))  # identical bits, signs of zeros included

    # the degenerate triangle sets of the unsigned tests: zero normals, never NaN for a finite query
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(300, 3))
    quads = rng.integers(0, 300, size=(500, 4)).astype(np.int32)
    deg = rng.integers(0, 300, size=(400, 3)).astype(np.int32)
    deg[:40, 1] = deg[:40, 0]
    deg[40:60] = deg[40:60, :1]
    deg[60:80, 2] = deg[60:80, 1]
    for faces, qq in ((quads, rng.normal(size=(700, 3)) * 2), (deg, rng.normal(size=(500, 3)) * 2),
                      (deg, rng.normal(size=(65, 3)) * 1.5), (deg, pts[:50])):
        sd, sface, feature, _, d2, face = _signed_and_unsigned(ctx, pts, faces, qq)
        assert not np.any(np.isnan(sd))
        _assert_magnitude_exact(sd, sface, d2, face)
        assert np.all((feature >= 0) & (feature <= 2))


@pytest.mark.gpu
def test_signed_point_data_round_trip_and_metrics(ctx, tmp_path):
    from pyfocusr_amd import (read_vtk_mesh, signed_distances_on_mesh, summarize_signed_distances, surface_distance_metrics,
                              write_vtk_mesh)
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(3000, seed=0), blob_mesh(3000, seed=1)
    sd = signed_distances_on_mesh(a, b, ctx=ctx)
    assert dict(a.point_data)["signed_distance"] is not sd and np.array_equal(dict(a.point_data)["signed_distance"], sd)
    path = str(tmp_path / "a.vtk")
    write_vtk_mesh(a, path)
    back = dict(read_vtk_mesh(path).point_data)["signed_distance"]
    assert np.array_equal(back, sd)

    plain = surface_distance_metrics(a, b, ctx=ctx)
    m = surface_distance_metrics(a, b, ctx=ctx, signed=True)
    for k, v in plain.items():
        assert m[k] == v, k  # the unsigned keys, bit for bit
    s_ab = summarize_signed_distances(sd)
    for k, v in s_ab.items():
        assert m[k + "_a_to_b"] == v, k
    assert m["n_inside_b_to_a"] + m["n_outside_b_to_a"] + m["n_on_b_to_a"] == 3000
