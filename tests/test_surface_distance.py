"""Surface distances between meshes (`pf_surface_distance`, `pyfocusr_amd.surface_distance`, `pyfocusr_amd.test`).

CPU: the C-ABI declaration, the pure summary helper against plain numpy, argument errors before any device call, and
the pairwise driver with the device and ICP replaced.  GPU: squared distances and faces bit-identical to the brute-force
oracle and to `pf_surface_closest`, the device statistics, and known answers."""
import os
import re

import numpy as np
import pytest

from oracle import icp_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sphere_mesh(n, radius):
    from scipy.spatial import ConvexHull

    from pyfocusr_amd.meshgen import fibonacci_sphere

    u = fibonacci_sphere(n)
    return radius * u, ConvexHull(u).simplices.astype(np.int32)


def _grid_mesh(n, z=0.0):
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], axis=1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return pts, faces


# ------------------------------------------------------------------------------ CPU
def test_distance_entry_point_is_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_surface_distance\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_surface_distance is not declared in the header"
    assert len(m.group(1).split(",")) == 6
    restype, argtypes = _hip.SIGNATURES["pf_surface_distance"]
    assert len(argtypes) == 6


def test_summary_helper_equals_numpy():
    from pyfocusr_amd.surface_distance import summarize_distances

    rng = np.random.default_rng(0)
    d_ab, d_ba = rng.random(1001) * 3, rng.random(517) * 2
    d_ab[[17, 400]] = d_ab.max() + 1.0    # a tie for the maximum: the lowest index is reported
    d_ba[5] = np.nan                      # non-finite distances are counted and left out
    m = summarize_distances(d_ab, d_ba)
    fb = d_ba[np.isfinite(d_ba)]
    assert m["n_a_to_b"] == 1001 and m["n_nan_a_to_b"] == 0 and m["n_b_to_a"] == 516 and m["n_nan_b_to_a"] == 1
    np.testing.assert_allclose(m["mean_a_to_b"], np.mean(d_ab), rtol=1e-14)
    np.testing.assert_allclose(m["mean_b_to_a"], np.mean(fb), rtol=1e-14)
    np.testing.assert_allclose(m["rms_a_to_b"], np.sqrt(np.mean(d_ab ** 2)), rtol=1e-14)
    np.testing.assert_allclose(m["rms_b_to_a"], np.sqrt(np.mean(fb ** 2)), rtol=1e-14)
    np.testing.assert_allclose(m["assd"], (d_ab.sum() + fb.sum()) / (len(d_ab) + len(fb)), rtol=1e-14)
    assert m["max_a_to_b"] == d_ab.max() and m["max_a_to_b_vertex"] == 17
    assert m["max_b_to_a"] == fb.max() and m["max_b_to_a_vertex"] == int(np.nanargmax(d_ba))
    assert m["hausdorff"] == max(d_ab.max(), fb.max())
    assert m["p95_a_to_b"] == np.percentile(d_ab, 95) and m["p95_b_to_a"] == np.percentile(fb, 95)
    assert m["hausdorff_95"] == max(np.percentile(d_ab, 95), np.percentile(fb, 95))
    one = summarize_distances(d_ab)
    assert "assd" not in one and one["mean_a_to_b"] == m["mean_a_to_b"]
    none = summarize_distances(np.array([np.nan]))
    assert none["n_a_to_b"] == 0 and none["max_a_to_b_vertex"] == -1 and np.isnan(none["mean_a_to_b"])


def test_argument_errors_before_any_device_call(monkeypatch):
    from pyfocusr_amd import _hip, surface_distance

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceSurface", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    pts, faces = _grid_mesh(4)
    with pytest.raises(ValueError):
        surface_distance.point_to_surface_distances(np.zeros((0, 3)), (pts, faces))
    with pytest.raises(ValueError):
        surface_distance.point_to_surface_distances(np.zeros((5, 2)), (pts, faces))
    with pytest.raises(ValueError):
        surface_distance.point_to_surface_distances(np.zeros(3), (pts, faces))
    with pytest.raises(ValueError):
        surface_distance.point_to_surface_distances(pts, (pts, np.zeros((0, 3), dtype=np.int32)))
    with pytest.raises(ValueError):
        surface_distance.point_to_surface_distances(pts, (pts, faces.ravel()))
    with pytest.raises(ValueError):
        surface_distance.surface_distance_metrics((pts, faces), (pts, np.zeros((0, 3), dtype=np.int32)))
    with pytest.raises(ValueError):
        surface_distance.surface_distance_metrics((pts[:0], faces), (pts, faces))


def test_pairwise_driver_shape_diagonal_icp_direction_and_one_surface_per_mesh(monkeypatch, tmp_path):
    from pyfocusr_amd import PolyMesh, _hip, test as pairwise, vtk_functions

    names = []
    for k in range(3):
        pts, faces = _grid_mesh(3 + k)
        vtk_functions.write_vtk_mesh(PolyMesh(pts + 100.0 * k, faces), str(tmp_path / ("m%d.vtk" % k)))
        names.append("m%d.vtk" % k)
    ident = lambda mesh: int(round(mesh.points[0, 0] / 100.0))  # noqa: E731

    built = []

    class FakeSurface(object):
        def __init__(self, points, faces, ctx=None):
            self.mesh = int(round(points[0, 0] / 100.0))
            built.append(self.mesh)

        def close(self):
            pass

    icp_calls = []

    class FakeTransform(object):
        def __init__(self, target, source):
            self.target, self.source = target, source

    def fake_icp(target, source, ctx=None, **kw):
        icp_calls.append((ident(target), ident(source)))
        return FakeTransform(ident(target), ident(source))

    def fake_apply(source, transform):
        assert ident(source) == transform.source
        return PolyMesh(source.points + 1000.0 * (transform.target + 1), source.faces)

    def fake_metrics(mesh_a, mesh_b, symmetric=True, ctx=None, surface_a=None, surface_b=None):
        assert not symmetric and surface_a is None and surface_b.mesh == ident(mesh_b)
        x = mesh_a.points[0, 0]  # 100 * source + 1000 * (target + 1), set by fake_apply
        src, moved_onto = int(round((x % 1000.0) / 100.0)), int(x // 1000.0) - 1
        assert moved_onto == ident(mesh_b)
        return {"mean_a_to_b": 10.0 * (src + 1) + moved_onto + 1}

    monkeypatch.setattr(_hip, "DeviceSurface", FakeSurface)
    monkeypatch.setattr(vtk_functions, "icp_transform", fake_icp)
    monkeypatch.setattr(vtk_functions, "apply_transform", fake_apply)
    monkeypatch.setattr(pairwise, "surface_distance_metrics", fake_metrics)
    errors = pairwise.get_all_pairwise_surface_errors(names, str(tmp_path))
    assert errors.shape == (3, 3) and np.all(np.diag(errors) == 0)
    for i in range(3):
        for j in range(3):
            if i != j:
                assert errors[i, j] == 10.0 * (i + 1) + j + 1  # mesh i moved onto mesh j, measured against j
    assert sorted(icp_calls) == sorted((j, i) for i in range(3) for j in range(3) if i != j)  # (target j, source i)
    assert sorted(built) == [0, 1, 2]  # one surface per mesh, reused across the pairs


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


def _distance(ctx, pts, faces, q):
    from pyfocusr_amd import _hip

    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        return surf.distance(q)
    finally:
        surf.close()


def _check_brute(ctx, pts, faces, q):
    d2, face, stats = _distance(ctx, pts, faces, q)
    _, want_face, want_d2 = icp_port.closest_points_on_surface(pts, faces, q)
    assert np.array_equal(d2, want_d2)
    assert np.array_equal(face, want_face)
    return d2, face, stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["target_mesh", "source_mesh", "target_mesh_15k", "source_mesh_15k"])
def test_distance_equals_brute_force_goldens(golden, ctx, name):
    g = golden(name)
    pts, faces = g["points"], g["faces"]
    rng = np.random.default_rng(11)
    lo, hi = pts.min(0), pts.max(0)
    step = max(1, len(pts) // 1200)
    near = pts[::step][:1200]
    q = np.concatenate([
        near + rng.normal(size=near.shape) * 0.5,               # near the surface
        pts[rng.integers(0, len(pts), 300)],                    # on vertices: distance 0, ties between faces
        rng.uniform(lo - 200, hi + 200, size=(150, 3)),         # far outside the surface's box / inside it
        np.repeat(near[:50], 3, axis=0),                        # duplicates
    ])
    d2, _, _ = _check_brute(ctx, pts, faces, q)
    assert np.all(d2[1200:1500] == 0.0)


@pytest.mark.gpu
def test_distance_quads_degenerate_and_small_counts(ctx):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(300, 3))
    faces = rng.integers(0, 300, size=(500, 4)).astype(np.int32)   # quads (vpf = 4)
    _check_brute(ctx, pts, faces, rng.normal(size=(700, 3)) * 2)
    deg = rng.integers(0, 300, size=(400, 3)).astype(np.int32)
    deg[:40, 1] = deg[:40, 0]                                        # zero-area: two corners equal
    deg[40:60] = deg[40:60, :1]                                      # all corners equal: a point
    deg[60:80, 2] = deg[60:80, 1]
    _check_brute(ctx, pts, deg, rng.normal(size=(500, 3)) * 2)
    for n in (1, 63, 64, 65):
        _check_brute(ctx, pts, deg, rng.normal(size=(n, 3)) * 1.5)


@pytest.mark.gpu
def test_distance_nan_queries_are_counted_and_excluded(ctx, golden):
    g = golden("target_mesh")
    pts, faces = g["points"], g["faces"]
    rng = np.random.default_rng(2)
    q = pts[::7] + rng.normal(size=pts[::7].shape)
    bad = q.copy()
    bad[[3, 100, 101]] = np.nan
    bad[200, 1] = np.inf
    d2, face, stats = _distance(ctx, pts, faces, bad)
    keep = np.ones(len(q), dtype=bool)
    keep[[3, 100, 101, 200]] = False
    assert np.all(np.isnan(d2[~keep])) and np.all(face[~keep] == -1)
    _, want_face, want_d2 = icp_port.closest_points_on_surface(pts, faces, q[keep])
    assert np.array_equal(d2[keep], want_d2) and np.array_equal(face[keep], want_face)
    assert stats["n_nan"] == 4 and stats["n_finite"] == keep.sum()
    d = np.sqrt(d2[keep])
    np.testing.assert_allclose(stats["sum_d"], d.sum(), rtol=1e-12)
    assert stats["argmax"] == np.flatnonzero(keep)[np.argmax(d)]


@pytest.mark.gpu
def test_distance_stats_agree_with_numpy_and_repeat_bit_for_bit(ctx):
    from pyfocusr_amd import _hip
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(20000, seed=0), blob_mesh(20000, seed=1)
    surf = _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
    d2, face, stats = surf.distance(a.points)
    d2_again, face_again, stats_again = surf.distance(a.points)
    _, _, stats_only = surf.distance(a.points, per_point=False)
    surf.close()
    d = np.sqrt(d2)
    assert stats["n_finite"] == len(d) and stats["n_nan"] == 0
    np.testing.assert_allclose(stats["sum_d"], d.sum(), rtol=1e-12)
    np.testing.assert_allclose(stats["sum_d2"], np.sum(d * d), rtol=1e-12)
    assert abs(stats["max_d"] - d.max()) <= np.spacing(d.max())
    assert stats["argmax"] == int(np.argmax(d))
    assert stats == stats_again == stats_only
    assert np.array_equal(d2, d2_again) and np.array_equal(face, face_again)


@pytest.mark.gpu
def test_distance_full_size_equals_closest_kernel(ctx):
    """Every vertex of a 250k mesh against another 250k mesh: bit for bit the existing per-query kernel's answer."""
    from pyfocusr_amd import _hip
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(250000, seed=0), blob_mesh(250000, seed=1)
    surf = _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
    _, want_face, want_d2 = surf.closest(a.points)
    d2, face, _ = surf.distance(a.points)
    surf.close()
    assert np.array_equal(d2, want_d2)
    assert np.array_equal(face, want_face)


@pytest.mark.gpu
def test_metrics_known_answers(ctx, golden):
    from pyfocusr_amd import PolyMesh, surface_distance_metrics

    g = golden("source_mesh")
    same = surface_distance_metrics(PolyMesh(g["points"], g["faces"]), (g["points"], g["faces"]), ctx=ctx)
    for key in ("mean_a_to_b", "mean_b_to_a", "assd", "rms_a_to_b", "hausdorff", "hausdorff_95"):
        assert same[key] == 0.0, key

    pts, faces = _grid_mesh(40)
    t = -0.375
    m = surface_distance_metrics((pts, faces), (pts + [0.0, 0.0, t], faces), ctx=ctx)
    for key in ("assd", "hausdorff", "hausdorff_95", "mean_a_to_b", "mean_b_to_a", "rms_b_to_a"):
        np.testing.assert_allclose(m[key], abs(t), rtol=1e-12, err_msg=key)

    def sag(p, f, r):  # how far the flat faces sink below the sphere they are inscribed in
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        n = np.cross(b - a, c - a)
        return r - np.min(np.abs(np.einsum("ij,ij->i", n, a)) / np.linalg.norm(n, axis=1))

    for r in (1.2, 0.7):
        pa, fa = _sphere_mesh(4000, 1.0)
        pb, fb = _sphere_mesh(5000, r)
        tol = max(sag(pa, fa, 1.0), sag(pb, fb, r)) + 1e-12
        m = surface_distance_metrics((pa, fa), (pb, fb), ctx=ctx)
        assert abs(m["hausdorff"] - abs(r - 1)) <= tol and abs(m["assd"] - abs(r - 1)) <= tol
        lo = min(m["mean_a_to_b"], m["mean_b_to_a"])
        assert lo >= abs(r - 1) - tol and m["max_a_to_b"] <= abs(r - 1) + tol


@pytest.mark.gpu
def test_point_to_surface_distances_returns_distances(ctx, golden):
    from pyfocusr_amd import point_to_surface_distances

    g = golden("target_mesh")
    q = g["points"][::50] * 1.01
    d, face = point_to_surface_distances(q, (g["points"], g["faces"]), ctx=ctx)
    _, want_face, want_d2 = icp_port.closest_points_on_surface(g["points"], g["faces"], q)
    assert np.array_equal(d, np.sqrt(want_d2)) and np.array_equal(face, want_face)


@pytest.mark.gpu
def test_pairwise_errors_on_files(ctx, tmp_path):
    from pyfocusr_amd import get_all_pairwise_surface_errors, vtk_functions
    from pyfocusr_amd.meshgen import blob_mesh

    meshes = [blob_mesh(600 + 50 * k, seed=k) for k in range(3)]
    names = ["blob%d.vtk" % k for k in range(3)]
    for m, name in zip(meshes, names):
        vtk_functions.write_vtk_mesh(m, str(tmp_path / name))

    plain = get_all_pairwise_surface_errors(names, str(tmp_path), icp=False, ctx=ctx)
    with_icp = get_all_pairwise_surface_errors(names, str(tmp_path), icp=True, ctx=ctx)
    assert np.all(np.diag(plain) == 0) and np.all(np.diag(with_icp) == 0)
    for i in range(3):
        for j in range(3):
            if i == j:
                continue
            _, _, d2 = icp_port.closest_points_on_surface(meshes[j].points, meshes[j].faces, meshes[i].points)
            np.testing.assert_allclose(plain[i, j], np.mean(np.sqrt(d2)), rtol=1e-12)
            tr = vtk_functions.icp_transform(target=meshes[j], source=meshes[i], ctx=ctx)
            moved = vtk_functions.apply_transform(meshes[i], tr)
            _, _, d2 = icp_port.closest_points_on_surface(meshes[j].points, meshes[j].faces, moved.points)
            np.testing.assert_allclose(with_icp[i, j], np.mean(np.sqrt(d2)), rtol=1e-12)
