"""Discrete curvatures (`pf_curvatures`, `pyfocusr_amd.curvature`, the curvature helpers of `vtk_functions`).

CPU: the numpy reference `_curvature_ref.curvatures` against exact values (regular tetrahedron, the 26-vertex cube,
Gauss-Bonnet, trace T = 2 H, an open cylinder), the pure helpers, argument errors before the library is loaded, the
declaration and the helper names.  GPU: the device against that reference on seven meshes - integers and masks exactly,
floating-point fields relative to the magnitude of what was summed, under the bounds of profiles/curvature.md (8 x the
worst ratio measured on an MI355X) - two calls bit for bit, and point data through the VTK writer and reader."""
import os
import re

import numpy as np
import pytest

import _curvature_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps

# |device - reference| <= BOUND x magnitude, per vertex: 8 x the worst ratio over the seven meshes of this file, measured
# once on an MI355X (profiles/curvature.md, "Measured ratios"), as head-room for other meshes; none may be looser than
# 1e-10.  Magnitudes: the field itself for area, 1 for the unit normals, sum of angles / A for K, sum |e| |beta| / A for
# H and the six tensor entries, the Frobenius norm of S for the tensor's eigenvalues.  The areas came out with the
# reference's bits on every mesh (only products, sums, a square root and divisions, in the reference's order): 8 x 0.
BOUND = {"area": 0.0, "normals": 8 * 2.220e-16, "gaussian": 8 * 5.659e-16, "mean": 8 * 1.179e-16, "tensor": 8 * 1.991e-16,
         "tensor_k": 8 * 7.639e-16}
DIRECTION_GAP = 1e-3      # directions are compared where k_max - k_min > DIRECTION_GAP x max |k| of the mesh
DIRECTION_COS = 1.0 - 1e-8
DIRECTION_LEFT_OUT = 0.01  # at most this share of the vertices may fail the gap test


def _blob(n, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    return m.points, m.faces


def _messy():
    from pyfocusr_amd.meshgen import messy_blob_mesh

    m = messy_blob_mesh(700)
    return m.points, m.faces


_MESHES = {
    "tetrahedron": lambda: ref.tetrahedron(),                # n = 4: the fewest index bits
    "cube": lambda: ref.cube26()[:2],
    "blob700": lambda: _blob(700, 1),                        # 1396 faces: several blocks, n no multiple of the block
    "cylinder": lambda: ref.open_cylinder(),                 # boundary edges
    "messy700": _messy,                                      # non-manifold, one-way and unreferenced
    "cone": lambda: ref.cone_fan(200),                       # one vertex run of 200 half-edges
    "zero_area": lambda: ref.with_zero_area_triangle(*_blob(700, 1)),
}
_cache = {}


def case(name):
    """(points, faces, reference) of a test mesh, computed once and never changed."""
    if name not in _cache:
        pts, faces = _MESHES[name]()
        pts, faces = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32)
        r = ref.curvatures(pts, faces)
        for v in list(r.values()) + [pts, faces]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = (pts, faces, r)
    return _cache[name]


# ------------------------------------------------------------------------------ CPU
def test_curvature_entry_point_is_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_curvatures\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_curvatures is not declared in the header"
    assert len(m.group(1).split(",")) == 15
    assert len(_hip.SIGNATURES["pf_curvatures"][1]) == 15


def test_helper_names_exist():
    import pyfocusr_amd
    from pyfocusr_amd import vtk_functions

    for name in ("get_min_curvature", "get_max_curvature", "get_min_max_curvature_values"):
        assert callable(getattr(vtk_functions, name))
        assert "vtkCurvatures" in getattr(vtk_functions, name).__doc__
    for name in ("discrete_curvatures", "principal_curvatures", "shape_index", "curvedness", "curvature_on_mesh"):
        assert callable(getattr(pyfocusr_amd, name))


def test_reference_regular_tetrahedron():
    _, _, r = case("tetrahedron")
    assert np.array_equal(r["topology"], [6, 0, 0, 0, 0]) and not r["boundary"].any()
    np.testing.assert_allclose(r["gaussian"] * r["area"], np.pi, rtol=8 * EPS)  # 2 pi - 3 x pi / 3
    assert np.all(r["mean"] > 0.0)
    # edge 2 sqrt 2, dihedral angle pi - acos(1/3), three edges per vertex
    np.testing.assert_allclose(r["mean"] * r["area"], 0.25 * 3 * 2.0 * np.sqrt(2.0) * (np.pi - np.arccos(1.0 / 3.0)), rtol=16 * EPS)


def test_reference_cube():
    pts, faces, r = case("cube")
    kind = ref.cube26()[2]
    assert len(pts) == 26 and len(faces) == 48
    assert np.array_equal(r["topology"][:4], [72, 0, 0, 0]) and not r["boundary"].any()
    KA, HA = r["gaussian"] * r["area"], r["mean"] * r["area"]
    np.testing.assert_allclose(KA.sum(), 4.0 * np.pi, rtol=1e-14)
    np.testing.assert_allclose(HA.sum(), 3.0 * np.pi, rtol=1e-14)
    np.testing.assert_allclose(KA[kind == 3], np.pi / 2.0, rtol=1e-14)
    assert np.all(KA[kind != 3] == 0.0)
    assert np.all(r["mean"][kind == 1] == 0.0) and np.all(r["tensor"][kind == 1] == 0.0)
    mid = np.flatnonzero(kind == 2)
    assert len(mid) == 12
    for v in mid:
        axis = int(np.flatnonzero((pts[v] != 0.0) & (pts[v] != 1.0))[0])  # the cube edge runs along this axis
        e = np.eye(3)[axis]
        want = np.zeros(6)
        want[axis] = np.pi / 4.0  # (pi / 4) e e^T: two segments of length 1/2 with beta = pi / 2, half of each
        np.testing.assert_allclose(r["tensor"][v] * r["area"][v], want, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose([r["tensor_k_min"][v], r["tensor_k_max"][v]], [0.0, np.pi / (4.0 * r["area"][v])], rtol=1e-14,
                                   atol=1e-15)
        np.testing.assert_allclose(np.abs(r["d_min"][v]), e, atol=1e-15)  # along the edge
        assert abs(r["d_max"][v] @ e) < 1e-15 and abs(r["d_max"][v] @ r["normals"][v]) < 1e-15  # across it, in the surface
        np.testing.assert_allclose(np.linalg.norm(r["d_max"][v]), 1.0, rtol=1e-15)


def test_reference_gauss_bonnet():
    pts, faces, r = case("blob700")
    chi = len(pts) - int(r["topology"][0]) + len(faces)
    assert chi == 2
    np.testing.assert_allclose(np.sum(r["gaussian"] * r["area"]), 2.0 * np.pi * chi, rtol=1e-10)
    assert np.all(r["mean"] > 0.0)  # outward-oriented and star-shaped enough: convex in the mean everywhere


@pytest.mark.parametrize("name", ["blob700", "cylinder", "messy700", "cube"])
def test_reference_trace_of_the_tensor_is_twice_the_mean(name):
    _, _, r = case(name)
    trace = r["tensor"][:, 0] + r["tensor"][:, 1] + r["tensor"][:, 2]
    assert np.all(np.abs(trace - 2.0 * r["mean"]) <= 16 * EPS * r["trace_terms"])


def test_reference_open_cylinder():
    radius, n_around, n_along = 1.5, 48, 20
    pts, _, r = case("cylinder")
    assert np.array_equal(r["topology"][:4], [3 * n_around * (n_along - 1) + n_around, 2 * n_around, 0, 0])
    rim = np.zeros(len(pts), dtype=bool)
    rim[:n_around] = rim[-n_around:] = True
    assert np.array_equal(r["boundary"], rim)
    inner = ~rim
    assert np.all(np.abs(r["gaussian"][inner]) <= 16 * EPS * r["mag_gauss"][inner])  # a developable surface
    np.testing.assert_allclose(r["mean"][inner], 1.0 / (2.0 * radius), rtol=1e-3)
    np.testing.assert_allclose(r["tensor_k_min"][inner], 0.0, atol=1e-13)
    np.testing.assert_allclose(r["tensor_k_max"][inner], 1.0 / radius, rtol=1e-3)
    np.testing.assert_allclose(np.abs(r["d_min"][inner]), np.tile([0.0, 0.0, 1.0], (inner.sum(), 1)), atol=1e-12)  # the axis
    radial = pts[inner] * [1.0, 1.0, 0.0] / radius
    around = np.cross([0.0, 0.0, 1.0], radial)
    np.testing.assert_allclose(np.abs(np.sum(r["d_max"][inner] * around, axis=1)), 1.0, rtol=1e-12)


def test_shape_index_and_curvedness():
    from pyfocusr_amd import curvedness, shape_index

    k_min = np.array([-2.0, -2.0, -1.0, 0.0, 3.0, 0.0])
    k_max = np.array([-2.0, 0.0, 1.0, 4.0, 3.0, 0.0])
    np.testing.assert_allclose(shape_index(k_min, k_max), [-1.0, -0.5, 0.0, 0.5, 1.0, 0.0], atol=1e-15)  # cup rut saddle ridge cap flat
    np.testing.assert_allclose(curvedness(k_min, k_max), np.sqrt((k_min**2 + k_max**2) / 2.0), rtol=1e-15)
    with pytest.raises(ValueError):
        shape_index(k_min, k_max[:3])


def test_argument_errors_before_the_library_is_loaded(monkeypatch):
    from pyfocusr_amd import PolyMesh, _hip, curvature, vtk_functions

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    pts, faces = ref.tetrahedron()
    quads = np.array([[0, 1, 2, 3]], dtype=np.int32)
    nan_pts = pts.copy()
    nan_pts[2, 1] = np.nan
    bad = [(pts, quads), (pts, faces.ravel()), (pts, faces[:0]), (pts[:, :2], faces), (pts[:0], faces), (nan_pts, faces),
           (pts, faces + 1), (pts, faces - 1), (pts, faces.astype(np.float64))]
    for p, f in bad:
        with pytest.raises(ValueError):
            curvature.discrete_curvatures(p, f)
        with pytest.raises(ValueError):
            curvature.discrete_curvatures((p, f))
    with pytest.raises(ValueError):
        curvature.discrete_curvatures(PolyMesh(pts, quads))
    with pytest.raises(ValueError):
        vtk_functions.get_min_curvature(PolyMesh(pts, quads))
    with pytest.raises(ValueError):
        curvature.principal_curvatures((pts, faces), method="vtk")
    with pytest.raises(ValueError):
        curvature.curvature_on_mesh(PolyMesh(pts, faces), fields=("k_min", "torsion"))
    with pytest.raises(ValueError):
        curvature.curvature_on_mesh(PolyMesh(pts, faces), method="vtk")


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


_device = {}


def device(ctx, name):
    """`discrete_curvatures` of a test mesh: one device call per mesh and module."""
    if name not in _device:
        from pyfocusr_amd import discrete_curvatures

        pts, faces, _ = case(name)
        _device[name] = discrete_curvatures(pts, faces, ctx=ctx)
    return _device[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_MESHES))
def test_device_counts_and_masks_equal_the_reference(ctx, name):
    _, _, r = case(name)
    dev = device(ctx, name)
    print("%s: topology device %s reference %s" % (name, dev["topology"].tolist(), r["topology"].tolist()))
    assert dev["topology"].dtype == np.int64 and np.array_equal(dev["topology"], r["topology"])
    assert dev["boundary"].dtype == bool and np.array_equal(dev["boundary"], r["boundary"])
    assert np.array_equal(dev["area"] == 0.0, r["area"] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_MESHES))
def test_device_fields_against_the_reference(ctx, name):
    _, _, r = case(name)
    dev = device(ctx, name)
    got = ref.ratios(dev, r)
    for field in sorted(got):
        print("%s: %-9s worst ratio %.3e (bound %.3e)" % (name, field, got[field], BOUND[field]))
    for field in sorted(got):
        assert BOUND[field] <= 1e-10
        assert got[field] <= BOUND[field], (name, field, got[field])
    # the curvatures from (H, K) are exact functions of the device's own H and K: products, a difference and a square
    # root, each correctly rounded on either side and nothing contracted - the same bits.  (Against the reference's
    # they are not comparable by a relative bound: the square root has no finite condition at H^2 = K.)
    H, K = dev["mean"], dev["gaussian"]
    s = np.sqrt(np.maximum(H * H - K, 0.0))
    assert np.array_equal(dev["k_min"], H - s) and np.array_equal(dev["k_max"], H + s)
    zero = r["area"] == 0.0  # no area: zeros everywhere
    for field in ("gaussian", "mean", "k_min", "k_max", "tensor", "tensor_k_min", "tensor_k_max", "d_min", "d_max", "normals"):
        assert np.all(dev[field][zero] == 0.0)
    for field in ("area", "gaussian", "mean", "k_min", "k_max", "tensor", "tensor_k_min", "tensor_k_max", "d_min", "d_max", "normals"):
        assert np.all(np.isfinite(dev[field])), field


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob700", "cylinder", "messy700", "cone", "zero_area", "cube"])
def test_device_principal_directions(ctx, name):
    """The tetrahedron is left out: its vertices are umbilic by symmetry (S is a multiple of the identity), no vertex
    passes the gap test.  On the cube only the edge midpoints are compared: its face centres are flat and its corners
    close to umbilic."""
    _, _, r = case(name)
    dev = device(ctx, name)
    gap = r["tensor_k_max"] - r["tensor_k_min"]
    top = max(np.max(np.abs(r["tensor_k_min"])), np.max(np.abs(r["tensor_k_max"])))
    use = gap > DIRECTION_GAP * top
    if name == "cube":
        mid = ref.cube26()[2] == 2
        assert np.all(use[mid])
        use = mid
    else:
        left_out = 1.0 - np.mean(use)
        print("%s: %.2f %% of the vertices left out by the gap test" % (name, 100.0 * left_out))
        assert left_out <= DIRECTION_LEFT_OUT
    for field in ("d_min", "d_max"):
        cos = np.abs(np.sum(dev[field][use] * r[field][use], axis=1))
        print("%s: %s least |cos| - 1 = %.3e" % (name, field, np.min(cos) - 1.0))
        assert np.all(cos >= DIRECTION_COS)
        lead = dev[field][np.arange(len(use)), np.argmax(np.abs(dev[field]), axis=1)]
        assert np.all(lead[use] > 0.0)  # the sign rule
    framed = np.linalg.norm(dev["normals"], axis=1) > 0.0
    ortho = np.abs(np.sum(dev["d_min"] * dev["d_max"], axis=1)) + np.abs(np.sum(dev["d_min"] * dev["normals"], axis=1))
    assert np.all(ortho[framed] <= 64 * EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob700", "messy700", "cone"])
def test_two_calls_give_the_same_bits(ctx, name):
    from pyfocusr_amd import discrete_curvatures

    pts, faces, _ = case(name)
    a, b = device(ctx, name), discrete_curvatures(pts, faces, ctx=ctx)
    for field in sorted(a):
        if field != "device_ms":
            assert np.asarray(a[field]).tobytes() == np.asarray(b[field]).tobytes(), field


@pytest.mark.gpu
def test_library_refuses_a_bad_index(ctx):
    from pyfocusr_amd import _hip

    pts, faces = ref.tetrahedron()
    for bad in (faces + 1, faces - 1):
        with pytest.raises(_hip.PfError) as e:
            ctx.curvatures(pts, bad)  # (discrete_curvatures would have refused it first)
        assert e.value.code == -1 and "references vertex" in str(e.value)


@pytest.mark.gpu
def test_curvature_on_mesh_round_trips_through_vtk(ctx, tmp_path):
    from pyfocusr_amd import PolyMesh, curvature_on_mesh, principal_curvatures, read_vtk_mesh, vtk_functions, write_vtk_mesh

    pts, faces, _ = case("blob700")
    dev = device(ctx, "blob700")
    mesh = PolyMesh(pts.copy(), faces.copy())
    names = curvature_on_mesh(mesh, ctx=ctx)
    assert names == ["k_min", "k_max"]
    names += curvature_on_mesh(mesh, fields=("gaussian", "mean", "shape_index", "curvedness"), method="tensor", ctx=ctx)
    stored = dict(mesh.point_data)
    assert sorted(stored) == sorted(names)
    assert np.array_equal(stored["k_min"], dev["k_min"]) and np.array_equal(stored["k_max"], dev["k_max"])
    assert np.array_equal(stored["gaussian"], dev["gaussian"]) and np.array_equal(stored["mean"], dev["mean"])
    assert np.all(np.abs(stored["shape_index"]) <= 1.0)
    path = str(tmp_path / "curved.vtk")
    write_vtk_mesh(mesh, path)
    back = dict(read_vtk_mesh(path).point_data)
    for name in names:
        assert np.array_equal(np.asarray(back[name], dtype=np.float64), stored[name]), name
    k_min, k_max = vtk_functions.get_min_max_curvature_values(mesh, ctx=ctx)
    assert np.array_equal(k_min, dev["k_min"]) and np.array_equal(k_max, dev["k_max"])
    assert np.array_equal(vtk_functions.get_min_curvature(mesh, ctx=ctx)[0], k_min)
    assert np.array_equal(vtk_functions.get_max_curvature(mesh, ctx=ctx)[0], k_max)
    t_min, t_max = principal_curvatures(mesh, method="tensor", ctx=ctx)
    assert np.array_equal(t_min, dev["tensor_k_min"]) and np.array_equal(t_max, dev["tensor_k_max"])
