"""Sub-vertex correspondences: the closest point of a surface embedded in d dimensions (`pf_surface_nd_*`,
`pyfocusr_amd.correspondence`, `Focusr(return_surface_final_points=True)`).

CPU: the C-ABI declarations, argument errors before any device call, `interpolate_on_surface` against a loop, the numpy
reference at d = 3 against `oracle.icp_port`, and the order of `Focusr`'s calls with the device replaced.  GPU: face,
corners, weights and squared distance bit-identical to the numpy brute force for every depth on both sides of each
templated / generic instance of the kernel (templated: 3, 4, 5, 6, 8, 10), the exhaustive device mode, `pf_surface_closest`
at d = 3, known answers, degenerate input, and the properties of the surface map on the bundled 5k pair.

The kernel has one packet size (8 queries per wave) for every query count, so there is no switch to straddle."""
import os
import re

import numpy as np
import pytest

import _surface_nd_ref as ref
from oracle import icp_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
DEPTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16]  # every templated depth, its generic neighbours, and both ends


def _sphere_mesh(n):
    from scipy.spatial import ConvexHull

    from pyfocusr_amd.meshgen import fibonacci_sphere

    u = fibonacci_sphere(n)
    return u, ConvexHull(u).simplices.astype(np.int32)


def _embed(xyz, d):
    """A smooth map of 3-D positions into d dimensions whose first three coordinates are the position itself (for d >= 3):
    the sphere stays a genuine 2-manifold.  For d < 3 it is a projection: triangles overlap and many distances tie."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    f = [x, y, z, 0.7 * x * y, 0.7 * y * z, 0.7 * z * x, 0.5 * (x * x - y * y), 0.5 * z * z, 0.4 * x * y * z, 0.3 * x ** 3,
         0.3 * y ** 3, 0.3 * z ** 3, 0.25 * x * x * y, 0.25 * y * y * z, 0.25 * z * z * x, 0.2 * x ** 4]
    return np.ascontiguousarray(np.stack(f[:d], axis=1))


def _grid(n):
    """(ij (n*n, 2) integer grid positions, triangles: all (a, b, c) of the cells first, then all (a, c, d), quads)."""
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    ij = np.stack([i.ravel(), j.ravel()], axis=1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    quads = np.stack([a, b, c, d], 1).astype(np.int32)
    return ij, tris, quads


# the grid step (1, 0) goes to E1 and (0, 1) to E2: integer, orthogonal, |E|^2 = 4, so every dot product of the walk on grid
# triangles is an exact integer (or dyadic) and the Gram determinant va + vb + vc = 16 a power of two; coordinate 4 is free
E1 = np.array([1.0, 1.0, 1.0, 1.0, 0.0])
E2 = np.array([1.0, -1.0, 1.0, -1.0, 0.0])
UP = np.array([0.0, 0.0, 0.0, 0.0, 1.0])


def _grid5(n):
    ij, tris, quads = _grid(n)
    return ij[:, :1] * E1 + ij[:, 1:] * E2, tris, quads


def _same(got, want):
    """bit for bit (NaN equal to NaN, -0.0 not equal to +0.0)"""
    for key in ("face", "vertices", "bary", "d2"):
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, key
        assert g.tobytes() == w.tobytes(), "%s differs in %d entries" % (key, int(np.sum(~((g == w) | ((g != g) & (w != w))))))


# ------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, arity in (("pf_surface_nd_create", 8), ("pf_surface_nd_free", 1), ("pf_surface_nd_closest", 8)):
        m = re.search(r"(?:int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity
        assert len(_hip.SIGNATURES[name][1]) == arity


def test_argument_errors_before_any_device_call(monkeypatch):
    from pyfocusr_amd import _hip, correspondence

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceSurfaceND", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    ij, tris, _ = _grid(4)
    x = _embed(np.concatenate([ij, ij[:, :1]], axis=1), 5)
    f = correspondence.closest_points_on_embedded_surface
    for q, coords, faces in ((np.zeros((0, 5)), x, tris), (np.zeros(5), x, tris), (np.zeros((3, 4)), x, tris),
                             (x, x, tris[:0]), (x, x, tris.ravel()), (x, x, tris[:, :2]), (x, x[:0], tris),
                             (np.zeros((3, 17)), np.zeros((16, 17)), tris), (np.zeros((3, 0)), np.zeros((16, 0)), tris),
                             (x, x, tris + 100), (x, x, -tris - 1), (x, x, tris.astype(np.float64))):
        with pytest.raises(ValueError):
            f(q, coords, faces)
    with pytest.raises(ValueError):
        correspondence.interpolate_on_surface(np.zeros((4, 2, 2)), np.zeros((3, 3), dtype=int), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        correspondence.interpolate_on_surface(np.zeros(4), np.zeros((3, 2), dtype=int), np.zeros((3, 2)))


def test_interpolate_equals_explicit_loop_bit_for_bit():
    from pyfocusr_amd import PolyMesh
    from pyfocusr_amd.correspondence import interpolate_on_surface, transfer_point_data

    rng = np.random.default_rng(3)
    n, q = 40, 101
    verts = rng.integers(0, n, size=(q, 3)).astype(np.int32)
    bary = rng.random((q, 3))
    verts[[5, 77]] = -1
    bary[[5, 77]] = np.nan
    for values in (rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=(n, 1))):
        want = np.full((q,) + values.shape[1:], np.nan)
        for i in range(q):
            if verts[i, 0] < 0:
                continue
            acc = values[verts[i, 0]] * bary[i, 0]
            acc = acc + values[verts[i, 1]] * bary[i, 1]
            acc = acc + values[verts[i, 2]] * bary[i, 2]
            want[i] = acc
        got = interpolate_on_surface(values, verts, bary)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
    mesh = PolyMesh(rng.normal(size=(n, 3)), np.array([[0, 1, 2]]), [("thickness", np.arange(n, dtype=np.float64))])
    got = transfer_point_data(mesh, "thickness", verts, bary)
    assert got.tobytes() == interpolate_on_surface(np.arange(n, dtype=np.float64), verts, bary).tobytes()
    with pytest.raises(KeyError):
        transfer_point_data(mesh, "absent", verts, bary)


def test_reference_at_three_dimensions_equals_the_icp_oracle():
    from pyfocusr_amd.correspondence import interpolate_on_surface

    rng = np.random.default_rng(5)
    pts, faces = _sphere_mesh(150)
    ij, tris, _ = _grid(5)
    grid = np.concatenate([ij, np.zeros((len(ij), 1))], axis=1)
    mid = 0.5 * (grid[tris[:, 0]] + grid[tris[:, 2]])
    for x, f, q in ((pts, faces, np.concatenate([pts[::7], 1.2 * pts[::5] + 0.01, rng.uniform(-1.5, 1.5, (60, 3))])),
                    (grid, tris, np.concatenate([grid, mid, mid + [0.0, 0.0, 0.75], rng.uniform(-1, 5, (60, 3))]))):
        want_pt, want_face, want_d2 = icp_port.closest_points_on_surface(x, f, q)
        got = ref.closest_points_on_surface_nd(x, f, q)
        assert np.array_equal(got["face"], want_face)
        assert got["d2"].tobytes() == want_d2.tobytes()
        assert got["point"].tobytes() == want_pt.tobytes()
        # the weights describe that point: interpolation agrees with it to rounding, exactly at corners
        back = interpolate_on_surface(x, got["vertices"], got["bary"])
        assert np.max(np.abs(back - want_pt)) <= 8 * EPS * np.max(np.abs(x))
        corner = (got["bary"] == 1.0).any(axis=1)
        assert corner.any() and np.array_equal(back[corner], want_pt[corner])


class _Recorder(object):
    def __init__(self):
        self.calls = []


def _bare_focusr(monkeypatch, flag, smoothed=True):
    """A `Focusr` that never saw a device: the attributes `align_maps` reads, every step replaced by a recorder."""
    from pyfocusr_amd import PolyMesh, focusr

    rec = _Recorder()
    reg = focusr.Focusr.__new__(focusr.Focusr)
    pts, faces = _sphere_mesh(30)

    class _G(object):
        points = pts
        n_points = len(pts)
        vtk_mesh = PolyMesh(pts, faces)

    reg.graph_target = reg.graph_source = _G()
    reg._ctx = "ctx"
    reg.n_total_spectral_features, reg.target_eigenmap_as_reference = 6, True
    reg.include_points_as_features = False
    reg.rigid_before_non_rigid_reg = False
    reg.smooth_correspondences = smoothed
    reg.return_average_final_points = smoothed
    reg.return_nearest_final_points = reg.return_transformed_mesh = True
    reg.return_surface_final_points = flag
    reg.smoothed_target_coords = None
    reg._coords = {"source": pts[:, :2] + 1.0, "target": pts[:, :2].copy()}
    reg.corresponding_target_idx_for_each_source_pt = np.arange(len(pts))

    class _Sorter(object):
        def __init__(self, **kw):
            pass

        def sort_eigenmaps(self):
            return np.ones(6)

    monkeypatch.setattr(focusr, "eigsort", _Sorter)

    def smooth():
        rec.calls.append("get_smoothed_correspondences")
        reg.smoothed_target_coords = pts * 0.5
        reg.source_projected_on_target = pts * 0.5 + 0.25

    monkeypatch.setattr(reg, "get_smoothed_correspondences", smooth, raising=False)
    for name in ("calc_spectral_coords", "register_target_to_source", "get_initial_correspondences",
                 "get_weighted_final_node_locations", "get_nearest_neighbour_final_node_locations",
                 "get_source_mesh_transformed_weighted_avg", "get_source_mesh_transformed_nearest_neighbour"):
        monkeypatch.setattr(reg, name, (lambda n: lambda *a, **k: rec.calls.append(n))(name), raising=False)

    def search(queries, coords, faces_, ctx=None, surface=None, exhaustive=False):
        rec.calls.append("closest_points_on_embedded_surface")
        rec.search = (queries, coords, faces_, ctx)
        n = len(queries)
        return {"face": np.zeros(n, np.int32), "vertices": np.tile(faces_[0], (n, 1)).astype(np.int32),
                "bary": np.tile([0.5, 0.25, 0.25], (n, 1)), "d2": np.ones(n)}

    monkeypatch.setattr(focusr, "closest_points_on_embedded_surface", search)
    return reg, rec, pts, faces


NEW_ATTRIBUTES = ("corresponding_target_face_for_each_source_pt", "corresponding_target_vertices_for_each_source_pt",
                  "corresponding_target_bary_for_each_source_pt", "surface_correspondence_d2", "surface_transformed_points",
                  "surface_transformed_mesh")


def test_focusr_flag_off_calls_nothing_new(monkeypatch):
    reg, rec, _, _ = _bare_focusr(monkeypatch, flag=False)
    reg.align_maps()
    assert "closest_points_on_embedded_surface" not in rec.calls
    assert not any(hasattr(reg, name) for name in NEW_ATTRIBUTES)
    assert rec.calls[-4:] == ["get_weighted_final_node_locations", "get_nearest_neighbour_final_node_locations",
                              "get_source_mesh_transformed_weighted_avg", "get_source_mesh_transformed_nearest_neighbour"]


@pytest.mark.parametrize("smoothed", [True, False])
def test_focusr_flag_on_searches_the_right_surface_last(monkeypatch, smoothed):
    from pyfocusr_amd import focusr

    reg, rec, pts, faces = _bare_focusr(monkeypatch, flag=True, smoothed=smoothed)
    order = []
    for name in ("get_surface_final_node_locations", "get_surface_correspondence", "get_source_mesh_transformed_surface"):
        real = getattr(focusr.Focusr, name)
        monkeypatch.setattr(reg, name, (lambda n, fn: lambda *a, **k: (order.append(n), fn(reg, *a, **k))[1])(name, real),
                            raising=False)
    idx_before = reg.corresponding_target_idx_for_each_source_pt.copy()
    reg.align_maps()
    assert order == ["get_surface_final_node_locations", "get_surface_correspondence", "get_source_mesh_transformed_surface"]
    assert rec.calls[-1] == "closest_points_on_embedded_surface"  # after every step the flag does not govern
    queries, coords, faces_, ctx = rec.search
    if smoothed:
        assert queries is reg.source_projected_on_target and coords is reg.smoothed_target_coords
    else:
        assert queries is reg.source_spectral_coords and coords is reg.target_spectral_coords
    assert ctx == "ctx" and np.array_equal(faces_, faces)
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, idx_before)
    want = pts[faces[0, 0]] * 0.5 + pts[faces[0, 1]] * 0.25 + pts[faces[0, 2]] * 0.25
    assert np.array_equal(reg.surface_transformed_points, np.tile(want, (len(pts), 1)))
    assert np.array_equal(reg.surface_transformed_mesh.points, reg.surface_transformed_points)
    assert np.array_equal(reg.surface_correspondence_d2, np.ones(len(pts)))
    reg.get_average_shape(align_type="surface")
    assert np.array_equal(reg.average_mesh.points, (reg.surface_transformed_points + pts) / 2)


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


@pytest.fixture(scope="module")
def sphere():
    """~2 200 vertices, ~4 400 triangles: 69 chunks, two super-chunks."""
    pts, faces = _sphere_mesh(2200)
    assert len(faces) > 4096
    return pts, faces


def _sphere_queries(d, seed):
    from pyfocusr_amd.meshgen import fibonacci_sphere

    rng = np.random.default_rng(seed)
    other = fibonacci_sphere(150)[:, [2, 0, 1]] * (1.0 + 0.02 * rng.normal(size=(150, 1)))  # another sampling, perturbed
    near = _embed(other, d)                                                                # the FOCUSR case
    box = _embed(rng.uniform(-1.0, 1.0, size=(4000, 3)), d)
    far = rng.uniform(box.min(0) - 0.5, box.max(0) + 0.5, size=(149, d))                    # far from the surface
    return np.concatenate([near, far])  # 299: not a multiple of the packet


def _search(ctx, coords, faces, q, **kw):
    from pyfocusr_amd import closest_points_on_embedded_surface

    return closest_points_on_embedded_surface(q, coords, faces, ctx=ctx, **kw)


_reference_cache = {}


def _sphere_case(sphere, d):
    """(coords, faces, queries, numpy reference), computed once per depth and left unchanged"""
    if d not in _reference_cache:
        pts, faces = sphere
        coords, q = _embed(pts, d), _sphere_queries(d, 100 + d)
        _reference_cache[d] = (coords, faces, q, ref.closest_points_on_surface_nd(coords, faces, q))
    return _reference_cache[d]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DEPTHS)
def test_equals_numpy_brute_force_pruned_and_exhaustive(ctx, sphere, d):
    from pyfocusr_amd import _hip

    coords, faces, q, want = _sphere_case(sphere, d)
    with _hip.DeviceSurfaceND(coords, faces, ctx=ctx) as surface:
        pruned = _search(ctx, None, None, q, surface=surface)
        stats = surface.last_search()
        exhaustive = _search(ctx, None, None, q, surface=surface, exhaustive=True)
        assert surface.last_search()["chunks_opened"] == stats["packets"] * stats["n_chunks"]
        again = _search(ctx, None, None, q, surface=surface)
        single = _search(ctx, None, None, q[17:18], surface=surface)
    _same(pruned, want)
    _same(exhaustive, want)
    _same(again, pruned)  # two calls: identical bits
    _same(single, {k: want[k][17:18] for k in ("face", "vertices", "bary", "d2")})
    assert stats["packets"] == (len(q) + 7) // 8 and stats["n_chunks"] == (len(faces) + 63) // 64
    assert 0 < stats["chunks_opened"] <= stats["packets"] * stats["n_chunks"]
    assert np.all(want["face"] >= 0)


@pytest.mark.gpu
def test_three_dimensions_equal_the_icp_search(ctx, sphere):
    from pyfocusr_amd import _hip

    coords, faces, q, _ = _sphere_case(sphere, 3)
    got = _search(ctx, coords, faces, q)
    surf = _hip.DeviceSurface(coords, faces, ctx=ctx)
    try:
        pt, face, d2 = surf.closest(q)
    finally:
        surf.close()
    assert got["d2"].tobytes() == d2.tobytes() and np.array_equal(got["face"], face)


@pytest.mark.gpu
def test_quad_mesh_at_three_dimensions_agrees_across_every_search(ctx):
    """One hierarchy build serves `DeviceSurfaceND` and `DeviceSurface`.  2 116 quads = 4 232 fan triangles: fan position 1
    in every face, 67 chunks (the last one of 8 triangles), two super-chunks; 299 queries fill no packet of 4, 8 or 16.
    A build that strides the boxes wrongly, miscounts the last chunk or drops the fan position cannot give the brute-force
    answer here, whichever search reads it."""
    from pyfocusr_amd import _hip

    n = 47
    ij, _, quads = _grid(n)
    n_tri = 2 * len(quads)
    assert n_tri > 4096 and n_tri % 64 != 0
    rng = np.random.default_rng(47)
    x = np.ascontiguousarray(np.concatenate([ij + 0.2 * rng.uniform(-1.0, 1.0, size=ij.shape),
                                             1.5 * rng.normal(size=(len(ij), 1))], axis=1))
    w = rng.dirichlet([1.0, 1.0, 1.0, 1.0], size=150)
    near = np.einsum("qc,qck->qk", w, x[quads[rng.integers(0, len(quads), 150)]]) + 0.05 * rng.normal(size=(150, 3))
    far = rng.uniform(x.min(0) - 3.0, x.max(0) + 3.0, size=(149, 3))
    q = np.concatenate([near, far])
    assert len(q) == 299
    want = ref.closest_points_on_surface_nd(x, quads, q)
    second = want["vertices"][:, 1] != quads[want["face"], 1]  # the winner is fan triangle (0, 2, 3) of its quad
    assert np.all(want["face"] >= 0) and second.any() and not second.all()

    _same(_search(ctx, x, quads, q), want)
    surf = _hip.DeviceSurface(x, quads, ctx=ctx)
    try:
        dist_d2, dist_face, _ = surf.distance(q)
        _, near_face, near_d2 = surf.closest(q)
    finally:
        surf.close()
    assert dist_d2.tobytes() == want["d2"].tobytes() and np.array_equal(dist_face, want["face"])
    assert near_d2.tobytes() == want["d2"].tobytes() and np.array_equal(near_face, want["face"])


@pytest.mark.gpu
def test_known_answers_on_an_integer_grid(ctx):
    from pyfocusr_amd import interpolate_on_surface

    n = 9
    x, tris, quads = _grid5(n)
    n_cells = (n - 1) ** 2
    # at the vertices: distance 0, all weight on that vertex
    got = _search(ctx, x, tris, x)
    assert np.all(got["d2"] == 0.0)
    assert np.array_equal(np.sort(got["bary"], axis=1), np.tile([0.0, 0.0, 1.0], (len(x), 1)))
    assert np.array_equal(got["vertices"][np.arange(len(x)), np.argmax(got["bary"], axis=1)], np.arange(len(x)))
    # at the midpoints of all three edges of every triangle: distance 0, a half on each end
    for j, k in ((0, 1), (1, 2), (2, 0)):
        ends = tris[:, [j, k]]
        got = _search(ctx, x, tris, (x[ends[:, 0]] + x[ends[:, 1]]) / 2)
        assert np.all(got["d2"] == 0.0)
        assert np.array_equal(np.sort(got["bary"], axis=1), np.tile([0.0, 0.5, 0.5], (len(tris), 1)))
        half = np.sort(np.where(got["bary"] == 0.5, got["vertices"], -1), axis=1)[:, 1:]
        assert np.array_equal(half, np.sort(ends, axis=1))
    # interior points from dyadic weights, lifted off the surface: the weights come back exactly, d2 is the lift squared
    for w in ((0.5, 0.25, 0.25), (0.125, 0.625, 0.25), (0.25, 0.25, 0.5)):
        q = x[tris[:, 0]] * w[0] + x[tris[:, 1]] * w[1] + x[tris[:, 2]] * w[2] + 0.5 * UP
        got = _search(ctx, x, tris, q)
        assert np.array_equal(got["face"], np.arange(len(tris))) and np.array_equal(got["vertices"], tris)
        assert np.array_equal(got["bary"], np.tile(w, (len(tris), 1))) and np.all(got["d2"] == 0.25)
        assert np.array_equal(interpolate_on_surface(x, got["vertices"], got["bary"]), q - 0.5 * UP)
    # above the middle of a cell's diagonal a - c: triangles k = (a, b, c) and k + n_cells = (a, c, d) tie; the lower wins
    q = (x[tris[:n_cells, 0]] + x[tris[:n_cells, 2]]) / 2 + 2.0 * UP
    got = _search(ctx, x, tris, q)
    assert np.all(got["d2"] == 4.0) and np.array_equal(got["face"], np.arange(n_cells))
    _same(got, ref.closest_points_on_surface_nd(x, tris, q))
    # quads: face t // 2, and the corners of the fan triangle itself
    inside_second = x[quads[:, 0]] * 0.25 + x[quads[:, 2]] * 0.25 + x[quads[:, 3]] * 0.5 - 1.0 * UP
    got = _search(ctx, x, quads, inside_second)
    assert np.array_equal(got["face"], np.arange(n_cells)) and np.array_equal(got["vertices"], quads[:, [0, 2, 3]])
    assert np.array_equal(got["bary"], np.tile([0.25, 0.25, 0.5], (n_cells, 1))) and np.all(got["d2"] == 1.0)
    _same(got, ref.closest_points_on_surface_nd(x, quads, inside_second))


@pytest.mark.gpu
def test_non_finite_queries_and_degenerate_triangles(ctx):
    """What "never wins" means is the header's rule: a triangle whose distance is NaN.  A repeated-vertex triangle
    (a, a, b) gives NaN (0 / 0 in the edge region) for every query that projects strictly inside a - b, and a finite
    distance only in its corner regions, like the 3-D search; triangles with a NaN vertex give NaN always."""
    x, tris, _ = _grid5(7)
    rng = np.random.default_rng(9)
    q = x[rng.integers(0, len(x), 90)] + rng.normal(size=(90, 5)) * 0.3
    # long repeated-vertex triangles across the whole grid, first in the list so that a wrongly finite tie would win,
    # and triangles on two NaN vertices
    far_a, far_b = len(x), len(x) + 1
    xs = np.concatenate([x, [-50.0 * E1 - 7.0 * UP], [50.0 * E1 - 7.0 * UP], [[np.nan] * 5], [[0.0, np.nan, 0.0, 0.0, 0.0]]])
    bad = np.array([[far_a, far_a, far_b], [far_a, far_b, far_b + 1], [far_b + 1, far_b + 2, 0], [far_a, far_a, far_b]],
                   dtype=np.int32)
    mixed = np.concatenate([bad, tris]).astype(np.int32)
    got = _search(ctx, xs, mixed, q)
    _same(got, ref.closest_points_on_surface_nd(xs, mixed, q))
    assert np.all(got["face"] >= len(bad)) and np.all(np.isfinite(got["d2"]))
    _same({k: v for k, v in got.items()}, dict(_search(ctx, xs, mixed, q, exhaustive=True)))
    # only such triangles: the sentinel for every query
    got = _search(ctx, xs, bad, q)
    assert np.all(got["face"] == -1) and np.all(got["vertices"] == -1)
    assert np.all(np.isnan(got["bary"])) and np.all(np.isnan(got["d2"]))
    _same(got, ref.closest_points_on_surface_nd(xs, bad, q))
    # non-finite queries between finite ones
    q2 = q.copy()
    q2[3, 2], q2[40, 0], q2[41, 4], q2[89, 1] = np.nan, np.inf, -np.inf, np.nan
    got = _search(ctx, x, tris, q2)
    rows = [3, 40, 41, 89]
    assert np.all(got["face"][rows] == -1) and np.all(got["vertices"][rows] == -1)
    assert np.all(np.isnan(got["bary"][rows])) and np.all(np.isnan(got["d2"][rows]))
    _same(got, ref.closest_points_on_surface_nd(x, tris, q2))
    _same(_search(ctx, x, tris, q2[40:41]), ref.closest_points_on_surface_nd(x, tris, q2[40:41]))


def _focusr(golden, ctx, flag, smooth):
    from pyfocusr_amd import Focusr, PolyMesh

    gt, gs = golden("target_mesh"), golden("source_mesh")
    kw = dict(graph_smoothing_iterations=30, projection_smooth_iterations=10) if smooth else dict(
        return_average_final_points=False, smooth_correspondences=False)
    reg = Focusr(PolyMesh(gt["points"], gt["faces"]), PolyMesh(gs["points"], gs["faces"]), icp_register_first=False,
                 n_spectral_features=3 if smooth else 5, n_extra_spectral=3 if smooth else 1,
                 n_coords_spectral_ordering=10000, list_features_to_calc=[],
                 ctx=ctx, registration=lambda src, tgt, kind: tgt, return_surface_final_points=flag, **kw)
    reg.align_maps()
    return reg


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [True, False])
def test_surface_map_of_the_5k_pair(golden, ctx, smooth):
    from pyfocusr_amd import point_to_surface_distances

    reg, off = _focusr(golden, ctx, True, smooth), _focusr(golden, ctx, False, smooth)
    # the flag changes nothing that existed before
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, off.corresponding_target_idx_for_each_source_pt)
    assert reg.nearest_neighbor_transformed_points.tobytes() == off.nearest_neighbor_transformed_points.tobytes()
    if smooth:
        assert reg.weighted_avg_transformed_points.tobytes() == off.weighted_avg_transformed_points.tobytes()
    assert not any(hasattr(off, name) for name in NEW_ATTRIBUTES)

    if smooth:
        tgt, src = reg.smoothed_target_coords, reg.source_projected_on_target
    else:
        tgt, src = reg.target_spectral_coords, reg.source_spectral_coords
    d = tgt.shape[1]
    assert d == (3 if smooth else 5)  # the smoothed physical surface / five weighted spectral coordinates
    idx = reg.corresponding_target_idx_for_each_source_pt
    diff = src - tgt[idx]
    d2_vertex = np.sum(diff * diff, axis=1)
    d2 = reg.surface_correspondence_d2
    # The surface contains its vertices, so in exact arithmetic d2 <= d2_vertex.  In floating point the computed closest
    # point is within delta = 16 sqrt(d) eps M of the exact one (M the largest coordinate magnitude: a handful of
    # roundings of size eps M per coordinate in the differences, the weights and the point), so the computed
    # d2 <= (sqrt(d2_exact) + delta)^2 <= d2_vertex + 2 sqrt(d2_vertex) delta + delta^2, and both sums of d squares carry
    # a relative 4 d eps on top.
    M = max(np.max(np.abs(tgt)), np.max(np.abs(src)))
    delta = 16.0 * np.sqrt(d) * EPS * M
    margin = 2.0 * np.sqrt(d2_vertex) * delta + delta * delta + 4.0 * d * EPS * d2_vertex
    print("d =", d, "max d2 - d2_vertex:", np.max(d2 - d2_vertex), "largest margin:", margin.max(),
          "strictly closer:", int(np.sum(d2 < d2_vertex)), "of", len(d2))
    assert np.all(np.isfinite(d2)) and np.all(reg.corresponding_target_face_for_each_source_pt >= 0)
    assert np.all(d2 <= d2_vertex + margin)

    # the images lie on the target surface: they are convex combinations of a target triangle's corners, rounded (3 products
    # and 2 sums per coordinate, < 4 eps M3 each with M3 the largest target coordinate), and the distance search rounds
    # its differences and its closest point the same way: 32 eps M3 covers both
    gt = golden("target_mesh")
    M3 = np.max(np.abs(gt["points"]))
    dist, _ = point_to_surface_distances(reg.surface_transformed_points, (gt["points"], gt["faces"]), ctx=ctx)
    print("largest distance of an image to the target surface:", dist.max(), "allowance:", 32.0 * EPS * M3)
    assert np.all(dist <= 32.0 * EPS * M3)
    assert np.array_equal(reg.surface_transformed_mesh.points, reg.surface_transformed_points)

    images = np.concatenate([reg.corresponding_target_face_for_each_source_pt[:, None].astype(np.float64),
                             reg.corresponding_target_bary_for_each_source_pt], axis=1)
    n_images = len(np.unique(images, axis=0))
    n_vertices = len(np.unique(idx))
    print("distinct (face, bary) images:", n_images, "unique vertex correspondences:", n_vertices, "of", len(idx))
    assert n_images >= n_vertices
