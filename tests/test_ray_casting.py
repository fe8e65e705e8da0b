"""Ray casting (`pf_surface_raycast`, `pf_surface_vertex_normals`, `pyfocusr_amd.ray_casting`).

CPU: the C-ABI declarations, the numpy reference (`_ray_ref.cast`: the exact test over all fan triangles, no pruning)
against closed forms, argument errors before any device call.  GPU: bit-for-bit parity of t, face, uv and count with the
reference on closed, open, defective, degenerate and quad meshes for five ray sets; invalid rays, misses, repeatability,
partial packets and permutations; inclusive interval ends; facing; crossing parity against the winding numbers;
thickness along normals; one run at 250k.

blob_mesh(3000) has 5996 triangles = 94 chunks (the last one partial) in 2 super-chunks: the smallest size that takes
both levels of the hierarchy.  What the reference alone gives on it (checked on the host) is asserted next to each use."""
import os
import re

import numpy as np
import pytest

import _ray_ref as rr
import _signed_ref as ref
import _winding_ref as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBLIQUE = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
# the six axis directions, zero components of both signs
AXES = np.array([[1.0, 0.0, -0.0], [-1.0, -0.0, 0.0], [-0.0, 1.0, 0.0], [0.0, -1.0, -0.0], [0.0, -0.0, 1.0], [-0.0, 0.0, -1.0]])


def _same(got, want):
    """t, face, uv (and count) equal bit for bit, NaNs matching."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name,n_args", [("pf_surface_raycast", 11), ("pf_surface_vertex_normals", 2)])
def test_ray_entry_points_are_declared_and_bound(name, n_args):
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, "%s is not declared in the header" % name
    assert len(m.group(1).split(",")) == n_args
    _, argtypes = _hip.SIGNATURES[name]
    assert len(argtypes) == n_args


def test_reference_against_closed_forms():
    pts = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    o = np.array([[0.25, -0.5, 1.0]])
    down, up = np.array([[0.0, 0.0, -2.0]]), np.array([[0.0, 0.0, 2.0]])
    for faces in (np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), np.array([[0, 1, 2, 3]], dtype=np.int32)):  # normals +z
        t, face, uv, count = rr.cast(pts, faces, o, down)
        assert t[0] == 0.5 and face[0] == 0 and count[0] == 1  # the point lies in fan triangle (0, 1, 2) of either mesh
        a, b, c = pts[0], pts[1], pts[2]
        assert np.array_equal(a + uv[0, 0] * (b - a) + uv[0, 1] * (c - a), [0.25, -0.5, 0.0])
        t, face, uv, count = rr.cast(pts, faces, o, up)
        assert t[0] == np.inf and face[0] == -1 and np.all(np.isnan(uv)) and count[0] == 0
        assert rr.cast(pts, faces, o, down, facing=1)[0][0] == 0.5  # from above: the side the normals point to
        assert rr.cast(pts, faces, o, down, facing=-1)[0][0] == np.inf
        assert rr.cast(pts, faces, -o, up, facing=-1)[0][0] == 0.5 and rr.cast(pts, faces, -o, up, facing=1)[0][0] == np.inf
        assert rr.cast(pts, faces, o, down, t_max=0.25)[3][0] == 0 and rr.cast(pts, faces, o, down, t_min=0.5, t_max=0.5)[3][0] == 1
    cp, cq = ref.cube_quads()
    t, face, uv, count = rr.cast(cp, cq, np.zeros((1, 3)), np.array([[0.3, 0.5, 0.8]]))
    assert count[0] == 1 and t[0] == 1.25 and face[0] == 5  # leaves through z = 1
    bad = rr.cast(cp, cq, np.array([[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]),
                  np.array([[1.0, 0.0, 0.0], [0.0, -0.0, 0.0], [0.0, np.inf, 0.0]]))
    assert np.all(np.isnan(bad[0])) and np.all(bad[1] == -1) and np.all(np.isnan(bad[2])) and np.all(bad[3] == 0)


def test_hit_points_on_the_host():
    from pyfocusr_amd import hit_points

    o = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 2.0, 3.0]])
    d = np.array([[0.0, 0.0, -2.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = hit_points(o, d, np.array([0.5, np.inf, np.nan]))
    assert np.array_equal(p[0], [0.0, 0.0, 0.0]) and np.all(np.isnan(p[1:]))
    with pytest.raises(ValueError):
        hit_points(o, d, np.zeros(2))


def test_ray_argument_errors_before_any_device_call(monkeypatch):
    from pyfocusr_amd import _hip, ray_casting

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceSurface", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    pts, faces = ref.cube_triangles()
    mesh = (pts, faces)
    empty = np.zeros((0, 3), dtype=np.int32)
    o, d = np.zeros((5, 3)), np.ones((5, 3))
    bad_rays = [(np.zeros((0, 3)), np.zeros((0, 3))), (np.zeros((5, 2)), np.ones((5, 2))), (np.zeros(3), np.ones(3)),
                (o, np.ones((4, 3))), (o, np.ones((5, 2)))]
    for oo, dd in bad_rays:
        with pytest.raises(ValueError):
            ray_casting.ray_mesh_intersections(oo, dd, mesh)
        with pytest.raises(ValueError):
            ray_casting.ray_crossings(oo, dd, mesh)
    for call in (ray_casting.ray_mesh_intersections, ray_casting.ray_crossings):
        for kw in ({"t_min": 2.0, "t_max": 1.0}, {"t_min": np.nan}, {"t_max": np.nan}):
            with pytest.raises(ValueError):
                call(o, d, mesh, **kw)
        with pytest.raises(ValueError):
            call(o, d, (pts, empty))
        with pytest.raises(ValueError):
            call(o, d, (np.zeros((0, 3)), faces))
    with pytest.raises(ValueError):
        ray_casting.ray_mesh_intersections(o, d, mesh, facing="sideways")
    with pytest.raises(ValueError):
        ray_casting.ray_mesh_intersections(o, d, mesh, facing=1)
    with pytest.raises(ValueError):
        ray_casting.vertex_normals((pts, empty))
    for kw in ({"direction": "up"}, {"facing": "nope"}, {"t_max": np.nan}, {"t_max": -1.0}, {"other": (pts, empty)},
               {"other": (np.zeros((4, 2)), faces)}):
        with pytest.raises(ValueError):
            ray_casting.thickness_along_normals(mesh, **kw)
    with pytest.raises(ValueError):
        ray_casting.thickness_along_normals((pts, empty))


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


def _mesh(name):
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    if name == "cube":
        return ref.cube_quads()
    if name == "messy":
        m = messy_blob_mesh(3000)
        return m.points, m.faces
    m = blob_mesh(3000)
    faces = {"closed": lambda: m.faces, "open": lambda: wr.open_mesh(m.points, m.faces),
             "degenerate": lambda: wr.with_degenerate_faces(m.points, m.faces)}[name]()
    return m.points, faces


@pytest.fixture(scope="module")
def case():
    """name -> (points, faces, origins of set (a), reference of set (a)), computed once per name."""
    cache = {}

    def get(name):
        if name not in cache:
            pts, faces = _mesh(name)
            o = wr.query_set(pts, 4000, vertex_step=3)
            cache[name] = (pts, faces, o, rr.cast(pts, faces, o, np.tile(OBLIQUE, (len(o), 1))))
        return cache[name]

    return get


@pytest.fixture(scope="module")
def axis_case(case):
    """(name, axis) -> reference of set (b): the origins of set (a) along AXES[axis], computed once."""
    cache = {}

    def get(name, axis):
        if (name, axis) not in cache:
            pts, faces, o, _ = case(name)
            cache[name, axis] = rr.cast(pts, faces, o, np.tile(AXES[axis], (len(o), 1)))
        return cache[name, axis]

    return get


@pytest.fixture(scope="module")
def surfaces(ctx):
    """name -> an open DeviceSurface of that mesh, built once, closed at the end of the module."""
    from pyfocusr_amd import _hip

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _hip.DeviceSurface(*_mesh(name), ctx=ctx)
        return cache[name]

    yield get
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def inward(surfaces):
    """(points, faces, inward unit normals of the closed blob, bounding-box diagonal)."""
    from pyfocusr_amd import vertex_normals

    pts, faces = _mesh("closed")
    n = vertex_normals(surfaces("closed"))
    assert n.shape == pts.shape and np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-15)
    assert np.mean(np.einsum("ij,ij->i", n, pts - pts.mean(axis=0)) > 0) > 0.99  # outward, as the faces are
    return pts, faces, -n, wr.diagonal(pts)


MESHES = ["closed", "open", "messy", "cube", "degenerate"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_set_a_oblique_direction(surfaces, case, name):
    pts, faces, o, want = case(name)
    d = np.tile(OBLIQUE, (len(o), 1))
    got = surfaces(name).raycast(o, d, count=True)
    print("%s: %d rays, %d hit, counts %s" % (name, len(o), np.isfinite(want[0]).sum(), np.bincount(want[3])))
    assert np.isfinite(want[0]).sum() > 0 and np.isinf(want[0]).sum() > 0
    _same(got, want)
    _same(surfaces(name).raycast(o, d), want[:3])  # the mode that narrows the interval to the best t


@pytest.mark.gpu
@pytest.mark.parametrize("axis", range(6))
@pytest.mark.parametrize("name", ["closed", "cube"])
def test_set_b_axis_directions(surfaces, case, axis_case, name, axis):
    pts, faces, o, _ = case(name)
    d = np.tile(AXES[axis], (len(o), 1))
    want = axis_case(name, axis)
    assert np.isfinite(want[0]).sum() > 0
    _same(surfaces(name).raycast(o, d, count=True), want)
    _same(surfaces(name).raycast(o, d), want[:3])


@pytest.mark.gpu
def test_set_c_one_origin_aimed_at_every_vertex(surfaces):
    pts, faces = _mesh("closed")
    o = np.tile(pts.mean(axis=0) + np.array([3.0, 2.0, 1.0]) * wr.diagonal(pts), (len(pts), 1))
    d = pts - o  # not normalised: t = 1 at the vertex
    want = rr.cast(pts, faces, o, d)
    t, face, uv, count = want
    on_edge = (uv[:, 0] == 0.0) | (uv[:, 1] == 0.0) | (uv[:, 0] + uv[:, 1] == 1.0)
    print("set c: %d first hits on an edge or a vertex, %d misses, counts %s" % (on_edge.sum(), np.isinf(t).sum(), np.bincount(count)))
    # every ray passes through a vertex of a closed surface, so geometry says hit; the exact test loses 27 of them, and
    # 839 of the first hits lie exactly on an edge or a vertex of the winning triangle: what a too-tight box test breaks
    assert np.isinf(t).sum() == 27 and on_edge.sum() == 839
    _same(surfaces("closed").raycast(o, d, count=True), want)
    _same(surfaces("closed").raycast(o, d), want[:3])


@pytest.mark.gpu
def test_sets_d_and_e_inward_normals(surfaces, inward):
    pts, faces, d, diag = inward
    want = rr.cast(pts, faces, pts, d)
    print("set d: counts %s, max |t| %.3e" % (np.bincount(want[3]), np.max(np.abs(want[0]))))
    assert want[3].min() == 3 and want[3].max() == 8 and np.max(np.abs(want[0])) < 1e-9 * diag  # the vertex's own triangles
    _same(surfaces("closed").raycast(pts, d, count=True), want)
    _same(surfaces("closed").raycast(pts, d), want[:3])
    t_min = 1e-9 * diag
    want = rr.cast(pts, faces, pts, d, t_min=t_min)
    print("set e: counts %s, least t %.4f" % (np.bincount(want[3]), want[0].min()))
    assert np.all(want[3] == 1) and abs(want[0].min() - 22.567) < 5e-4
    _same(surfaces("closed").raycast(pts, d, t_min=t_min, count=True), want)
    _same(surfaces("closed").raycast(pts, d, t_min=t_min), want[:3])


@pytest.mark.gpu
def test_invalid_rays_misses_bits_and_null_outputs(surfaces, case):
    import ctypes as C

    from pyfocusr_amd import _hip

    pts, faces, o, want = case("closed")
    o = o[:1000].copy()
    d = np.tile(OBLIQUE, (len(o), 1))
    bad = np.array([3, 4, 200, 500, 777, 900])
    o[3, 0] = np.nan
    o[4, 2] = np.inf
    o[200] = [-np.inf, 1.0, np.nan]
    d[500] = [0.0, -0.0, 0.0]
    d[777, 1] = np.nan
    d[900, 0] = -np.inf
    surf = surfaces("closed")
    t, face, uv, count = surf.raycast(o, d, count=True)
    assert np.all(np.isnan(t[bad])) and np.all(face[bad] == -1) and np.all(np.isnan(uv[bad])) and np.all(count[bad] == 0)
    others = np.setdiff1d(np.arange(len(o)), bad)
    for g, w in zip((t, face, uv, count), want):  # a ray's result does not depend on which rays share its packet
        assert np.array_equal(g[others], w[:1000][others], equal_nan=True)
    miss = others[np.isinf(t[others])]
    assert len(miss) > 0 and np.all(face[miss] == -1) and np.all(np.isnan(uv[miss])) and np.all(count[miss] == 0)
    assert np.all(t[miss] == np.inf)
    _same(surf.raycast(o, d, count=True), (t, face, uv, count))  # two calls: identical bits
    _same(rr.cast(pts, faces, o, d), (t, face, uv, count))
    # each output alone
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    args = (surf._h, o.ctypes.data_as(f64p), d.ctypes.data_as(f64p), len(o), C.c_double(0.0), C.c_double(np.inf), 0)
    only_t, only_uv = np.full(len(o), -7.0), np.full((len(o), 2), -7.0)
    only_face, only_count = np.full(len(o), -7, dtype=np.int32), np.full(len(o), -7, dtype=np.int32)
    _hip._check(surf._lib.pf_surface_raycast(*args, only_t.ctypes.data_as(f64p), None, None, None))
    _hip._check(surf._lib.pf_surface_raycast(*args, None, only_face.ctypes.data_as(i32p), None, None))
    _hip._check(surf._lib.pf_surface_raycast(*args, None, None, only_uv.ctypes.data_as(f64p), None))
    _hip._check(surf._lib.pf_surface_raycast(*args, None, None, None, only_count.ctypes.data_as(i32p)))
    _same((only_t, only_face, only_uv, only_count), (t, face, uv, count))
    for n, lo, hi, facing in ((0, 0.0, 1.0, 0), (5, 2.0, 1.0, 0), (5, np.nan, 1.0, 0), (5, 0.0, np.nan, 0), (5, 0.0, 1.0, 2),
                              (5, 0.0, 1.0, -2)):
        with pytest.raises(_hip.PfError) as err:
            _hip._check(surf._lib.pf_surface_raycast(surf._h, o.ctypes.data_as(f64p), d.ctypes.data_as(f64p), n, C.c_double(lo),
                                                     C.c_double(hi), facing, None, None, None, None))
        assert err.value.code == -1


@pytest.mark.gpu
def test_partial_packets_and_permutations(surfaces, case):
    pts, faces, o, want = case("closed")
    d = np.tile(OBLIQUE, (len(o), 1))
    surf = surfaces("closed")
    start = int(np.flatnonzero(np.isfinite(want[0]))[0])
    for n in (1, 3, 65):
        sel = np.arange(start, start + n)
        _same(surf.raycast(o[sel], d[sel], count=True), tuple(w[sel] for w in want))
    perm = np.random.default_rng(3).permutation(len(o))
    _same(surf.raycast(o[perm], d[perm], count=True), tuple(w[perm] for w in want))
    # other directions in the same packets: each ray's own result again
    mixed = d.copy()
    mixed[::2] = AXES[np.arange(len(mixed[::2])) % 6]
    _same(surf.raycast(o, mixed, count=True), rr.cast(pts, faces, o, mixed))


@pytest.mark.gpu
def test_sixteen_ray_packets(surfaces, case, axis_case):
    """From 65536 rays on a wave takes 16 rays instead of 4: sets (a) and (b) twice over, 84000 rays, so that the rays
    of a packet share origins and differ in direction."""
    pts, faces, o, oblique = case("closed")
    wants = [oblique] + [axis_case("closed", axis) for axis in range(6)]
    dirs = [OBLIQUE] + list(AXES)
    origins = np.concatenate([o] * 14)
    d = np.concatenate([np.tile(x, (len(o), 1)) for x in dirs] * 2)
    want = tuple(np.concatenate([w[k] for w in wants] * 2) for k in range(4))
    assert len(origins) >= 16 * 4096
    _same(surfaces("closed").raycast(origins, d, count=True), want)
    _same(surfaces("closed").raycast(origins, d), want[:3])


@pytest.mark.gpu
def test_vertex_normals_before_prepare_and_raw_values(ctx):
    from pyfocusr_amd import _hip, vertex_normals

    pts, quads = ref.cube_quads()
    pts = np.concatenate([pts, [[5.0, 5.0, 5.0]]])  # a vertex no face references
    surf = _hip.DeviceSurface(pts, quads, ctx=ctx)
    try:
        out = np.empty((len(pts), 3))
        with pytest.raises(_hip.PfError) as err:
            _hip._check(surf._lib.pf_surface_vertex_normals(surf._h, _hip._f64(out)))
        assert err.value.code == -1
        raw = surf.vertex_normals()
        assert np.all(raw[8] == 0.0)
        unit = vertex_normals(surf)
        assert np.all(np.isnan(unit[8]))
        np.testing.assert_allclose(unit[:8], pts[:8] / np.sqrt(3.0), rtol=0, atol=1e-15)  # the corners' diagonals
        np.testing.assert_allclose(np.linalg.norm(raw[:8], axis=1), np.sqrt(3.0) * np.pi / 2, rtol=1e-14)  # three right angles
        t, face, uv = surf.raycast(pts, -unit)  # a NaN direction gives NaN
        assert np.isnan(t[8]) and face[8] == -1
    finally:
        surf.close()


@pytest.mark.gpu
def test_interval_ends_are_inclusive(surfaces, case):
    pts, faces, o, want = case("closed")
    d = np.tile(OBLIQUE, (len(o), 1))
    surf = surfaces("closed")
    hits = np.flatnonzero(want[3] >= 2)[:3]  # rays from outside: a first and a second hit
    assert len(hits) == 3
    for r in hits:
        oo, dd, t = o[r:r + 1], d[r:r + 1], want[0][r]
        inclusive = surf.raycast(oo, dd, t_max=t, count=True)
        assert inclusive[0][0] == t and inclusive[3][0] == 1
        _same(inclusive, rr.cast(pts, faces, oo, dd, t_max=t))
        below = np.nextafter(t, 0.0)
        _same(surf.raycast(oo, dd, t_max=below, count=True), rr.cast(pts, faces, oo, dd, t_max=below))
        assert surf.raycast(oo, dd, t_max=below)[0][0] == np.inf
        inclusive = surf.raycast(oo, dd, t_min=t, count=True)
        assert inclusive[0][0] == t and inclusive[3][0] == want[3][r]
        _same(inclusive, rr.cast(pts, faces, oo, dd, t_min=t))
        above = np.nextafter(t, np.inf)
        second = surf.raycast(oo, dd, t_min=above, count=True)
        _same(second, rr.cast(pts, faces, oo, dd, t_min=above))
        assert second[0][0] > t and second[3][0] == want[3][r] - 1
        _same(surf.raycast(oo, dd, t_min=t, t_max=t, count=True), rr.cast(pts, faces, oo, dd, t_min=t, t_max=t))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["closed", "messy"])
def test_facing(ctx, surfaces, case, name):
    from pyfocusr_amd import ray_mesh_intersections

    pts, faces, o, any_side = case(name)
    d = np.tile(OBLIQUE, (len(o), 1))
    front = rr.cast(pts, faces, o, d, facing=1)
    back = rr.cast(pts, faces, o, d, facing=-1)
    _same(surfaces(name).raycast(o, d, facing=1, count=True), front)
    _same(surfaces(name).raycast(o, d, facing=-1, count=True), back)
    assert np.array_equal(front[3] + back[3], any_side[3])
    _same(ray_mesh_intersections(o, d, (pts, faces), facing="front", ctx=ctx), front[:3])
    _same(ray_mesh_intersections(o, d, surfaces(name), facing="back"), back[:3])
    if name == "closed":  # from outside, a ray that meets the closed surface at all meets a front face
        outside = ref.winding_number(pts, faces, o) < 0.5
        assert outside.sum() > 1000
        assert np.array_equal(np.isfinite(front[0][outside]), np.isfinite(any_side[0][outside]))
        assert np.isfinite(any_side[0][outside]).sum() > 0


@pytest.mark.gpu
def test_crossing_parity_against_winding_numbers(ctx, surfaces, case):
    from pyfocusr_amd import points_inside, ray_crossings

    pts, faces, o, want = case("closed")
    inside = points_inside(o, (pts, faces), ctx=ctx)
    assert inside.sum() == 1955  # the reference's winding numbers say the same (checked on the host)
    for d, w in ((OBLIQUE, want), (np.array([0.0, 0.0, 1.0]), None)):
        d = np.tile(d, (len(o), 1))
        if w is None:
            w = rr.cast(pts, faces, o, d)
        assert np.array_equal(w[3] % 2 == 1, inside)  # the reference: no disagreement, no ray through an edge
        count = ray_crossings(o, d, surfaces("closed"))
        assert count.dtype == np.int32 and np.array_equal(count, w[3])
        assert np.array_equal(ray_crossings(o, d, (pts, faces), ctx=ctx) % 2 == 1, inside)


@pytest.mark.gpu
def test_thickness_along_normals(ctx, surfaces, inward):
    from pyfocusr_amd import PolyMesh, thickness_along_normals, vertex_normals

    pts, faces, inward_normals, diag = inward
    inner = PolyMesh(pts.mean(axis=0) + 0.9 * (pts - pts.mean(axis=0)), faces)
    n = vertex_normals(inner, ctx=ctx)
    want = rr.cast(pts, faces, inner.points, n)
    print("thickness: counts %s, t from %.4f to %.4f, diagonal %.2f" % (np.bincount(want[3]), want[0].min(), want[0].max(), diag))
    assert np.all(want[3] == 1) and abs(want[0].min() - 1.6247) < 5e-5 and abs(want[0].max() - 4.9373) < 5e-5
    got = thickness_along_normals(inner, (pts, faces), ctx=ctx)
    assert np.array_equal(got, want[0])
    assert np.array_equal(thickness_along_normals(inner, surfaces("closed"), name="gap"), want[0])
    assert np.array_equal(dict(inner.point_data)["gap"], want[0])
    assert np.all(thickness_along_normals(inner, (pts, faces), t_max=1.0, ctx=ctx) == np.inf)
    # the blob's own thickness: set (e)
    own = thickness_along_normals((pts, faces), direction="inward", ctx=ctx)
    assert np.array_equal(own, rr.cast(pts, faces, pts, inward_normals, t_min=1e-9 * diag)[0])
    assert np.array_equal(thickness_along_normals(surfaces("closed"), direction="inward"), own)


@pytest.mark.gpu
def test_250k_thickness_bounded_below_by_the_distance(ctx):
    from pyfocusr_amd import _hip, vertex_normals
    from pyfocusr_amd.meshgen import blob_mesh

    outer = blob_mesh(250000)
    centre = outer.points.mean(axis=0)
    inner = centre + 0.9 * (outer.points - centre)
    surf = _hip.DeviceSurface(outer.points, outer.faces, ctx=ctx)
    own = _hip.DeviceSurface(inner, outer.faces, ctx=ctx)
    try:
        n = vertex_normals(own)
        t, face, uv, count = surf.raycast(inner, n, count=True)
        first = surf.raycast(inner, n)
        d = np.sqrt(surf.distance(inner)[0])
    finally:
        surf.close()
        own.close()
    print("250k: t from %.4f to %.4f, min (t - d) = %.3e" % (t.min(), t.max(), np.min(t - d)))
    assert np.all(np.isfinite(t)) and np.all(face >= 0)
    assert np.all(count == 1)
    assert np.all(t >= d * (1.0 - 1e-12))  # a hit point is a surface point (unit directions: t is a distance)
    _same(first, (t, face, uv))
