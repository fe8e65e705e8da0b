"""Generalized winding numbers (`pf_surface_prepare_winding`, `pf_surface_winding`, `winding_numbers`, `points_inside`
and `sign="winding"` of `pyfocusr_amd.surface_distance`).

CPU: the C-ABI declarations, the numpy reference (`_signed_ref.winding_number`) against closed forms, argument errors
before any device call.  GPU: exact mode against the reference on closed, open, defective, quad and degenerate meshes;
non-finite queries and reproducibility; the hierarchical mode against its own bound; the signs of `sign="winding"`; the
inside test; one 250k consistency run against the pseudonormal signs.

The reference on the inputs of the exact-mode test (10 000 queries each, 4016 for the cube; checked on the host with the
reference alone): closed blob, cube and blob with degenerate faces: every w within 4e-15 of 0 or 1; open blob: w from
-0.2495 to 0.8534; messy blob: -0.0852 to 1.1706.  The query nearest to any of the surfaces is 1.0e-5 diagonals away, so
the 1e-9 diagonal filter leaves none out."""
import os
import re

import numpy as np
import pytest

import _signed_ref as ref
import _winding_ref as wr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10  # absolute, on w: <= 6100 terms of at most 2 pi, each with a few eps, summed in another order: ~4e-12


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name,n_args", [("pf_surface_prepare_winding", 1), ("pf_surface_winding", 6)])
def test_winding_entry_points_are_declared_and_bound(name, n_args):
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, "%s is not declared in the header" % name
    assert len(m.group(1).split(",")) == n_args
    _, argtypes = _hip.SIGNATURES[name]
    assert len(argtypes) == n_args


def test_reference_against_closed_forms():
    a, h = 1.0, 0.7
    pts = np.array([[-a, -a, 0.0], [a, -a, 0.0], [a, a, 0.0], [-a, a, 0.0]])
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)  # normals +z
    omega = 4.0 * np.arctan(a * a / (h * np.sqrt(2.0 * a * a + h * h)))
    np.testing.assert_allclose(omega, 2.94298705, rtol=1e-8)
    w = ref.winding_number(pts, faces, np.array([[0.0, 0.0, h], [0.0, 0.0, -h]]))
    np.testing.assert_allclose(4.0 * np.pi * w, [-omega, omega], rtol=1e-13)  # minus on the side the normals point to
    quad = ref.winding_number(pts, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([[0.0, 0.0, -h]]))
    np.testing.assert_allclose(4.0 * np.pi * quad, [omega], rtol=1e-13)
    cp, cf = ref.cube_triangles()
    w = ref.winding_number(cp, cf, np.array([[0.0, 0.0, 0.0], [3.0, 0.2, 0.1]]))
    np.testing.assert_allclose(w[0], 1.0, rtol=1e-13)
    assert abs(w[1]) <= 1e-13


def test_winding_argument_errors_before_any_device_call(monkeypatch):
    from pyfocusr_amd import _hip, surface_distance

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceSurface", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    pts, faces = ref.cube_triangles()
    empty = np.zeros((0, 3), dtype=np.int32)
    for q, mesh in [(np.zeros((0, 3)), (pts, faces)), (np.zeros((5, 2)), (pts, faces)), (np.zeros(3), (pts, faces)),
                    (pts, (pts, empty))]:
        with pytest.raises(ValueError):
            surface_distance.winding_numbers(q, mesh)
        with pytest.raises(ValueError):
            surface_distance.points_inside(q, mesh)
        with pytest.raises(ValueError):
            surface_distance.signed_point_to_surface_distances(q, mesh, sign="winding")
    with pytest.raises(ValueError):
        surface_distance.winding_numbers(pts, (pts, faces), beta=0.5)
    with pytest.raises(ValueError):
        surface_distance.signed_point_to_surface_distances(pts, (pts, faces), sign="nope")
    with pytest.raises(ValueError):
        surface_distance.signed_distances_on_mesh((pts, faces), (pts, faces), sign="nope")
    with pytest.raises(ValueError):
        surface_distance.surface_distance_metrics((pts, faces), (pts, faces), signed=True, sign="nope")
    with pytest.raises(ValueError):
        surface_distance.surface_distance_metrics((pts, faces), (pts, empty), signed=True, sign="winding")


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
    """name -> (points, faces, queries, reference w, keep = not within 1e-9 diagonals of the surface by the reference's
    distance), computed once per name."""
    cache = {}

    def get(name):
        if name not in cache:
            pts, faces = _mesh(name)
            q = wr.query_set(pts)
            tol = 1e-9 * wr.diagonal(pts)
            keep = wr.unsigned_distance(pts, faces, q, far=tol) >= tol
            cache[name] = (pts, faces, q, ref.winding_number(pts, faces, q), keep)
        return cache[name]

    return get


def _winding(ctx, pts, faces, q, beta=0.0):
    from pyfocusr_amd import _hip

    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        return surf.winding_number(q, beta=beta)
    finally:
        surf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["closed", "open", "messy", "cube", "degenerate"])
def test_exact_mode_against_reference(ctx, case, name):
    pts, faces, q, want, keep = case(name)
    assert np.mean(~keep) < 0.01
    w, bound = _winding(ctx, pts, faces, q)
    err = np.abs(w - want)[keep]
    print("%s: %d queries, %d left out, max |w - w_ref| = %.3e" % (name, len(q), int(np.sum(~keep)), err.max()))
    assert np.all(bound == 0.0)
    assert err.max() <= TOL


@pytest.mark.gpu
def test_nonfinite_queries_vertex_queries_bits_and_null_outputs(ctx, case):
    import ctypes as C

    from pyfocusr_amd import _hip

    pts, faces, q, want, _ = case("closed")
    q = q[:1000].copy()
    bad = np.array([3, 4, 200, 777])
    dirty = q.copy()
    dirty[3, 0] = np.nan
    dirty[4, 2] = np.inf
    dirty[200] = [-np.inf, 1.0, np.nan]
    dirty[777, 1] = np.nan
    dirty[500] = pts[17]  # exactly on a vertex: every triangle around it gives 0
    f64p = C.POINTER(C.c_double)
    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        clean, _ = surf.winding_number(q)
        for beta in (0.0, 3.0):
            base, _ = surf.winding_number(q, beta=beta)
            w, bound = surf.winding_number(dirty, beta=beta)
            assert np.all(np.isnan(w[bad])) and np.all(np.isnan(bound[bad]))
            others = np.setdiff1d(np.arange(len(q)), np.append(bad, 500))
            assert np.all(np.isfinite(w[others])) and np.isfinite(w[500]) and np.isfinite(bound[500])
            if beta == 0.0:  # a query's sum does not depend on which queries share its packet
                assert np.array_equal(w[others], base[others])
            else:  # the packets, and with them the clusters taken as dipoles, do
                assert np.all(np.abs(w[others] - clean[others]) <= bound[others] + TOL)
            w2, bound2 = surf.winding_number(dirty, beta=beta)
            assert np.array_equal(w, w2, equal_nan=True) and np.array_equal(bound, bound2, equal_nan=True)
            only = np.full(len(q), -7.0)
            args = (surf._h, dirty.ctypes.data_as(f64p), len(dirty), C.c_double(beta))
            _hip._check(surf._lib.pf_surface_winding(*args, only.ctypes.data_as(f64p), None))
            assert np.array_equal(only, w, equal_nan=True)
            _hip._check(surf._lib.pf_surface_winding(*args, None, only.ctypes.data_as(f64p)))
            assert np.array_equal(only, bound, equal_nan=True)
        with pytest.raises(_hip.PfError) as err:
            _hip._check(surf._lib.pf_surface_winding(surf._h, dirty.ctypes.data_as(f64p), 0, C.c_double(0.0), None, None))
        assert err.value.code == -1
    finally:
        surf.close()
    fresh = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:  # before pf_surface_prepare_winding
        with pytest.raises(_hip.PfError) as err:
            _hip._check(fresh._lib.pf_surface_winding(fresh._h, dirty.ctypes.data_as(f64p), len(dirty), C.c_double(0.0), None, None))
        assert err.value.code == -1
    finally:
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opened", [False, True])
def test_hierarchical_mode_within_its_own_bound(ctx, opened):
    from pyfocusr_amd import _hip
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(20000)
    pts, faces = m.points, (wr.open_mesh(m.points, m.faces) if opened else m.faces)
    q = wr.query_set(pts, n_uniform=1000, vertex_step=80)
    want = ref.winding_number(pts, faces, q)
    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        worst = []
        for beta in (2.0, 4.0, 8.0):
            w, bound = surf.winding_number(q, beta=beta)
            err = np.abs(w - want)
            print("beta %g: max |w - w_ref| = %.3e, max bound = %.3e, min (bound - err) = %.3e"
                  % (beta, err.max(), bound.max(), np.min(bound - err)))
            assert np.all(bound >= 0.0)
            assert np.all(err <= bound + TOL)
            worst.append(bound.max())
        assert worst[0] > 0.0  # dipoles were taken: this is not exact mode under another name
        assert worst[0] >= worst[1] >= worst[2]
        with pytest.raises(_hip.PfError) as e:
            surf.winding_number(q, beta=0.5)
        assert e.value.code == -1
    finally:
        surf.close()


@pytest.mark.gpu
def test_winding_and_pseudonormal_signs_agree_on_closed_blob(ctx, case):
    from pyfocusr_amd import point_to_surface_distances, signed_point_to_surface_distances

    pts, faces, q, _, _ = case("closed")
    d, face = point_to_surface_distances(q, (pts, faces), ctx=ctx)
    sw, fw = signed_point_to_surface_distances(q, (pts, faces), ctx=ctx, sign="winding")
    sp, fp = signed_point_to_surface_distances(q, (pts, faces), ctx=ctx, sign="pseudonormal")
    for s, f in ((sw, fw), (sp, fp)):
        assert np.array_equal(np.abs(s), d) and np.array_equal(f, face)
    assert np.array_equal(np.sign(sw), np.sign(sp))
    assert np.sum(sw < 0) > 0 and np.sum(sw > 0) > 0


@pytest.mark.gpu
def test_winding_sign_inside_open_blob(ctx, case):
    from pyfocusr_amd import signed_point_to_surface_distances

    pts, faces, _, _, _ = case("open")
    c = pts.mean(axis=0)
    lower = pts[pts[:, 2] < 0.5 * (pts[:, 2].min() + pts[:, 2].max())]
    q = c + 0.4 * (lower - c)
    want = ref.winding_number(pts, faces, q)
    assert want.min() > 0.5, want.min()  # the expectation itself (0.5486 on the host)
    sd, _ = signed_point_to_surface_distances(q, (pts, faces), ctx=ctx, sign="winding")
    assert np.all(sd < 0)


@pytest.mark.gpu
def test_winding_sign_on_messy_blob(ctx):
    from pyfocusr_amd import signed_point_to_surface_distances
    from pyfocusr_amd.meshgen import messy_blob_mesh

    m = messy_blob_mesh(3000)
    q = wr.query_set(m.points, n_uniform=500, vertex_step=10)
    with pytest.raises(ValueError):
        signed_point_to_surface_distances(q, m, ctx=ctx, sign="pseudonormal")
    with pytest.raises(ValueError, match="inconsistent"):
        signed_point_to_surface_distances(q, m, ctx=ctx, sign="winding")
    q[7, 1] = np.nan
    sd, face = signed_point_to_surface_distances(q, m, ctx=ctx, sign="winding", check_orientation=False)
    fin = np.arange(len(q)) != 7
    assert np.all(np.isfinite(sd[fin])) and np.isnan(sd[7]) and face[7] == -1
    clean = messy_blob_mesh(3000, n_flip=0)  # holes and fins only: what the mode is for
    assert ref.topology_counts(clean.faces)[2] > 0
    sd, _ = signed_point_to_surface_distances(q[fin], clean, ctx=ctx, sign="winding")
    assert np.all(np.isfinite(sd))


@pytest.mark.gpu
def test_points_inside_metrics_and_surface_reuse(ctx, case):
    from pyfocusr_amd import _hip, points_inside, surface_distance_metrics, winding_numbers
    from pyfocusr_amd.meshgen import blob_mesh

    for name in ("closed", "cube", "degenerate"):
        pts, faces, q, want, keep = case(name)
        inside = points_inside(q, (pts, faces), ctx=ctx)
        assert inside.dtype == bool and np.array_equal(inside[keep], (want > 0.5)[keep])
    pts, faces, q, want, _ = case("closed")
    assert not points_inside(np.array([[np.nan, 0.0, 0.0]]), (pts, faces), ctx=ctx)[0]
    surf = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        w1 = winding_numbers(q[:500], surf)
        assert np.array_equal(points_inside(q[:500], surf), w1 > 0.5)
        assert np.array_equal(winding_numbers(q[:500], surf), w1)  # still open and usable
        assert np.max(np.abs(w1 - want[:500])) <= TOL
        d2, _, _ = surf.distance(q[:500])
        assert np.all(np.isfinite(d2))
    finally:
        surf.close()
    a, b = blob_mesh(3000, seed=0), blob_mesh(3000, seed=1)
    mw = surface_distance_metrics(a, b, ctx=ctx, signed=True, sign="winding")
    mp = surface_distance_metrics(a, b, ctx=ctx, signed=True, sign="pseudonormal")
    unsigned = surface_distance_metrics(a, b, ctx=ctx)
    assert set(mw) == set(mp)
    for k, v in unsigned.items():
        assert mw[k] == v and mp[k] == v, k
    assert mw["n_inside_a_to_b"] == mp["n_inside_a_to_b"] and mw["mean_signed_b_to_a"] == mp["mean_signed_b_to_a"]


@pytest.mark.gpu
def test_250k_decisions_agree_with_pseudonormal_signs(ctx):
    from pyfocusr_amd import _hip
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(250000, seed=0), blob_mesh(250000, seed=1)
    surf = _hip.DeviceSurface(b.points, b.faces, ctx=ctx)
    try:
        sd, _, _, _ = surf.signed_distance(a.points)
        w, _ = surf.winding_number(a.points)
    finally:
        surf.close()
    differ = (w > 0.5) != (sd < 0)
    near = np.abs(sd) < 1e-9 * wr.diagonal(b.points)
    print("250k: %d inside by w, %d decisions differ, %d queries near the surface" % (np.sum(w > 0.5), differ.sum(), near.sum()))
    assert not np.any(differ & ~near)
    assert np.mean(differ) < 0.01
