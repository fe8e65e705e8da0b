"""Map distortion and coverage of correspondences (`pf_map_distortion`, `pyfocusr_amd.map_quality`).

CPU: the declaration and the exports, argument errors before the library is loaded, the numpy reference
`_map_quality_ref.distortion` on cases with exact answers (identity, scalings, a stretch, a rotation, a map onto one
vertex, one merged edge, a mirrored target), the reference against an independent SVD of the per-face Jacobian, and the
pure helpers.  GPU: the device against the reference on the smallest cases that reach each mechanism - integers, flags and
masks exactly, every floating-point output bit for bit (only + - x / sqrt occur; profiles/map_quality.md) - the vertex
area against `discrete_curvatures`, two calls bit for bit, `Focusr.map_quality` against a direct call, and point data
through the VTK writer and reader."""
import os
import re

import numpy as np
import pytest

import _curvature_ref as cref
import _map_quality_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SVD_BOUND = 1e-12  # |sigma - sigma_svd| <= SVD_BOUND x max(sigma1, 1) on the faces that are not collapsed


def _blob(n, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    return np.ascontiguousarray(m.points, dtype=np.float64), np.ascontiguousarray(m.faces, dtype=np.int32)


def _messy():
    from pyfocusr_amd.meshgen import messy_blob_mesh

    m = messy_blob_mesh(700)
    return np.ascontiguousarray(m.points, dtype=np.float64), np.ascontiguousarray(m.faces, dtype=np.int32)


def _normals(pts, faces):
    """Unit angle-weighted vertex normals by the curvature reference (zero where a vertex has none)."""
    return np.ascontiguousarray(cref.curvatures(pts, faces)["normals"])


def _identity(n):
    return np.arange(n, dtype=np.int32)


def _case_tetrahedron():
    pts, faces = cref.tetrahedron()
    return pts, faces, pts, _identity(4), None, _normals(pts, faces)


def _case_nearest():
    (ps, fs), (pt, ft) = _blob(700, 1), _blob(900, 2)
    return ps, fs, pt, ref.nearest_vertex_map(ps, pt).astype(np.int32), None, _normals(pt, ft)


def _case_surface():
    (ps, fs), (pt, ft) = _blob(700, 1), _blob(900, 2)
    vertices, bary = ref.partial_surface_map(ps, pt, ft, 200)
    return ps, fs, pt, vertices, bary, _normals(pt, ft)


def _case_messy():
    pts, faces = _messy()
    return pts, faces, pts, _identity(len(pts)), None, _normals(pts, faces)


def _case_cone():
    pts, faces = cref.cone_fan(200)
    return pts, faces, pts, _identity(len(pts)), None, None


def _case_zero_area():
    pts, faces = cref.with_zero_area_triangle(*_blob(700, 1))
    return pts, faces, pts, _identity(len(pts)), None, _normals(pts, faces)


def _case_one_vertex():
    (ps, fs), (pt, ft) = _blob(700, 1), _blob(900, 2)
    return ps, fs, pt, np.zeros(700, dtype=np.int32), None, _normals(pt, ft)


def _case_blob40000():
    pts, faces = _blob(40000, 5)
    return pts, faces, pts, _identity(len(pts)), None, None


_CASES = {
    "tetrahedron": _case_tetrahedron,  # n = 4: the fewest index bits, one block
    "nearest": _case_nearest,          # blob700 -> blob900 by nearest vertex: collapsed faces, shared owners
    "surface": _case_surface,          # ... as a 3-corner map, 500 rows unmapped
    "messy700": _case_messy,           # non-manifold edges, unreferenced vertices, reversed faces
    "cone": _case_cone,                # one vertex run of 200 half-edges; no normals
    "zero_area": _case_zero_area,      # an invalid face with mapped corners
    "one_vertex": _case_one_vertex,    # a run of 700 owners: eleven runs of 64
    "blob40000": _case_blob40000,      # 79 996 faces > 65 536: the totals reach the third level of the tree
}
_cache = {}


def case(name):
    """(arguments of `Context.map_distortion` / `ref.distortion`, reference) of a case, computed once, never changed."""
    if name not in _cache:
        ps, fs, pt, mv, mw, nrm = _CASES[name]()
        r = ref.distortion(ps, fs, pt, mv, mw, nrm)
        for v in list(r.values()) + [ps, fs, pt, mv, mw, nrm]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = ((ps, fs, pt, mv, mw, nrm), r)
    return _cache[name]


# ------------------------------------------------------------------------------ CPU
def test_entry_point_is_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_map_distortion\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_map_distortion is not declared in the header"
    assert len(m.group(1).split(",")) == 22
    assert len(_hip.SIGNATURES["pf_map_distortion"][1]) == 22
    assert callable(_hip.Context.map_distortion)


def test_package_exports():
    import pyfocusr_amd

    for name in ("map_distortion", "conformal_distortion", "isometric_distortion", "symmetric_dirichlet", "distortion_on_mesh"):
        assert callable(getattr(pyfocusr_amd, name))
    assert callable(pyfocusr_amd.Focusr.map_quality)


def test_argument_errors_before_the_library_is_loaded(monkeypatch):
    from pyfocusr_amd import Focusr, PolyMesh, _hip, map_quality

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    pts, faces = cref.tetrahedron()
    ident = _identity(4)
    bary = np.tile([1.0, 0.0, 0.0], (4, 1))
    corners = np.tile(ident[:, None], (1, 3))
    quads = np.array([[0, 1, 2, 3]], dtype=np.int32)
    nan_pts = pts.copy()
    nan_pts[2, 1] = np.nan
    nan_bary = bary.copy()
    nan_bary[1, 2] = np.inf
    hole = corners.copy()
    hole[2, 1] = -1
    bad = [
        dict(source=(pts, quads), target=pts, vertex_map=ident),                       # the source must be triangles
        dict(source=(nan_pts, faces), target=pts, vertex_map=ident),
        dict(source=(pts, faces + 1), target=pts, vertex_map=ident),
        dict(source=(pts, faces), target=pts[:, :2], vertex_map=ident),                # target points (k, 3)
        dict(source=(pts, faces), target=pts[:0], vertex_map=ident),
        dict(source=(pts, faces), target=(pts, faces + 1), vertex_map=ident),          # target face out of range
        dict(source=(pts, faces), target=nan_pts, vertex_map=ident),                   # a mapped row reads a NaN point
        dict(source=(pts, faces), target=pts),                                         # neither map
        dict(source=(pts, faces), target=pts, vertex_map=ident, surface_map=(corners, bary)),  # both
        dict(source=(pts, faces), target=pts, vertex_map=ident[:3]),
        dict(source=(pts, faces), target=pts, vertex_map=ident.astype(np.float64)),
        dict(source=(pts, faces), target=pts, vertex_map=ident + 1),                   # 4 is no target vertex
        dict(source=(pts, faces), target=pts, vertex_map=ident - 2),                   # -2 is not "unmapped"
        dict(source=(pts, faces), target=pts, surface_map=(corners, bary[:, :2])),
        dict(source=(pts, faces), target=pts, surface_map=(corners[:3], bary[:3])),
        dict(source=(pts, faces), target=pts, surface_map=(corners, nan_bary)),
        dict(source=(pts, faces), target=pts, surface_map={"vertices": corners}),
        dict(source=(pts, faces), target=pts, surface_map=corners),
        dict(source=(pts, faces), target=pts, surface_map=(hole, bary)),               # -1 behind a vertex: not "unmapped"
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            map_quality.map_distortion(**kwargs)
    with pytest.raises(ValueError):
        map_quality.map_distortion(PolyMesh(pts, quads), pts, vertex_map=ident)
    with pytest.raises(ValueError):
        map_quality.conformal_distortion(np.ones(3), np.ones(2))
    result = {"vertex_sigma_max": np.ones(4), "vertex_sigma_min": np.ones(4)}
    with pytest.raises(ValueError):
        map_quality.distortion_on_mesh(PolyMesh(pts, faces), result, fields=("sigma_max", "torsion"))
    with pytest.raises(ValueError):
        map_quality.distortion_on_mesh(PolyMesh(pts[:3], faces[:1] * 0 + [0, 1, 2]), result)
    reg = Focusr.__new__(Focusr)  # no correspondence has been computed on this object
    reg.corresponding_target_idx_for_each_source_pt = None
    for kind in ("nearest", "surface", "geodesic"):
        with pytest.raises(ValueError):
            reg.map_quality(kind)


def test_reference_identity_is_exact():
    pts, faces = _blob(700, 1)
    r = ref.distortion(pts, faces, pts, _identity(700), None, _normals(pts, faces))
    assert np.all(r["face_flags"] == ref.VALID)
    assert np.all(r["face_sigma"] == 1.0) and np.all(r["face_area_ratio"] == 1.0)
    assert np.all(r["vertex_sigma"] == 1.0)
    assert r["totals"][2] == r["totals"][0] and r["totals"][1] == r["totals"][0] > 0.0  # Dirichlet energy = area
    assert r["totals"][3] == r["totals"][0] and r["totals"][5] == 0.0 and r["totals"][6] == 0.0
    assert np.array_equal(r["report"], [1396, 0, 0, 0, 0, 700, 1, 0])
    assert np.all(r["target_count"] == 1) and np.array_equal(r["target_premass"], r["vertex_area"])
    assert np.array_equal(r["vertex_area"], cref.curvatures(pts, faces)["area"])


def test_reference_scaling_by_two_is_exact():
    pts, faces = _blob(700, 1)
    r = ref.distortion(pts, faces, 2.0 * pts, _identity(700))
    assert np.all(r["face_sigma"] == 2.0) and np.all(r["face_area_ratio"] == 4.0)
    assert np.array_equal(r["report"], [1396, 0, -1, 0, 0, 700, 1, -1])


def test_reference_stretch_and_rotation():
    pts, faces = ref.grid_mesh(9, 7)
    r = ref.distortion(pts, faces, pts * [2.0, 1.0, 1.0], _identity(len(pts)))
    assert np.all(np.abs(r["face_sigma"] - [2.0, 1.0]) <= 8 * EPS)
    assert np.all(np.abs(r["face_area_ratio"] - 2.0) <= 8 * EPS)
    pts, faces = _blob(700, 1)
    r = ref.distortion(pts, faces, pts @ ref.rotation().T, _identity(700))
    assert np.all(np.abs(r["face_sigma"] - 1.0) <= 64 * EPS)


def test_reference_everything_onto_one_vertex():
    r = case("one_vertex")[1]
    assert np.all(r["face_flags"] == ref.VALID | ref.COLLAPSED)
    assert np.all(r["face_sigma"] == 0.0) and np.all(r["face_area_ratio"] == 0.0)
    assert r["target_count"][0] == 700 and np.all(r["target_count"][1:] == 0)
    A = r["vertex_area"]
    runs = [0.0] * 11
    for k in range(11):
        for a in A[64 * k:64 * (k + 1)]:
            runs[k] = runs[k] + a
    total = 0.0
    for s in runs:
        total = total + s
    assert r["target_premass"][0] == total and np.all(r["target_premass"][1:] == 0.0)
    assert np.array_equal(r["report"], [1396, 1396, 0, 0, 0, 1, 700, 0])
    assert r["totals"][5] == r["totals"][0] and r["totals"][1] == 0.0 and r["totals"][2] == 0.0


def test_reference_one_merged_edge():
    pts, faces = _blob(700, 1)
    vmap = _identity(700).copy()
    i0, i1, i2 = faces[10]
    vmap[i1] = i0  # the edge (i0, i1) of face 10 - and of its neighbour across it - becomes a point
    r = ref.distortion(pts, faces, pts, vmap)
    svd = ref.svd_sigmas(pts, faces, pts[vmap])
    merged = np.flatnonzero((r["face_flags"] & ref.COLLAPSED) != 0)
    assert 10 in merged and len(merged) == 2
    assert np.all(r["face_sigma"][merged, 1] == 0.0) and np.all(r["face_sigma"][merged, 0] > 0.0)
    assert np.all(np.abs(r["face_sigma"][merged] - svd[merged]) <= SVD_BOUND * np.maximum(svd[merged, :1], 1.0))
    assert r["target_count"][i0] == 2 and r["target_count"][i1] == 0


def test_reference_mirrored_target_flips_every_face():
    pts, faces = _blob(700, 1)
    mp, mf = ref.mirrored(pts, faces)
    nrm = _normals(mp, mf)
    assert np.all(np.sum(nrm * mp, axis=1) > 0.0)  # outward again (the blob is star-shaped around the origin)
    r = ref.distortion(pts, faces, mp, _identity(700), None, nrm)
    assert np.all(r["face_flags"] == ref.VALID | ref.FLIPPED)
    assert np.all(np.abs(r["face_sigma"] - 1.0) <= 64 * EPS)
    assert r["report"][2] == 1396 and r["report"][7] == 700 and r["totals"][6] == r["totals"][0]
    plain = ref.distortion(pts, faces, mp, _identity(700))  # orientation=False: no normals
    assert np.all(plain["face_flags"] == ref.VALID) and plain["report"][2] == -1 and plain["report"][7] == -1
    assert np.array_equal(plain["face_sigma"], r["face_sigma"])


@pytest.mark.parametrize("name", ["nearest", "surface"])
def test_reference_against_the_svd(name):
    """Worst |sigma - sigma_svd| / max(sigma1, 1) on this host: nearest 1.2e-15, surface 7.9e-16 (profiles/map_quality.md),
    both under a tenth of the bound."""
    (ps, fs, pt, mv, mw, _), r = case(name)
    y = ref.images(pt, mv, mw)[0]
    svd = ref.svd_sigmas(ps, fs, y)
    use = ((r["face_flags"] & ref.VALID) != 0) & ((r["face_flags"] & ref.COLLAPSED) == 0)
    assert use.sum() >= 100
    ratio = np.abs(r["face_sigma"][use] - svd[use]) / np.maximum(svd[use, :1], 1.0)
    print("%s: %d faces, worst |sigma - svd| / max(sigma1, 1) = %.3e" % (name, use.sum(), ratio.max()))
    assert ratio.max() <= SVD_BOUND
    # the area ratio is the product of the singular values
    product = r["face_sigma"][use, 0] * r["face_sigma"][use, 1]
    assert np.all(np.abs(product - r["face_area_ratio"][use]) <= 1e-12 * np.maximum(r["face_area_ratio"][use], 1.0))
    if name == "nearest":
        assert r["report"][1] > 0  # 700 vertices onto 900 by nearest vertex: some faces collapse
    else:
        assert r["report"][4] > 0 and np.all(r["face_sigma"][(r["face_flags"] & ref.UNMAPPED) != 0] == 0.0)


def test_helpers_and_their_rules_at_zero():
    from pyfocusr_amd import conformal_distortion, isometric_distortion, symmetric_dirichlet

    s1 = np.array([1.0, 2.0, 4.0, 0.5, 3.0, 0.0])
    s2 = np.array([1.0, 1.0, 0.5, 0.25, 0.0, 0.0])
    assert np.array_equal(conformal_distortion(s1, s2), [1.0, 2.0, 8.0, 2.0, np.inf, 0.0])
    assert np.array_equal(isometric_distortion(s1, s2), [1.0, 2.0, 4.0, 4.0, np.inf, 0.0])
    assert np.array_equal(symmetric_dirichlet(s1, s2), [4.0, 6.25, 16.0 + 0.25 + 0.0625 + 4.0, 0.25 + 0.0625 + 4.0 + 16.0, np.inf, 0.0])


def test_distortion_on_mesh_stores_point_data():
    from pyfocusr_amd import PolyMesh, distortion_on_mesh

    pts, faces = cref.tetrahedron()
    mesh = PolyMesh(pts, faces)
    result = {"vertex_sigma_max": np.array([1.0, 2.0, 3.0, 0.0]), "vertex_sigma_min": np.array([1.0, 0.5, 0.0, 0.0]),
              "vertex_area": np.full(4, 0.25), "vertex_flipped": np.array([True, False, False, False]),
              "vertex_collapsed": np.array([False, False, True, True])}
    names = distortion_on_mesh(mesh, result, fields=("sigma_max", "area", "flipped", "collapsed", "conformal", "isometric"))
    assert names == ["map_sigma_max", "map_area", "map_flipped", "map_collapsed", "map_conformal", "map_isometric"]
    stored = dict(mesh.point_data)
    assert np.array_equal(stored["map_sigma_max"], result["vertex_sigma_max"]) and np.array_equal(stored["map_flipped"], [1.0, 0.0, 0.0, 0.0])
    assert np.array_equal(stored["map_conformal"], [1.0, 4.0, np.inf, 0.0]) and np.array_equal(stored["map_isometric"], [1.0, 2.0, np.inf, 0.0])


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


_device = {}


def device(ctx, name):
    """`Context.map_distortion` of a case: one device call per case and module."""
    if name not in _device:
        ps, fs, pt, mv, mw, nrm = case(name)[0]
        _device[name] = ctx.map_distortion(ps, fs, pt, mv, mw, nrm)
    return _device[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_CASES))
def test_device_equals_the_reference(ctx, name):
    r = case(name)[1]
    dev = device(ctx, name)
    print("%s: report device %s reference %s" % (name, dev["report"].tolist(), r["report"].tolist()))
    for field in ref.INT_FIELDS:
        assert dev[field].dtype == r[field].dtype and np.array_equal(dev[field], r[field]), (name, field)
    for field in ref.FLOAT_FIELDS:
        scale = np.max(np.abs(r[field])) if r[field].size else 0.0
        worst = np.max(np.abs(dev[field] - r[field])) / scale if scale > 0.0 else 0.0
        print("%s: %-15s worst |device - reference| / max |reference| = %.3e" % (name, field, worst))
    for field in ref.FLOAT_FIELDS:
        assert np.all(np.isfinite(dev[field])), (name, field)
        assert np.array_equal(dev[field], r[field]), (name, field)
    assert dev["device_ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nearest", "messy700", "zero_area"])
def test_vertex_area_is_the_curvature_units(ctx, name):
    from pyfocusr_amd import discrete_curvatures

    ps, fs = case(name)[0][:2]
    assert np.array_equal(device(ctx, name)["vertex_area"], discrete_curvatures(ps, fs, ctx=ctx)["area"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nearest", "surface", "one_vertex"])
def test_two_calls_give_the_same_bits(ctx, name):
    ps, fs, pt, mv, mw, nrm = case(name)[0]
    a, b = device(ctx, name), ctx.map_distortion(ps, fs, pt, mv, mw, nrm)
    for field in sorted(a):
        if field != "device_ms":
            assert np.asarray(a[field]).tobytes() == np.asarray(b[field]).tobytes(), field


@pytest.mark.gpu
def test_map_distortion_names_and_scalars(ctx):
    from pyfocusr_amd import map_distortion

    (ps, fs, pt, mv, _, _), r = case("nearest")
    _, ft = _blob(900, 2)
    out = map_distortion((ps, fs), (pt, ft), vertex_map=mv, ctx=ctx)
    dev = device(ctx, "nearest")
    assert np.array_equal(out.sigma_max, dev["face_sigma"][:, 0]) and np.array_equal(out.sigma_min, dev["face_sigma"][:, 1])
    assert np.array_equal(out.area_ratio, dev["face_area_ratio"]) and np.array_equal(out.vertex_area, dev["vertex_area"])
    assert np.array_equal(out.valid, (r["face_flags"] & ref.VALID) != 0)
    assert np.array_equal(out.collapsed, (r["face_flags"] & ref.COLLAPSED) != 0)
    assert out.flipped.dtype == bool and out.report[2] >= 0 and out.report[7] >= 0  # the target has faces: normals
    assert np.array_equal(out.vertex_collapsed, (r["vertex_flags"] & ref.COLLAPSED) != 0)
    assert np.array_equal(out.target_count, r["target_count"]) and np.array_equal(out.target_premass, r["target_premass"])
    assert out.dirichlet_energy == r["totals"][2] and out.area_distortion == r["totals"][1] / r["totals"][0]
    assert out.collapsed_area_fraction == r["totals"][5] / r["totals"][0] > 0.0
    assert out.target_vertices_hit_fraction == r["report"][5] / 900.0
    bare = map_distortion((ps, fs), pt, vertex_map=mv, ctx=ctx)  # bare points: no flip flags
    assert not bare.flipped.any() and bare.report[2] == -1 and bare.flipped_area_fraction == 0.0
    off = map_distortion((ps, fs), (pt, ft), vertex_map=mv, orientation=False, ctx=ctx)
    assert off.report[2] == -1 and np.array_equal(off.sigma_max, out.sigma_max)
    surface = map_distortion((ps, fs), (pt, ft), surface_map=dict(zip(("vertices", "bary"), case("surface")[0][3:5])), ctx=ctx)
    assert np.array_equal(surface.sigma_max, case("surface")[1]["face_sigma"][:, 0])
    assert np.array_equal(surface.unmapped, (case("surface")[1]["face_flags"] & ref.UNMAPPED) != 0)


@pytest.mark.gpu
def test_library_refuses_bad_arguments(ctx):
    from pyfocusr_amd import _hip

    pts, faces = cref.tetrahedron()
    ident = _identity(4)
    nan_pts = pts.copy()
    nan_pts[1, 0] = np.nan
    for args, code in (((pts, faces + 1, pts, ident), -1), ((pts, faces, pts, ident + 1), -1), ((pts, faces, pts, ident - 2), -1),
                       ((pts, faces, nan_pts, ident), -1), ((nan_pts, faces, pts, ident), -1),
                       ((pts, faces, pts, ident, None, nan_pts), -1),
                       ((pts, np.array([[0, 1, 1]], dtype=np.int32), pts, ident), _hip.PF_E_DEGENERATE)):
        with pytest.raises(_hip.PfError) as e:
            ctx.map_distortion(*args)  # (map_distortion would have refused most of them first)
        assert e.value.code == code
    unmapped = ident.copy()
    unmapped[1] = -1  # an unmapped row may point at anything: its NaN target point is not read
    out = ctx.map_distortion(pts, faces, nan_pts, unmapped)
    assert np.array_equal(out["report"][:5], [1, 0, -1, 3, 3]) and np.all(np.isfinite(out["face_sigma"]))


@pytest.mark.gpu
def test_focusr_map_quality_is_a_direct_call(ctx, golden):
    from pyfocusr_amd import Focusr, PolyMesh, map_distortion

    gt, gs = golden("target_mesh"), golden("source_mesh")
    target, source = PolyMesh(gt["points"], gt["faces"]), PolyMesh(gs["points"], gs["faces"])
    np.random.seed(0)
    reg = Focusr(target, source, icp_register_first=False, list_features_to_calc=[], n_spectral_features=3, n_extra_spectral=0,
                 ctx=ctx, registration=lambda src, tgt, kind: tgt)
    with pytest.raises(ValueError):
        reg.map_quality("nearest")
    reg.align_maps()
    with pytest.raises(ValueError):
        reg.map_quality("surface")
    idx = np.asarray(reg.corresponding_target_idx_for_each_source_pt).copy()
    got = reg.map_quality("nearest")
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, idx)
    want = map_distortion(reg.graph_source.vtk_mesh, reg.graph_target.vtk_mesh, vertex_map=idx, ctx=ctx)
    assert sorted(got) == sorted(want) and got.report[0] > 0
    for field in sorted(got):
        if field != "device_ms":
            assert np.asarray(got[field]).tobytes() == np.asarray(want[field]).tobytes(), field
    reg.get_surface_final_node_locations()
    surface = reg.map_quality("surface")
    assert surface.sigma_max.shape == (len(gs["faces"]),) and surface.report[0] > 0


@pytest.mark.gpu
def test_distortion_on_mesh_round_trips_through_vtk(ctx, tmp_path):
    from pyfocusr_amd import PolyMesh, distortion_on_mesh, map_distortion, read_vtk_mesh, write_vtk_mesh

    (ps, fs, pt, mv, _, _), _ = case("nearest")
    _, ft = _blob(900, 2)
    mesh = PolyMesh(ps.copy(), fs.copy())
    result = map_distortion(mesh, (pt, ft), vertex_map=mv, ctx=ctx)
    names = distortion_on_mesh(mesh, result)
    assert names == ["map_sigma_max", "map_sigma_min"]
    names += distortion_on_mesh(mesh, result, fields=("area", "flipped", "collapsed"))
    stored = dict(mesh.point_data)
    assert sorted(stored) == sorted(names)
    assert np.array_equal(stored["map_sigma_max"], result.vertex_sigma_max) and np.array_equal(stored["map_area"], result.vertex_area)
    assert np.array_equal(stored["map_collapsed"], result.vertex_collapsed.astype(np.float64))
    path = str(tmp_path / "distorted.vtk")
    write_vtk_mesh(mesh, path)
    back = dict(read_vtk_mesh(path).point_data)
    for name in names:
        assert np.array_equal(np.asarray(back[name], dtype=np.float64), stored[name]), name
