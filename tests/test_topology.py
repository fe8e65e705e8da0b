"""Mesh topology and face orientation (`pf_mesh_topology`, `pyfocusr_amd.topology`).

CPU: the numpy / scipy reference `_topology_ref.topology` on shapes with known answers, on a blob with reversed faces and
on the messy blob; `orient_faces` and `extract_patches` over a reference-computed topology (the device call replaced by
the reference); argument errors before the library is loaded; the declaration and the helper names.  GPU: every integer
output of the device equal to the reference, the signed volume within 1e-12 x sum |a . (b x c)| / 6, two calls bit for
bit, the counts against the library's two other counters, bad input, and the two repairs the feature exists for: signed
distances and the core path's W on a blob whose reversed faces `orient_faces` put back."""
import os
import re

import numpy as np
import pytest

import _curvature_ref as cref
import _topology_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reversed_blob(n, seed, count, rng_seed):
    """(points, faces with `count` random faces reversed, the clean faces, the reversed set)"""
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    which = np.sort(np.random.default_rng(rng_seed).choice(len(m.faces), size=count, replace=False))
    return m.points, ref.reverse(m.faces, which), m.faces, which


def _messy():
    from pyfocusr_amd.meshgen import messy_blob_mesh

    m = messy_blob_mesh(700, seed=2)
    return m.points, m.faces


# name -> (points, faces); the points of the ribbons take no part (they are open, or given without the outward rule)
_MESHES = {
    "tetrahedron": ref.tetrahedron,                                   # n = 4: the fewest index bits
    "cube_one_reversed": lambda: (ref.cube()[0], ref.reverse(ref.cube()[1], [5])),
    "cube_all_reversed": lambda: (ref.cube()[0], ref.reverse(ref.cube()[1], np.arange(12))),
    "torus": ref.torus_grid,
    "cylinder": ref.open_cylinder,
    "moebius": ref.moebius,
    "nested_spheres": ref.nested_spheres,
    "two_triangles": ref.two_triangles_at_a_vertex,
    "fin": ref.tetrahedron_with_fin,
    "blob700_reversed": lambda: _reversed_blob(700, 1, 40, 7)[:2],      # 1396 faces: several blocks
    "messy700": _messy,                                               # holes, fins, reversed faces, stranded vertices
    "blob5000_reversed": lambda: _reversed_blob(5000, 0, 200, 8)[:2],   # 2 %: waves with one patch and waves with several
    "ribbon_open": lambda: ref.ribbon(4096, closed=False),            # a path of 4096 faces: many blocks, the largest diameter
    "ribbon_band": lambda: ref.ribbon(4096, closed=True),
}
_cache = {}


def case(name, outward=True):
    """(points, faces, reference) of a test mesh, computed once and never changed."""
    if (name, outward) not in _cache:
        pts, faces = _MESHES[name]()
        pts, faces = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32)
        r = ref.topology(len(pts), faces, pts, outward=outward)
        for v in list(r.values()) + list(r["patches"].values()) + [pts, faces]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[(name, outward)] = (pts, faces, r)
    return _cache[(name, outward)]


# ------------------------------------------------------------------------------ CPU
def test_topology_entry_point_is_declared_and_bound():
    import pyfocusr_amd
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_mesh_topology\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_mesh_topology is not declared in the header"
    assert len(m.group(1).split(",")) == 14
    assert len(_hip.SIGNATURES["pf_mesh_topology"][1]) == 14
    assert callable(_hip.Context.mesh_topology)
    for name in ("mesh_topology", "orient_faces", "is_consistently_oriented", "extract_patches"):
        assert callable(getattr(pyfocusr_amd, name))
    assert "bow-tie" in pyfocusr_amd.topology.__doc__


def _single(r, **want):
    assert r["n_patches"] == 1
    for key, value in want.items():
        assert r["patches"][key][0] == value, (key, r["patches"][key][0], value)


def test_reference_tetrahedron():
    _, _, r = case("tetrahedron")
    _single(r, closed=True, genus=0, euler=2, orientable=True, manifold=True, n_flipped=0, n_faces=4, n_vertices=4, n_edges=6)
    assert (r["n_edges"], r["n_boundary_edges"], r["n_nonmanifold_edges"], r["n_inconsistent_edges"]) == (6, 0, 0, 0)
    assert np.array_equal(np.sort(r["face_neighbours"], axis=1), [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    assert not r["flip"].any() and np.all(r["boundary_loop"] == -1)
    np.testing.assert_allclose(r["patches"]["signed_volume"][0], 8.0 / 3.0, rtol=1e-15)


def test_reference_cube_reversed_faces():
    _, _, r = case("cube_one_reversed")
    assert np.array_equal(np.flatnonzero(r["flip"]), [5]) and r["n_inconsistent_edges"] == 3
    _single(r, closed=True, genus=0, euler=2, n_flipped=1)
    np.testing.assert_allclose(r["patches"]["signed_volume"][0], 1.0, rtol=1e-15)
    _, _, r = case("cube_all_reversed")
    assert r["flip"].all() and r["n_inconsistent_edges"] == 0
    np.testing.assert_allclose(r["patches"]["signed_volume"][0], 1.0, rtol=1e-15)
    _, _, r = case("cube_all_reversed", outward=False)
    assert not r["flip"].any() and r["patches"]["signed_volume"][0] == 0.0


def test_reference_torus_cylinder_moebius():
    _, _, r = case("torus")
    _single(r, genus=1, euler=0, closed=True, orientable=True, n_boundary_loops=0)
    assert r["patches"]["signed_volume"][0] > 0.0 and not r["flip"].any()
    _, _, r = case("cylinder")
    _single(r, genus=0, euler=0, closed=False, orientable=True, n_boundary_loops=2, signed_volume=0.0)
    assert r["n_boundary_loops"] == 2 and r["n_boundary_edges"] == 24
    rim = r["boundary_loop"][r["boundary_loop"] >= 0]
    assert np.array_equal(np.bincount(rim), [12, 12])
    pts, faces, r = case("moebius")
    assert len(faces) == 24
    _single(r, orientable=False, n_boundary_loops=1, closed=False, genus=-1, euler=0, n_flipped=0)
    assert not r["flip"].any() and r["n_boundary_loops"] == 1 and r["n_boundary_edges"] == 24


def test_reference_several_patches():
    pts, faces, r = case("nested_spheres")
    assert r["n_patches"] == 2 and np.array_equal(r["patches"]["n_faces"], [116, 76])
    assert np.array_equal(r["flip"], np.arange(len(faces)) >= 116)  # the inner blob was reversed: outward on its own
    assert np.all(r["patches"]["signed_volume"] > 0.0) and np.all(r["patches"]["genus"] == 0)
    _, _, r = case("nested_spheres", outward=False)
    assert not r["flip"].any()
    _, _, r = case("two_triangles")
    assert r["n_patches"] == 2 and np.array_equal(r["patch"], [0, 1]) and r["n_boundary_loops"] == 2
    assert np.array_equal(r["boundary_loop"], [[0, 0, 0], [1, 1, 1]])
    _, _, r = case("fin")
    assert r["n_nonmanifold_edges"] == 1 and r["n_patches"] == 2 and np.array_equal(r["patch"], [0, 0, 0, 0, 1])
    assert np.sum(r["face_neighbours"] == -2) == 3 and r["face_neighbours"][4, 0] == -2
    assert np.array_equal(r["patches"]["manifold"], [False, False]) and np.array_equal(r["patches"]["genus"], [-1, -1])
    assert np.array_equal(r["patches"]["closed"], [False, False]) and np.all(r["patches"]["signed_volume"] == 0.0)


def test_reference_ribbons():
    _, faces, r = case("ribbon_open")
    reversed_ = np.arange(4096) % 3 == 0
    assert np.array_equal(r["flip"], reversed_)  # the root is one of them: the minimum-change rule, not rel, decides
    _single(r, orientable=True, n_boundary_loops=1, genus=0, euler=1)
    _, _, r = case("ribbon_band")
    assert np.array_equal(r["flip"], reversed_)
    _single(r, orientable=True, n_boundary_loops=2, genus=0, euler=0)


def test_reference_blob_with_reversed_faces():
    pts, faces, clean, which = _reversed_blob(700, 1, 40, 7)
    _, _, r = case("blob700_reversed")
    assert np.array_equal(np.flatnonzero(r["flip"]), which)
    assert np.array_equal(ref.reverse(faces, r["flip"]), clean)
    _single(r, closed=True, genus=0, euler=2, n_flipped=40)
    assert r["patches"]["signed_volume"][0] > 0.0


def test_reference_messy_blob():
    from pyfocusr_amd.meshgen import blob_mesh

    pts, faces, r = case("messy700")
    assert r["n_patches"] == 3 and np.array_equal(r["patches"]["n_faces"], [1370, 1, 1])
    # the reversed faces of the main patch: those whose reverse, not they themselves, is a face of the clean blob
    def rotations(f):
        return {(a, b, c) for a, b, c in np.concatenate([f, f[:, [1, 2, 0]], f[:, [2, 0, 1]]]).tolist()}

    clean = rotations(blob_mesh(700, seed=2).faces)
    was_reversed = np.array([tuple(f) not in clean and (f[0], f[2], f[1]) in clean for f in faces.tolist()])
    assert was_reversed.sum() == 2 and np.all(r["patch"][was_reversed] == 0)
    assert np.array_equal(r["flip"], was_reversed)
    c = cref.curvatures(pts, faces)["topology"]
    assert [r["n_edges"], r["n_boundary_edges"], r["n_nonmanifold_edges"], r["n_inconsistent_edges"]] == c[:4].tolist()
    assert np.all(r["patches"]["signed_volume"] == 0.0)  # no patch is closed


def _reference_as_device(monkeypatch):
    from pyfocusr_amd import _hip, topology

    def no_device(*a, **k):
        raise AssertionError("device touched")

    def by_reference(pts, faces, outward, ctx):
        return ref.as_device_output(ref.topology(len(pts), faces, pts if outward else None, outward=outward))

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    monkeypatch.setattr(topology, "_device_topology", by_reference)


def test_orient_faces_over_the_reference(monkeypatch):
    from pyfocusr_amd import PolyMesh, is_consistently_oriented, mesh_topology, orient_faces

    _reference_as_device(monkeypatch)
    pts, faces, clean, which = _reversed_blob(700, 1, 40, 7)
    height = pts[:, 2].copy()
    mesh = PolyMesh(pts.copy(), faces.copy(), [("height", height)])
    fixed, topo = orient_faces(mesh)
    assert np.array_equal(mesh.faces, faces) and np.array_equal(mesh.points, pts)  # the input is untouched
    assert np.array_equal(fixed.faces, clean) and fixed.faces.dtype == np.int32 and np.array_equal(fixed.points, pts)
    assert fixed.points is not mesh.points and fixed.faces is not mesh.faces
    assert [n for n, _ in fixed.point_data] == ["height"] and np.array_equal(fixed.point_data[0][1], height)
    assert np.array_equal(np.flatnonzero(topo.flip), which) and topo.n_inconsistent_edges > 0 and topo.n_patches == 1
    assert not is_consistently_oriented(mesh) and is_consistently_oriented(fixed)
    assert not is_consistently_oriented(ref.moebius())  # no inconsistent edge decides that: the patch is one-sided
    # the table of the package (vectorised, from the per-face outputs) against the reference's (patch by patch)
    for name in ("messy700", "nested_spheres", "fin", "moebius", "cylinder", "two_triangles", "ribbon_band"):
        p, f, r = case(name)
        t = mesh_topology((p, f))
        assert sorted(t.patches) == sorted(r["patches"])
        for key in r["patches"]:
            assert np.array_equal(t.patches[key], r["patches"][key]), (name, key)
        assert (t.n_patches, t.n_boundary_loops, t.n_edges) == (r["n_patches"], r["n_boundary_loops"], r["n_edges"])


def test_extract_patches_over_the_reference(monkeypatch):
    from pyfocusr_amd import PolyMesh, extract_patches

    _reference_as_device(monkeypatch)
    pts, faces, r = case("messy700")
    tag = np.arange(len(pts), dtype=np.float64)
    mesh = PolyMesh(pts.copy(), faces.copy(), [("tag", tag)])
    sub, index = extract_patches(mesh)
    main = faces[r["patch"] == 0]
    assert np.array_equal(index, np.unique(main)) and len(index) < len(pts)  # the stranded vertices are gone
    assert np.array_equal(sub.points, pts[index]) and np.array_equal(index[sub.faces], main)
    assert np.array_equal(sub.point_data[0][1], tag[index]) and sub.point_data[0][0] == "tag"
    assert np.array_equal(mesh.faces, faces) and np.array_equal(mesh.points, pts)
    sub, index = extract_patches(mesh, which=[2, 1])
    assert np.array_equal(index[sub.faces], faces[r["patch"] >= 1]) and len(sub.faces) == 2
    sub, index = extract_patches(mesh, which=1)
    assert np.array_equal(index[sub.faces], faces[r["patch"] == 1])
    two = extract_patches(ref.two_triangles_at_a_vertex())[0]  # a tie: the lower patch id
    assert np.array_equal(two.points, ref.two_triangles_at_a_vertex()[0][:3])
    for bad in ("smallest", 3, [0, 7], -1, 0.5):
        with pytest.raises(ValueError):
            extract_patches(mesh, which=bad)


def test_argument_errors_before_the_library_is_loaded(monkeypatch):
    from pyfocusr_amd import PolyMesh, _hip, topology

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    pts, faces = ref.tetrahedron()
    quads = np.array([[0, 1, 2, 3]], dtype=np.int32)
    bad = [(pts, quads), (pts, faces.ravel()), (pts, faces[:0]), (pts, faces.astype(np.float64)), (pts[:3], faces), (pts[:0], faces),
           (pts[:, :2], faces), (pts, faces - 1)]
    for p, f in bad:
        for call in (topology.mesh_topology, topology.orient_faces, topology.is_consistently_oriented, topology.extract_patches):
            with pytest.raises(ValueError):
                call((p, f))
    with pytest.raises(ValueError, match="triangles"):
        topology.mesh_topology(PolyMesh(pts, quads))


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


_device = {}


def device(ctx, name, outward=True):
    """`mesh_topology` of a test mesh: one device call per mesh and module."""
    if (name, outward) not in _device:
        from pyfocusr_amd import mesh_topology

        pts, faces, _ = case(name, outward)
        _device[(name, outward)] = mesh_topology((pts, faces), outward=outward, ctx=ctx)
    return _device[(name, outward)]


def _assert_equal_integers(dev, r, what):
    for key in ("n_edges", "n_boundary_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "n_patches", "n_boundary_loops"):
        assert dev[key] == r[key], (what, key, dev[key], r[key])
    for key in ("face_neighbours", "patch", "boundary_loop"):
        assert dev[key].dtype == np.int32 and np.array_equal(dev[key], r[key]), (what, key)
    assert dev["flip"].dtype == bool and np.array_equal(dev["flip"], r["flip"]), (what, "flip")
    assert sorted(dev["patches"]) == sorted(r["patches"])
    for key in r["patches"]:
        if key != "signed_volume":
            assert np.array_equal(dev["patches"][key], r["patches"][key]), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_MESHES))
def test_device_integers_equal_the_reference(ctx, name):
    _, faces, r = case(name)
    dev = device(ctx, name)
    print("%s: %d faces, %d patches, %d loops, rounds %d, loop rounds %d" % (name, len(faces), dev.n_patches, dev.n_boundary_loops,
                                                                          dev.rounds, dev.loop_rounds))
    _assert_equal_integers(dev, r, name)
    assert 1 <= dev.rounds <= len(faces) and dev.loop_rounds <= 3 * len(faces)  # below the caps of F + 1 and 3 F + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube_all_reversed", "nested_spheres", "messy700", "moebius"])
def test_device_integers_without_the_outward_rule(ctx, name):
    _, _, r = case(name, outward=False)
    dev = device(ctx, name, outward=False)
    _assert_equal_integers(dev, r, name)
    assert np.all(dev.patches["signed_volume"] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tetrahedron", "cube_one_reversed", "cube_all_reversed", "torus", "nested_spheres", "blob700_reversed",
                                  "blob5000_reversed"])
def test_device_signed_volume(ctx, name):
    """Closed patches with |V| far from 0: at least 1e-3 of the sum of the terms' magnitudes, nine orders above the bound."""
    _, _, r = case(name)
    dev = device(ctx, name)
    want, got, mag = r["patches"]["signed_volume"], dev.patches["signed_volume"], r["volume_terms"]
    print("%s: V %s, |device - reference| / terms %s" % (name, want.tolist(), (np.abs(got - want) / mag).tolist()))
    assert np.all(want > 1e-3 * mag)
    assert np.all(np.abs(got - want) <= 1e-12 * mag)
    assert np.array_equal(np.sign(got), np.sign(want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["messy700", "ribbon_open", "ribbon_band", "nested_spheres"])
def test_two_calls_give_the_same_bits(ctx, name):
    from pyfocusr_amd import mesh_topology

    pts, faces, _ = case(name)
    a, b = device(ctx, name), mesh_topology((pts, faces), ctx=ctx)
    for field in sorted(a):
        if field == "patches":
            for key in sorted(a[field]):
                assert np.asarray(a[field][key]).tobytes() == np.asarray(b[field][key]).tobytes(), key
        elif field not in ("device_ms", "rounds", "loop_rounds"):
            assert np.asarray(a[field]).tobytes() == np.asarray(b[field]).tobytes(), field


@pytest.mark.gpu
def test_counts_agree_with_the_other_two_counters(ctx):
    from pyfocusr_amd import _hip

    pts, faces, _ = case("messy700")
    dev = device(ctx, "messy700")
    mine = [dev.n_edges, dev.n_boundary_edges, dev.n_nonmanifold_edges, dev.n_inconsistent_edges]
    assert ctx.curvatures(pts, faces)["topology"][:4].tolist() == mine
    surface = _hip.DeviceSurface(pts, faces, ctx=ctx)
    try:
        assert surface._prepare_signed().tolist() == mine
    finally:
        surface.close()


@pytest.mark.gpu
def test_library_refuses_bad_input_and_stays_usable(ctx):
    from pyfocusr_amd import _hip

    pts, faces = ref.tetrahedron()
    for bad in (faces + 1, faces - 1):
        with pytest.raises(_hip.PfError) as e:
            ctx.mesh_topology(len(pts), bad, points=pts)
        assert e.value.code == -1 and "references vertex" in str(e.value)
    twice = np.concatenate([faces, [[0, 1, 2], [2, 3, 2], [1, 1, 0]]]).astype(np.int32)
    with pytest.raises(_hip.PfError) as e:
        ctx.mesh_topology(len(pts), twice, points=pts)
    assert e.value.code == _hip.PF_E_DEGENERATE and "face 5 repeats a vertex" in str(e.value)
    flat = np.concatenate([pts, [pts[1]]])  # a zero-area face of three distinct indices is legal
    out = ctx.mesh_topology(len(flat), np.concatenate([faces, [[0, 1, 4]]]).astype(np.int32), points=flat)
    assert out["report"][4] == 2
    again = ctx.mesh_topology(len(pts), faces, points=pts)
    assert again["report"].tolist()[:6] == [6, 0, 0, 0, 1, 0] and not again["flip"].any()


@pytest.mark.gpu
def test_repaired_blob_gives_the_clean_blob_signed_distances(ctx):
    from pyfocusr_amd import PolyMesh, orient_faces, signed_point_to_surface_distances

    pts, faces, clean, which = _reversed_blob(700, 1, 40, 7)
    queries = np.random.default_rng(5).normal(scale=25.0, size=(300, 3))
    broken = PolyMesh(pts, faces)
    with pytest.raises(ValueError, match="consistently oriented"):
        signed_point_to_surface_distances(queries, broken, ctx=ctx)
    fixed, topo = orient_faces(broken, ctx=ctx)
    assert np.array_equal(np.flatnonzero(topo.flip), which) and np.array_equal(fixed.faces, clean)
    sd, face = signed_point_to_surface_distances(queries, fixed, ctx=ctx)
    sd_clean, face_clean = signed_point_to_surface_distances(queries, PolyMesh(pts, clean), ctx=ctx)
    assert np.array_equal(sd, sd_clean) and np.array_equal(face, face_clean)
    assert np.any(sd < 0.0) and np.any(sd > 0.0)


@pytest.mark.gpu
def test_repaired_blob_gives_the_clean_blob_graph(ctx):
    from pyfocusr_amd import Graph, PolyMesh, orient_faces

    pts, faces, clean, _ = _reversed_blob(700, 1, 40, 7)

    def graph(f):
        return Graph(PolyMesh(pts, f), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)

    broken = graph(faces)
    assert broken.device.n_oneway > 0
    fixed = graph(orient_faces(PolyMesh(pts, faces), ctx=ctx)[0].faces)
    want = graph(clean)
    assert fixed.device.n_oneway == 0 and want.device.n_oneway == 0
    got, exp = fixed.device.download(), want.device.download()
    for key in ("w", "rowptr", "colidx"):
        assert np.array_equal(got[key], exp[key]), key
