"""Mesh smoothing (`pf_smoother_*`, `pyfocusr_amd.smoothing`).

CPU: the declaration and the binding, the public names, argument errors before the library is loaded, and the numpy
reference `_smoothing_ref` against what smoothing is for: a voxel staircase loses its steps and keeps its volume under
Taubin's scheme, loses volume under the plain Laplacian, stays inside the clamp, keeps a fixed rim, smooths a rim along
itself, and leaves a constant field alone.  GPU: the device against that reference bit for bit - only + - x / and
comparisons occur, every sum has one order, and the volumes' tree is the one map quality and the shape models share -
on the smallest meshes that reach each path; two calls and a reused handle give the same bytes; the pool may hold
anything; the public functions."""
import os
import re

import numpy as np
import pytest

import _curvature_ref as cref
import _remesh_ref as rref
import _smoothing_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blob(n, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    return m.points, m.faces


def _messy():
    from pyfocusr_amd.meshgen import messy_blob_mesh

    m = messy_blob_mesh(700)
    return m.points, m.faces


def _repeated():
    """blob700 with two more faces that repeat a vertex: (a, a, b) brings the edge {a, b} of no triangle of the blob."""
    pts, faces = _blob(700, 1)
    far = int(np.argmax(np.linalg.norm(pts - pts[0], axis=1)))
    return pts, np.concatenate([faces, [[0, 0, far], [5, 5, 5]]]).astype(np.int32)


_MESHES = {
    "tetrahedron": lambda: cref.tetrahedron(),               # n = 4: the fewest index bits
    "blob700": lambda: _blob(700, 1),                        # n is not a block multiple
    "cylinder": lambda: cref.open_cylinder(),                # boundary runs
    "cone": lambda: cref.cone_fan(200),                      # one row of 200
    "messy700": _messy,                                      # non-manifold, one-way, duplicated directed edges, unreferenced
    "zero_area": lambda: cref.with_zero_area_triangle(*_blob(700, 1)),
    "grid": lambda: rref.grid_mesh(9, 7),                    # a mesh with a rim
    "sphere_mask": lambda: ref.sphere_mask_mesh()[:2],       # anisotropic spacing
    "repeated": _repeated,                                   # faces that repeat a vertex
    "no_edge": lambda: (np.eye(3), np.array([[1, 1, 1]], dtype=np.int32)),  # not one proper edge
}
_mesh_cache, _adj_cache, _run_cache = {}, {}, {}


def mesh(name):
    if name not in _mesh_cache:
        pts, faces = _MESHES[name]()
        pts, faces = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32)
        pts.setflags(write=False), faces.setflags(write=False)
        _mesh_cache[name] = (pts, faces)
    return _mesh_cache[name]


def pinned_of(name, pinned):
    """None, or every fifth vertex of the mesh."""
    if not pinned:
        return None
    mask = np.zeros(len(mesh(name)[0]), dtype=bool)
    mask[2::5] = True
    return mask


def adjacency(name, weights, boundary, pinned=False):
    """The reference adjacency of a case, computed once and never changed."""
    key = (name, weights, boundary, pinned)
    if key not in _adj_cache:
        pts, faces = mesh(name)
        _adj_cache[key] = ref.adjacency(pts, faces, weights, boundary, pinned_of(name, pinned))
    return _adj_cache[key]


def field(name, ncols):
    """A fixed field of ncols columns on the mesh's vertices, about the size of its coordinates."""
    return np.random.default_rng(ncols).uniform(-1.0, 1.0, size=(len(mesh(name)[0]), ncols))


def reference_run(name, weights, boundary, pinned, factors, clamp_every, bound, ncols):
    """(result, stats or None) of the reference for a case; ncols None: the mesh's own points."""
    key = (name, weights, boundary, pinned, tuple(factors), clamp_every, None if bound is None else tuple(bound), ncols)
    if key not in _run_cache:
        pts, faces = mesh(name)
        x0 = pts if ncols is None else field(name, ncols)
        x = ref.run(adjacency(name, weights, boundary, pinned), x0, factors, clamp_every, bound)
        _run_cache[key] = (x, ref.stats(x0, x, faces) if ncols is None else None)
    return _run_cache[key]


# ------------------------------------------------------------------------------ CPU
def test_smoother_entry_points_are_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, arity in (("pf_smoother_create", 9), ("pf_smoother_info", 2), ("pf_smoother_adjacency", 5), ("pf_smoother_run", 10),
                        ("pf_smoother_free", 1)):
        m = re.search(r"(?:int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity
        assert len(_hip.SIGNATURES[name][1]) == arity
    assert issubclass(_hip.DeviceSmoother, _hip._Handle) and _hip.DeviceSmoother._free == "pf_smoother_free"
    for word, code in (("PF_SMOOTH_UNIFORM", _hip.SMOOTH_WEIGHTS["uniform"]), ("PF_SMOOTH_COTANGENT", _hip.SMOOTH_WEIGHTS["cotangent"]),
                       ("PF_SMOOTH_FREE", _hip.SMOOTH_BOUNDARY["free"]), ("PF_SMOOTH_FIXED", _hip.SMOOTH_BOUNDARY["fixed"]),
                       ("PF_SMOOTH_CURVE", _hip.SMOOTH_BOUNDARY["curve"])):
        assert re.search(r"\b%s = %d\b" % (word, code), header), word


def test_public_names_exist():
    import pyfocusr_amd
    from pyfocusr_amd import smoothing

    for name in ("MeshSmoother", "smooth_mesh", "smooth_mask_mesh", "smooth_point_data"):
        assert callable(getattr(pyfocusr_amd, name)) and getattr(pyfocusr_amd, name) is getattr(smoothing, name)
    for name in ("smooth_points", "smooth_values", "adjacency", "info"):
        assert hasattr(smoothing.MeshSmoother, name)


def test_argument_errors_before_the_library_is_loaded(monkeypatch):
    from pyfocusr_amd import PolyMesh, _hip, smoothing

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    pts, faces = cref.tetrahedron()
    quads = np.array([[0, 1, 2, 3]], dtype=np.int32)
    nan_pts = pts.copy()
    nan_pts[2, 1] = np.nan
    for p, f in [(pts, quads), (nan_pts, faces), (pts, faces + 1), (pts, faces.astype(np.float64)), (pts[:0], faces)]:
        for call in (smoothing.smooth_mesh, smoothing.MeshSmoother, lambda m: smoothing.smooth_mask_mesh(m, 1.0),
                     lambda m: smoothing.smooth_point_data(m, np.zeros(len(pts)))):
            with pytest.raises(ValueError):
                call((p, f))
    with pytest.raises(ValueError):
        smoothing.smooth_mesh(PolyMesh(pts, quads))
    good = (pts, faces)
    for pass_band in (2.0, 2.5, -1.0, 0.0):  # mu = inf, 2, -1/3 (|mu| < lam), -1/2 (|mu| = lam)
        with pytest.raises(ValueError, match="mu"):
            smoothing.smooth_mesh(good, lam=0.5, pass_band=pass_band)
    assert smoothing.taubin_mu(0.5, 0.1) == 1.0 / (0.1 - 1.0 / 0.5)
    for kw in (dict(method="implicit"), dict(lam=0.0), dict(lam=np.inf), dict(iterations=-1), dict(iterations=2.5),
               dict(pass_band=np.nan), dict(weights="mean"), dict(boundary="open"), dict(pinned=np.zeros(3, dtype=bool)),
               dict(pinned=np.zeros((4, 1), dtype=bool)), dict(pinned=np.zeros(4)), dict(max_displacement=-0.1),
               dict(max_displacement=[0.1, 0.2]), dict(max_displacement=np.nan)):
        with pytest.raises(ValueError):
            smoothing.smooth_mesh(good, **kw)
    with pytest.raises(ValueError):
        smoothing.smooth_mask_mesh(good, 1.0, max_displacement=0.2)
    for spacing in (0.0, -1.0, (1.0, 1.0), np.nan):
        with pytest.raises(ValueError):
            smoothing.smooth_mask_mesh(good, spacing)
    for values in (np.zeros((4, 33)), np.zeros(3), np.zeros((4, 2, 2)), np.zeros((4, 0)), np.full(4, np.nan)):
        with pytest.raises(ValueError):
            smoothing.smooth_point_data(good, values)
    with pytest.raises(ValueError):
        smoothing.smooth_point_data(good, np.zeros(4), method="taubin", pass_band=2.5)
    with pytest.raises(ValueError):
        smoothing.smooth_point_data(good, np.zeros((4, 2)), max_change=[0.1, 0.2, 0.3])
    # preserve_volume: an open mesh, and a closed one with a face turned over
    with pytest.raises(ValueError, match="closed"):
        smoothing.smooth_mesh(cref.open_cylinder(), preserve_volume=True)
    turned = faces.copy()
    turned[1] = turned[1, ::-1]
    with pytest.raises(ValueError, match="closed"):
        smoothing.smooth_mesh((pts, turned), preserve_volume=True)
    assert smoothing._closed_and_oriented(faces) and smoothing._closed_and_oriented(_blob(700, 1)[1])


def test_reference_adjacency_on_small_meshes():
    pts, faces = cref.tetrahedron()
    a = ref.adjacency(pts, faces, "cotangent", "fixed")
    assert np.array_equal(a["rowptr"], [0, 3, 6, 9, 12]) and np.array_equal(a["col"], [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2])
    assert np.array_equal(a["counts"], [6, 0, 0, 12, 3, 4]) and np.all(a["kind"] == ref.MOVABLE)
    np.testing.assert_allclose(a["w"], 2.0 * 0.5 / np.sqrt(3.0), rtol=1e-14)  # two angles of 60 degrees opposite every edge
    a = adjacency("cone", "uniform", "fixed", True)
    assert a["rowptr"][1] == 200 and np.array_equal(a["col"][:200], 1 + np.arange(200))
    assert np.array_equal(a["counts"][:5], [400, 200, 0, 800, 200])
    assert a["kind"][0] == ref.MOVABLE and np.all(a["kind"][1:] & ref.BOUNDARY) and a["kind"][2] == ref.BOUNDARY | ref.PINNED
    assert a["counts"][5] == 1
    a = adjacency("repeated", "uniform", "free")
    b = adjacency("blob700", "uniform", "free")
    assert a["counts"][0] == b["counts"][0] + 1 and a["counts"][1] == 0  # (0, 0, far): one more edge, there and back ...
    assert a["counts"][3] == b["counts"][3] + 2                          # ... and (5, 5, 5) brings none
    a = adjacency("no_edge", "cotangent", "curve")
    assert np.array_equal(a["counts"], [0, 0, 0, 0, 0, 0]) and np.all(a["kind"] == 0) and np.all(a["rowptr"] == 0)
    a = adjacency("messy700", "uniform", "free")
    assert a["counts"][2] > 0 and np.any(np.diff(a["rowptr"]) == 0)  # non-manifold edges, and vertices in no face


def test_reference_takes_the_staircase_out_of_a_sphere_mask():
    pts, faces, centre = ref.sphere_mask_mesh()
    assert len(pts) == 4182 and len(faces) == 8360 and ref.volume(pts, faces) > 0.0
    start = ref.normal_deviation(pts, faces, centre)
    x, st = ref.smooth(pts, faces, 20, "taubin", 0.5, 0.1)
    after = ref.normal_deviation(x, faces, centre)
    print("normal deviation %.2f -> %.2f degrees (ratio %.4f), volume ratio %.6f" % (start, after, after / start, st[1] / st[0]))
    assert after <= 0.6 * start           # measured 35.98 -> 19.81 degrees: 0.5507
    assert abs(st[1] / st[0] - 1.0) <= 0.01  # measured 1.003879
    assert st[0] == ref.volume(pts, faces) and st[1] == ref.volume(x, faces)
    y, sl = ref.smooth(pts, faces, 20, "laplacian", 0.5)
    print("plain Laplacian: volume ratio %.6f" % (sl[1] / sl[0]))
    assert sl[1] / sl[0] < 0.95           # measured 0.928341: the shrinkage Taubin's second sweep undoes


def test_reference_clamp_keeps_every_vertex_in_its_half_voxel():
    pts, faces, _ = ref.sphere_mask_mesh()
    spacing = np.array(ref.SPHERE_SPACING)
    x, st = ref.smooth(pts, faces, 20, max_displacement=spacing / 2.0)
    assert np.all(np.abs(x - pts) <= spacing / 2.0) and st[5] == np.max(np.abs(x - pts))
    c = spacing / 8.0
    y, _ = ref.smooth(pts, faces, 20, max_displacement=c)
    assert np.all(y >= pts - c) and np.all(y <= pts + c)
    on = (y == pts - c) | (y == pts + c)
    print("bound spacing / 8: %d components sit on it" % on.sum())
    assert on.any() and not np.array_equal(y, ref.smooth(pts, faces, 20)[0])


def test_reference_boundary_modes_on_an_open_cylinder():
    n_around = 48
    pts, faces = mesh("cylinder")
    rim = np.zeros(len(pts), dtype=bool)
    rim[:n_around] = rim[-n_around:] = True
    for weights in ref.WEIGHTS:
        assert np.array_equal((adjacency("cylinder", weights, "fixed")["kind"] & ref.BOUNDARY) != 0, rim)
        fixed = ref.smooth(pts, faces, 5, weights=weights, boundary="fixed")[0]
        assert fixed[rim].tobytes() == pts[rim].tobytes() and not np.array_equal(fixed[~rim], pts[~rim])
        free = ref.smooth(pts, faces, 5, "laplacian", weights=weights, boundary="free")[0]
        assert np.all(free[:n_around, 2] > pts[:n_around, 2])  # pulled towards the inside of the tube
    # curve: one Laplacian sweep takes a rim vertex to the midpoint-ward point between its two rim neighbours
    adj = adjacency("cylinder", "cotangent", "curve")
    x = ref.run(adj, pts, [0.5])
    for v in (0, 7, n_around - 1, len(pts) - 1):
        ring = v - v % n_around
        a, b = ring + (v - 1) % n_around, ring + (v + 1) % n_around
        assert x[v].tobytes() == (pts[v] + 0.5 * ((pts[a] + pts[b]) / 2.0 - pts[v])).tobytes()
        assert not np.array_equal(x[v], pts[v]) and x[v, 2] == pts[v, 2]  # it moves, and stays in its rim's plane
        lo, hi = np.minimum(np.minimum(pts[a], pts[b]), pts[v]), np.maximum(np.maximum(pts[a], pts[b]), pts[v])
        assert np.all(x[v] >= lo) and np.all(x[v] <= hi)  # within what it and its two rim neighbours span


def test_reference_constant_field_is_a_fixed_point():
    for name, weights, boundary in (("blob700", "uniform", "free"), ("messy700", "cotangent", "free"), ("cylinder", "cotangent", "curve")):
        adj = adjacency(name, weights, boundary)
        const = np.full((len(mesh(name)[0]), 2), [0.375, -12.0])  # exactly representable: s / W gives the value back
        out = ref.run(adj, const, ref.factors(6, "taubin")[0])
        if weights == "uniform":
            assert out.tobytes() == const.tobytes()
        else:  # sum(w c) / sum(w) rounds: within an ulp or two per sweep
            np.testing.assert_allclose(out, const, rtol=1e-14)


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


def smoother(ctx, name, weights="uniform", boundary="fixed", pinned=False):
    from pyfocusr_amd import MeshSmoother

    return MeshSmoother(mesh(name), weights=weights, boundary=boundary, pinned=pinned_of(name, pinned), ctx=ctx)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.ravel().view(np.uint8 if got.itemsize == 1 else "u%d" % got.itemsize)
                             != want.ravel().view(np.uint8 if want.itemsize == 1 else "u%d" % want.itemsize))
        raise AssertionError("%s: %d of %d entries differ, first at %d: %r against %r"
                             % (what, len(bad), got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize("weights", ref.WEIGHTS)
@pytest.mark.parametrize("name", sorted(_MESHES))
def test_device_adjacency_equals_the_reference(ctx, name, weights):
    for boundary, pinned in (("fixed", False), ("free", True), ("curve", True)):
        want = adjacency(name, weights, boundary, pinned)
        with smoother(ctx, name, weights, boundary, pinned) as sm:
            rowptr, col, w, kind = sm.adjacency()
            counts = sm.info
        what = "%s %s %s" % (name, weights, boundary)
        print(what, dict(counts))
        assert [counts[k] for k in ("edges", "boundary_edges", "non_manifold_edges", "entries", "largest_row", "movable_vertices")] \
            == want["counts"].tolist(), what
        same_bits(rowptr, want["rowptr"], what + " rowptr")
        same_bits(col, want["col"], what + " col")
        same_bits(w, want["w"], what + " w")
        same_bits(kind, want["kind"], what + " kind")


def _device_points(sm, factors, clamp_every=1, bound=None):
    out, st, _ = sm._device.run(None, np.ascontiguousarray(factors, dtype=np.float64), clamp_every,
                                None if bound is None else np.ascontiguousarray(bound, dtype=np.float64), True)
    return out, st


@pytest.mark.gpu
@pytest.mark.parametrize("n_sweeps", [0, 1, 2, 3, 40])
@pytest.mark.parametrize("method", ["laplacian", "taubin"])
def test_device_sweep_counts_equal_the_reference(ctx, method, n_sweeps):
    """Both parities of the ping-pong, and none: n_sweeps = 0 returns the input's bits."""
    mu = 1.0 / (0.1 - 1.0 / 0.5)
    factors = [0.5 if method == "laplacian" or s % 2 == 0 else mu for s in range(n_sweeps)]
    for name, weights, boundary in (("blob700", "uniform", "fixed"), ("cylinder", "cotangent", "curve")):
        want, want_stats = reference_run(name, weights, boundary, False, factors, 1, None, None)
        with smoother(ctx, name, weights, boundary) as sm:
            got, st = _device_points(sm, factors)
        same_bits(got, want, "%s %s %d sweeps" % (name, method, n_sweeps))
        same_bits(st, want_stats, "%s %s %d sweeps: stats" % (name, method, n_sweeps))
        if n_sweeps == 0:
            same_bits(got, mesh(name)[0], name + " untouched")


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", ref.MODES)
@pytest.mark.parametrize("weights", ref.WEIGHTS)
@pytest.mark.parametrize("name", sorted(_MESHES))
def test_device_points_equal_the_reference(ctx, name, weights, boundary):
    """Three Taubin iterations of the mesh's own points, then the same with a pinned subset and a clamp that binds; the
    stats with both volumes."""
    factors = ref.factors(3, "taubin")[0]
    pts = mesh(name)[0]
    with smoother(ctx, name, weights, boundary) as sm:
        got, st = _device_points(sm, factors)
    want, want_stats = reference_run(name, weights, boundary, False, factors, 1, None, None)
    what = "%s %s %s" % (name, weights, boundary)
    print("%s: volumes %r -> %r, largest move %r" % (what, st[0], st[1], st[5]))
    same_bits(got, want, what)
    same_bits(st, want_stats, what + " stats")
    bound = 0.25 * np.max(np.abs(want - pts), axis=0)  # a quarter of the free run's largest move per axis: it binds
    want_c, want_cs = reference_run(name, weights, boundary, True, factors, 2, bound, None)
    with smoother(ctx, name, weights, boundary, pinned=True) as sm:
        got_c, st_c = _device_points(sm, factors, 2, bound)
    same_bits(got_c, want_c, what + " pinned, clamped")
    same_bits(st_c, want_cs, what + " pinned, clamped: stats")
    pin = pinned_of(name, True)
    same_bits(got_c[pin], pts[pin], what + " pinned vertices")
    if bound.max() > 0.0:
        assert np.all(got_c >= pts - bound) and np.all(got_c <= pts + bound)  # the bounds as the clamp forms them
        assert np.any((got_c == pts - bound) | (got_c == pts + bound)), what + ": the clamp does not bind"


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", [1, 3, 5, 32])
@pytest.mark.parametrize("weights", ref.WEIGHTS)
def test_device_values_equal_the_reference(ctx, weights, ncols):
    """Fields of 1, 3, 5 and 32 columns (3 takes the points' kernel, the others the generic one), Laplacian and Taubin,
    with and without a clamp."""
    lap, tau = ref.factors(3, "laplacian")[0], ref.factors(2, "taubin")[0]
    bound = np.linspace(0.05, 0.4, ncols)
    for name, boundary, pinned in (("blob700", "free", False), ("cylinder", "curve", True), ("cone", "fixed", False), ("messy700", "free", True)):
        values = field(name, ncols)
        with smoother(ctx, name, weights, boundary, pinned) as sm:
            for factors, every, c in ((lap, 1, None), (tau, 2, bound), (lap, 3, bound)):
                got, st, _ = sm._device.run(values, factors, every, None if c is None else np.ascontiguousarray(c), False)
                want, _ = reference_run(name, weights, boundary, pinned, factors, every, c, ncols)
                same_bits(got, want, "%s %s %s %d columns, clamp every %d" % (name, weights, boundary, ncols, every))
                assert st is None


@pytest.mark.gpu
def test_two_calls_and_a_reused_handle_give_the_same_bytes(ctx):
    factors = ref.factors(4, "taubin")[0]
    values = field("messy700", 5)
    for weights, boundary in (("uniform", "fixed"), ("cotangent", "curve")):
        with smoother(ctx, "messy700", weights, boundary) as one:
            a_pts, a_st = _device_points(one, factors)
            b_pts, b_st = _device_points(one, factors)              # one handle, twice
            a_val = one.smooth_values(values, 3)                     # ... and for values after points
            c_pts, c_st = _device_points(one, factors)              # ... and points again
        with smoother(ctx, "messy700", weights, boundary) as fresh:
            d_val = fresh.smooth_values(values, 3)                   # values first
            d_pts, d_st = _device_points(fresh, factors)
        for other in (b_pts, c_pts, d_pts):
            same_bits(other, a_pts, "points")
        for other in (b_st, c_st, d_st):
            same_bits(other, a_st, "stats")
        same_bits(d_val, a_val, "values")
        same_bits(a_val, reference_run("messy700", weights, boundary, False, ref.factors(3, "laplacian")[0], 1, None, 5)[0], "values")


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [1, 2])
def test_poisoned_pool_changes_nothing(ctx, fill):
    from pyfocusr_amd import _hip

    factors = ref.factors(3, "taubin")[0]
    want, want_stats = reference_run("messy700", "cotangent", "curve", False, factors, 1, None, None)
    want_adj = adjacency("messy700", "cotangent", "curve")
    values = field("messy700", 5)
    want_val, _ = reference_run("messy700", "cotangent", "curve", False, factors, 1, None, 5)
    _hip.pool_poison(fill)
    try:
        with smoother(ctx, "messy700", "cotangent", "curve") as sm:
            rowptr, col, w, kind = sm.adjacency()
            got, st = _device_points(sm, factors)
            got_val, _, _ = sm._device.run(values, factors, 1, None, False)
            counts = sm._device.counts.copy()
    finally:
        _hip.pool_poison(0)
    same_bits(counts, want_adj["counts"], "counts")
    for g, k in ((rowptr, "rowptr"), (col, "col"), (w, "w"), (kind, "kind")):
        same_bits(g, want_adj[k], k)
    same_bits(got, want, "points")
    same_bits(st, want_stats, "stats")
    same_bits(got_val, want_val, "values")


@pytest.mark.gpu
def test_library_refuses_a_bad_index_and_bad_arguments(ctx):
    from pyfocusr_amd import _hip

    pts, faces = cref.tetrahedron()
    for bad in (faces + 1, faces - 1):
        with pytest.raises(_hip.PfError) as e:
            _hip.DeviceSmoother(pts, bad, ctx=ctx)  # (MeshSmoother would have refused it first)
        assert e.value.code == -1 and "references vertex" in str(e.value)
    for kw in (dict(weights=2), dict(boundary=3)):
        with pytest.raises(_hip.PfError) as e:
            _hip.DeviceSmoother(pts, faces, ctx=ctx, **kw)
        assert e.value.code == -1
    with _hip.DeviceSmoother(pts, faces, ctx=ctx) as sm:
        half = np.array([0.5])
        for values, factors, every, clamp, stats in ((np.zeros((4, 33)), half, 1, None, False), (np.zeros((4, 2)), half, 1, None, True),
                                                     (None, np.array([np.nan]), 1, None, False), (None, half, 0, np.ones(3), False),
                                                     (None, half, 1, np.array([0.1, -0.1, 0.1]), False)):
            with pytest.raises(_hip.PfError) as e:
                sm.run(values, factors, every, clamp, stats)
            assert e.value.code == -1


@pytest.mark.gpu
def test_smooth_mesh_carries_the_mesh_over_and_preserves_volume(ctx):
    from pyfocusr_amd import PolyMesh, smooth_mesh, smooth_point_data

    pts, faces = mesh("blob700")
    height = pts[:, 2].copy()
    source = PolyMesh(pts.copy(), faces.copy(), [("height", height)])
    out, info = smooth_mesh(source, iterations=5, return_info=True, ctx=ctx)
    assert isinstance(out, PolyMesh) and out is not source
    assert source.points.tobytes() == pts.tobytes() and source.faces.tobytes() == faces.tobytes()  # the input is untouched
    assert np.array_equal(out.faces, faces) and out.faces is not source.faces
    assert [n for n, _ in out.point_data] == ["height"] and np.array_equal(dict(out.point_data)["height"], height)
    want, want_stats = ref.smooth(pts, faces, 5)
    same_bits(out.points, want, "smooth_mesh")
    assert info.mu == 1.0 / (0.1 - 2.0) and info.sweeps == 10 and info.edges == 3 * len(faces) // 2 and info.device_ms > 0.0
    assert (info.volume_in, info.volume_out, info.max_displacement) == (want_stats[0], want_stats[1], want_stats[5])
    same_bits(info.mean, want_stats[2:5], "mean")
    pair = smooth_mesh((pts, faces), iterations=5, ctx=ctx)
    assert isinstance(pair, tuple) and pair[0].tobytes() == want.tobytes() and np.array_equal(pair[1], faces)
    # the plain Laplacian shrinks; preserve_volume brings the volume back about the vertex mean
    shrunk, info = smooth_mesh((pts, faces), iterations=10, method="laplacian", return_info=True, ctx=ctx)
    assert info.volume_out < 0.99 * info.volume_in
    kept, info = smooth_mesh((pts, faces), iterations=10, method="laplacian", preserve_volume=True, return_info=True, ctx=ctx)
    v_in, v_out = ref.volume(pts, faces), ref.volume(kept[0], faces)
    print("preserve_volume: scale %.6f, V_out / V_in - 1 = %.3e" % (info.scale, v_out / v_in - 1.0))
    assert abs(v_out - v_in) <= 1e-12 * abs(v_in) and info.scale > 1.0
    same_bits(kept[0], info.mean + info.scale * (shrunk[0] - info.mean), "the rescaling")
    # a field on the fixed mesh
    smooth = smooth_point_data(source, height, iterations=4, ctx=ctx)
    assert smooth.shape == height.shape
    same_bits(smooth, ref.run(adjacency("blob700", "uniform", "free"), height[:, None], [0.5] * 4)[:, 0], "smooth_point_data")
    const = smooth_point_data(source, np.full((len(pts), 2), [0.375, -12.0]), iterations=6, method="taubin", ctx=ctx)
    assert np.all(const == [0.375, -12.0])  # a constant field is a fixed point


@pytest.mark.gpu
def test_smooth_mask_mesh_equals_the_reference(ctx):
    from pyfocusr_amd import smooth_mask_mesh

    pts, faces = mesh("sphere_mask")
    spacing = np.array(ref.SPHERE_SPACING)
    for divisor in (2.0, 8.0):  # spacing / 2 is smooth_mask_mesh itself; spacing / 8 binds
        want, want_stats = ref.smooth(pts, faces, 20, max_displacement=spacing / divisor)
        (got, _), info = smooth_mask_mesh((pts, faces), spacing * (2.0 / divisor), iterations=20, return_info=True, ctx=ctx)
        same_bits(got, want, "smooth_mask_mesh, spacing / %g" % divisor)
        assert info.max_displacement == want_stats[5]
        assert np.all(got >= pts - spacing / divisor) and np.all(got <= pts + spacing / divisor)
        assert (info.volume_in, info.volume_out) == (want_stats[0], want_stats[1])
