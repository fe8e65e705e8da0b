"""Isosurface extraction (`pf_isosurface_*`, `pyfocusr_amd.isosurface`).

CPU: the numpy definition `_isosurface_ref.isosurface_ref` on shapes with known answers (closed, consistently oriented,
vertex / face counts, Euler characteristic, components, positive signed volume), the coverage of all 84 non-trivial
(tetrahedron, case) pairs by the random field the GPU parity test uses, `inside="above"`, `closed=True` and the mask
case over the reference, argument errors before the library is loaded, the declarations.  GPU: points, faces,
vertex_key and face_cell equal to the reference bit for bit on rows that cross, end on and start a 64-bit word, on ties
and on a random sweep; two calls bit for bit; `mesh_topology` of the result; the four runs of the pool hygiene; and the
chains the feature exists for: offset surfaces and a re-meshed open blob."""
import os
import re

import numpy as np
import pytest

import _isosurface_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _integer_field():
    return np.random.default_rng(11).integers(-1, 2, size=(7, 8, 9)).astype(np.float64)


def _one_corner():
    v = np.ones((2, 2, 2))
    v[1, 0, 1] = -2.0
    return v


# name -> (values, level, spacing, origin)
_FIELDS = {
    "sphere": lambda: (ref.sphere_field(), 0.0, (0.5, 1.0, 2.0), (-1.0, 2.0, 0.25)),
    "torus": lambda: (ref.torus_field(), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "one_voxel": lambda: (ref.one_voxel_field(), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "random": lambda: (ref.random_field(5), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "ties": lambda: (_integer_field(), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),       # values equal to the level: zero-area faces
    "one_corner": lambda: (_one_corner(), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),  # one cell
    "wave_130": lambda: (ref.wave_field((3, 4, 130)), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),  # a row crosses two word ends
    "wave_64": lambda: (ref.wave_field((3, 4, 64)), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),    # a row ends on a word
    "wave_65": lambda: (ref.wave_field((2, 3, 65)), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),    # a row starts a second word
    "outside": lambda: (np.ones((3, 3, 3)), 0.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
}
_cache = {}


def case(name):
    """(arguments, reference outputs, (tetrahedron, case) pairs hit) of a test field, computed once and never changed."""
    if name not in _cache:
        args = _FIELDS[name]()
        out = ref.isosurface_ref(*args, return_cases=True)
        for a in (args[0],) + out[:4]:
            a.setflags(write=False)
        _cache[name] = (args, out[:4], out[4])
    return _cache[name]


def _closed_and_outward(name, n_points, n_faces, euler, components=1):
    _, (pts, faces, key, cell), _ = case(name)
    assert (len(pts), len(faces)) == (n_points, n_faces)
    assert ref.is_closed(faces) and ref.is_consistent(faces)
    assert ref.euler_characteristic(len(pts), faces) == euler
    assert ref.n_components(len(pts), faces) == components
    assert ref.signed_volume(pts, faces) > 0.0
    assert np.all(np.diff(key) > 0) and np.all(np.diff(cell) >= 0)


# ------------------------------------------------------------------------------ CPU
def test_reference_sphere():
    _closed_and_outward("sphere", 608, 1212, 2)


def test_reference_torus():
    _closed_and_outward("torus", 1070, 2140, 0)


def test_reference_one_voxel():
    _closed_and_outward("one_voxel", 14, 24, 2)
    _, (pts, faces, _, _), _ = case("one_voxel")
    assert ref.signed_volume(pts, faces) == 0.5


def test_reference_random_field_covers_every_case():
    _, (pts, faces, _, _), hit = case("random")
    assert ref.is_closed(faces) and ref.is_consistent(faces) and ref.signed_volume(pts, faces) > 0.0
    assert ref.euler_characteristic(len(pts), faces) == -20
    assert hit == {(t, c) for t in range(6) for c in range(1, 15)}  # all 84: the parity test below covers the whole table


def test_reference_wave_counts_and_ties():
    _, (pts, faces, _, _), _ = case("wave_130")
    assert (len(pts), len(faces)) == (1415, 2126)
    _, (pts, faces, _, _), _ = case("ties")
    p = pts[faces]
    area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area2 == 0.0).any()  # zero-area faces are kept ...
    assert ref.is_consistent(faces)  # ... and the connectivity stays oriented
    _, (pts, faces, key, cell), _ = case("outside")
    assert pts.shape == (0, 3) and faces.shape == (0, 3) and key.shape == (0,) and cell.shape == (0,)


def test_case_table_is_derived():
    table = ref.case_table()
    assert [len(table[t][c]) for t in range(6) for c in (0, 15)] == [0] * 12
    for t in range(6):
        for c in range(1, 15):
            assert len(table[t][c]) == (2 if bin(c).count("1") == 2 else 1)
            # the complementary case cuts the same lattice edges; a lone triangle comes back reversed
            assert {e for tri in table[t][c] for e in tri} == {e for tri in table[t][15 - c] for e in tri}
            if len(table[t][c]) == 1:
                a, b = table[t][c][0], table[t][15 - c][0]
                assert b == (a[0], a[2], a[1])


def test_inside_above_is_the_negated_call():
    from pyfocusr_amd.isosurface import prepare_volume

    v = ref.sphere_field()
    above = ref.isosurface_ref(*prepare_volume(-v, 0.25, inside="above"))
    below = ref.isosurface_ref(v, -0.25)
    for a, b in zip(above, below):
        assert a.tobytes() == b.tobytes()
    assert ref.signed_volume(above[0], above[1]) > 0.0


def test_closed_caps_a_cut_surface():
    from pyfocusr_amd.isosurface import prepare_volume

    x, y, z = ref.grid((6, 7, 8))
    v = np.sqrt((x - 2.0) ** 2 + (y - 3.0) ** 2 + (z - 3.5) ** 2) - 3.2
    pts, faces, _, _ = ref.isosurface_ref(*prepare_volume(v, 0.0))
    assert not ref.is_closed(faces)
    values, level, spacing, origin = prepare_volume(v, 0.0, spacing=(1.0, 2.0, 3.0), origin=(1.0, 1.0, 1.0), closed=True)
    assert values.shape == (8, 9, 10) and np.array_equal(origin, [0.0, -1.0, -2.0])
    assert np.array_equal(values[1:-1, 1:-1, 1:-1], v) and values[0, 0, 0] == abs(v[0, 0, 0])
    pts, faces, _, _ = ref.isosurface_ref(values, level, spacing, origin)
    assert ref.is_closed(faces) and ref.is_consistent(faces) and ref.euler_characteristic(len(pts), faces) == 2


def _mask():
    mask = np.zeros((12, 8, 9), dtype=bool)
    mask[1:4, 1:4, 1:6] = True  # a 3 x 3 x 5 block
    mask[7:12, 5, 5] = True     # a bar of 5 voxels that reaches the border
    return mask


def test_mask_reference_volume_and_components():
    from pyfocusr_amd.isosurface import prepare_volume

    pts, faces, _, _ = ref.isosurface_ref(*prepare_volume(_mask().astype(np.float64), 0.5, inside="above", closed=True))
    assert ref.is_closed(faces) and ref.n_components(len(pts), faces) == 2
    assert ref.signed_volume(pts, faces) == 46.0


def test_isosurface_entry_points_are_declared_and_bound():
    import pyfocusr_amd
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, res, arity in (("pf_isosurface_create", "int", 12), ("pf_isosurface_fetch", "int", 5), ("pf_isosurface_free", "void", 1)):
        m = re.search(r"%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity
        assert len(_hip.SIGNATURES[name][1]) == arity
    assert callable(_hip.Context.isosurface) and _hip.DeviceIsosurface._free == "pf_isosurface_free"
    for name in ("isosurface", "mask_to_mesh", "signed_distance_volume", "voxel_remesh", "offset_surface"):
        assert callable(getattr(pyfocusr_amd, name))
    import sys

    assert "zero area" in sys.modules["pyfocusr_amd.isosurface"].__doc__  # (the function shadows the module's name)


def test_argument_errors_come_before_the_library():
    from pyfocusr_amd.isosurface import isosurface, mask_to_mesh, signed_distance_volume

    good = ref.sphere_field()
    with pytest.raises(ValueError, match="3|dimensions"):
        isosurface(good[0])  # wrong rank
    with pytest.raises(ValueError, match="at least 2"):
        isosurface(good[:, :1, :])  # an extent of 1
    bad = good.copy()
    bad[2, 3, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        isosurface(bad)
    with pytest.raises(ValueError, match="inside"):
        isosurface(good, inside="under")
    with pytest.raises(ValueError, match="finite"):
        isosurface(good, level=np.inf)
    with pytest.raises(ValueError, match="spacing"):
        isosurface(good, spacing=(1.0, 2.0))
    with pytest.raises(ValueError, match="dimensions"):
        mask_to_mesh(np.zeros((4, 4), dtype=bool))
    tri = (np.eye(3), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="exactly one"):
        signed_distance_volume(tri)
    with pytest.raises(ValueError, match="exactly one"):
        signed_distance_volume(tri, spacing=0.1, shape=(8, 8, 8))
    with pytest.raises(ValueError, match="positive"):
        signed_distance_volume(tri, spacing=-0.1)


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def _assert_equal(raw, want):
    pts, faces, key, cell = want
    assert raw["points"].dtype == np.float64 and raw["faces"].dtype == np.int32
    assert raw["vertex_key"].dtype == np.int64 and raw["face_cell"].dtype == np.int32
    assert raw["points"].shape == pts.shape and raw["faces"].shape == faces.shape
    assert np.array_equal(raw["vertex_key"], key)
    assert np.array_equal(raw["face_cell"], cell)
    assert np.array_equal(raw["faces"], faces)
    assert np.array_equal(raw["points"], pts) and raw["points"].tobytes() == pts.tobytes()  # the bits, signs of zero too
    assert tuple(raw["report"][:2]) == (len(pts), len(faces)) and raw["report"][2] == len(np.unique(cell))
    assert np.all(raw["report"][5:] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_FIELDS))
def test_device_equals_the_reference(ctx, name):
    args, want, _ = case(name)
    raw = ctx.isosurface(*args)
    _assert_equal(raw, want)
    nx, ny, nz = args[0].shape
    assert tuple(raw["report"][3:5]) == (nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1))
    assert raw["device_ms"] > 0.0


@pytest.mark.gpu
def test_device_equals_the_reference_on_a_random_sweep(ctx):
    rng = np.random.default_rng(2024)
    for _ in range(20):
        shape = tuple(int(n) for n in rng.integers(2, 13, size=3))
        values = rng.standard_normal(shape)
        level = float(rng.uniform(-1.0, 1.0))
        spacing, origin = rng.uniform(0.25, 2.0, size=3), rng.uniform(-3.0, 3.0, size=3)
        _assert_equal(ctx.isosurface(values, level, spacing, origin), ref.isosurface_ref(values, level, spacing, origin))


@pytest.mark.gpu
def test_a_volume_of_millions_of_samples(ctx):
    """8.5 million samples, 7.4 million vertices: many blocks per pass and the scans' recursive form.  An earlier form of
    `k_iso_edges` (its neighbour loads inside branches) passed every small case and gave a few hundred vertices too many
    or too few here, differently on every call.  The keys are checked against numpy, the rest by a second call."""
    shape = (256, 256, 130)
    values = np.random.default_rng(1).standard_normal(shape)
    inside = values < 1.5
    lin = np.arange(values.size, dtype=np.int64).reshape(shape)
    keys = []
    for kind, (di, dj, dk) in enumerate(ref.KINDS):
        lo = (slice(0, shape[0] - di), slice(0, shape[1] - dj), slice(0, shape[2] - dk))
        hi = (slice(di, None), slice(dj, None), slice(dk, None))
        keys.append(7 * lin[lo][inside[lo] != inside[hi]] + kind)
    keys = np.sort(np.concatenate(keys))
    a, b = ctx.isosurface(values, 1.5), ctx.isosurface(values, 1.5)
    assert a["report"][0] == len(keys) and np.array_equal(a["vertex_key"], keys)
    for k in ("points", "faces", "vertex_key", "face_cell", "report"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(ctx):
    args, _, _ = case("random")
    a, b = ctx.isosurface(*args), ctx.isosurface(*args)
    for k in ("points", "faces", "vertex_key", "face_cell", "report"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.gpu
def test_the_library_refuses_bad_input(hip, ctx):
    import ctypes as C

    lib, h = hip.load_library(), C.c_void_p()
    v, three = np.ones((2, 2, 2)), np.ones(3)

    def create(values, nx, ny, nz, level=0.0, flags=0):
        return lib.pf_isosurface_create(ctx._h, hip._f64(values), nx, ny, nz, level, hip._f64(three), hip._f64(three), flags,
                                        C.byref(h), None, None)

    assert create(v, 2, 2, 1) == -1 and b"extents" in lib.pf_last_error()
    assert create(v, 2, 2, 2, flags=1) == -1 and b"flags" in lib.pf_last_error()
    assert create(v, 2, 2, 2, level=float("nan")) == -1
    bad = v.copy()
    bad[1, 1, 0] = np.inf
    assert create(bad, 2, 2, 2) == -1 and b"value 6" in lib.pf_last_error()
    assert not h.value
    assert create(v, 2, 2, 2) == 0 and h.value  # without report and device_ms
    assert lib.pf_isosurface_fetch(h, None, None, None, None) == 0  # an empty surface has nothing to fetch
    lib.pf_isosurface_free(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name,genus", [("sphere", 0), ("torus", 1)])
def test_mesh_topology_of_the_result(ctx, name, genus):
    from pyfocusr_amd.isosurface import isosurface
    from pyfocusr_amd.topology import mesh_topology

    args, want, _ = case(name)
    mesh, info = isosurface(*args, return_info=True, ctx=ctx)
    assert np.array_equal(mesh.points, want[0]) and np.array_equal(info.face_cell, want[3]) and info.shape == args[0].shape
    topo = mesh_topology(mesh, ctx=ctx)
    assert topo.n_patches == 1 and topo.n_boundary_edges == 0 and topo.n_nonmanifold_edges == 0 and topo.n_inconsistent_edges == 0
    p = topo.patches
    assert p["closed"][0] and p["orientable"][0] and p["genus"][0] == genus
    assert not topo.flip.any() and p["signed_volume"][0] > 0.0  # already consistent and outward: nothing to reverse


@pytest.mark.gpu
def test_mask_to_mesh_and_closed_on_the_device(ctx):
    from pyfocusr_amd.isosurface import mask_to_mesh, prepare_volume

    mask = _mask()
    mesh = mask_to_mesh(mask, ctx=ctx)
    want = ref.isosurface_ref(*prepare_volume(mask.astype(np.float64), 0.5, inside="above", closed=True))
    assert np.array_equal(mesh.points, want[0]) and np.array_equal(mesh.faces, want[1])
    assert ref.signed_volume(mesh.points, mesh.faces) == 46.0
    empty = mask_to_mesh(np.zeros((3, 3, 3), dtype=bool), ctx=ctx)
    assert empty.points.shape == (0, 3) and empty.faces.shape == (0, 3)


@pytest.mark.gpu
def test_pool_contents_change_nothing(hip, ctx):
    """The four runs of tests/test_pool_hygiene.py for this unit: plain, every pool block filled with 0xFF, with 0x00, and
    after a neighbour twice as large per axis on the same ctx."""
    from test_pool_hygiene import _drop, _flat

    values, big = ref.wave_field((5, 6, 70)), ref.wave_field((10, 12, 140))
    want = ref.isosurface_ref(values, 0.1, (1.0, 0.5, 2.0), (0.0, 1.0, 2.0))

    def run(neighbour):
        if neighbour:
            ctx.isosurface(big, 0.1)
        return _drop(ctx.isosurface(values, 0.1, (1.0, 0.5, 2.0), (0.0, 1.0, 2.0)))

    lib, runs = hip.load_library(), {}
    try:
        for mode, label in ((0, "plain"), (1, "0xFF"), (2, "0x00")):
            assert lib.pf_pool_poison(mode) == 0
            out = run(False)
            if mode == 0:
                _assert_equal(out, want)
            runs[label] = _flat(out)
    finally:
        lib.pf_pool_poison(0)
    runs["after a larger neighbour"] = _flat(run(True))
    plain = runs.pop("plain")
    assert len(plain) == 5
    for label, got in runs.items():
        differ = [w for (w, a), (_, b) in zip(plain, got) if a != b]
        assert len(got) == len(plain) and not differ, "%s: %s differ from the plain run" % (label, ", ".join(differ))


_H = 4.0  # the lattice spacing of the chains: the blob is about 96 x 53 x 33


@pytest.fixture(scope="module")
def blob():
    from pyfocusr_amd.meshgen import blob_mesh

    return blob_mesh(700, seed=0)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [-0.5, 0.0, 2.0])
def test_offset_surface_lies_within_a_cell_diagonal(ctx, blob, factor):
    """|d| against the exact distance of every output vertex.  The bound is derived: the distance is 1-Lipschitz, so along
    a lattice edge both the field and its linear interpolant stay within the edge's length of the level, and the longest
    edge is the cell's diagonal; 1e-12 for the rounding."""
    from pyfocusr_amd.isosurface import offset_surface
    from pyfocusr_amd.surface_distance import point_to_surface_distances
    from pyfocusr_amd.topology import mesh_topology

    d = factor * _H
    out = offset_surface(blob, d, _H, sign="pseudonormal", ctx=ctx)
    assert len(out.points) > 100
    dist, _ = point_to_surface_distances(out.points, blob, ctx=ctx)
    worst = float(np.max(np.abs(abs(d) - dist)))
    print("offset %g: worst | |d| - distance | = %g, bound %g" % (d, worst, np.sqrt(3.0) * _H))
    assert worst <= np.sqrt(3.0 * _H * _H) + 1e-12
    topo = mesh_topology(out, ctx=ctx)
    assert topo.n_patches == 1 and topo.patches["closed"][0] and topo.patches["genus"][0] == 0


@pytest.mark.gpu
def test_voxel_remesh_closes_an_open_blob(ctx, blob):
    from pyfocusr_amd.isosurface import voxel_remesh
    from pyfocusr_amd.topology import mesh_topology

    keep = np.ones(len(blob.faces), dtype=bool)
    keep[np.random.default_rng(3).choice(len(blob.faces), size=40, replace=False)] = False
    out = voxel_remesh((blob.points, blob.faces[keep]), _H, sign="winding", ctx=ctx)
    topo = mesh_topology(out, ctx=ctx)
    assert len(out.faces) > 100 and topo.n_boundary_edges == 0 and topo.n_nonmanifold_edges == 0 and topo.n_inconsistent_edges == 0
    assert np.all(topo.patches["closed"]) and np.all(topo.patches["orientable"])
