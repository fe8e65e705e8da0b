"""The Python side of the library boundary has one idiom: `_hip._ptr` for every array that crosses it, `_hip._Handle` for
every object that owns device memory, one copy of each shape check, and `_meshargs.checked_mesh` for the mesh argument of
the units.  Everything here but the last test runs without the library and without a GPU."""
import ctypes as C
import gc
import threading
import weakref

import numpy as np
import pytest

from pyfocusr_amd import _hip, _meshargs
from pyfocusr_amd.curvature import discrete_curvatures
from pyfocusr_amd.map_quality import map_distortion
from pyfocusr_amd.ray_casting import ray_mesh_intersections
from pyfocusr_amd.remesh import resample_mesh
from pyfocusr_amd.surface_distance import point_to_surface_distances, signed_point_to_surface_distances, winding_numbers
from pyfocusr_amd.topology import mesh_topology, orient_faces
from pyfocusr_amd.vtk_functions import PolyMesh

CUBE_POINTS = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                       [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], dtype=np.int32)
CUBE_QUADS = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]], dtype=np.int32)


# ---- pointers ------------------------------------------------------------------------------------------------------
def test_ptr_takes_its_type_from_the_array():
    assert _hip._ptr(None) is None
    for dtype, ctype in ((np.float64, C.c_double), (np.int32, C.c_int32), (np.int64, C.c_int64), (np.uint8, C.c_uint8)):
        a = np.zeros((3, 2), dtype=dtype)
        p = _hip._ptr(a)
        assert type(p) is C.POINTER(ctype)
        assert C.cast(p, C.c_void_p).value == a.ctypes.data


def test_ptr_refuses_what_the_library_cannot_read():
    with pytest.raises(TypeError):
        _hip._ptr(np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError):
        _hip._ptr(np.zeros((4, 4))[:, 0])


def test_f64_checks_dtype_and_layout():
    a = np.zeros((4, 4))
    assert C.cast(_hip._f64(a), C.c_void_p).value == a.ctypes.data
    with pytest.raises(TypeError):
        _hip._f64(np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError):
        _hip._f64(a[:, 0])


def test_structures_become_dicts_of_python_numbers():
    t = _hip.Timing(op_ms=1.5, op_launches=3)
    d = t.as_dict()
    assert list(d) == [name for name, _ in _hip.Timing._fields_]
    assert type(d["op_ms"]) is float and type(d["op_launches"]) is int and type(d["persist_steps"]) is int
    info = _hip._PersistInfo(enabled=1, launches=2**40)
    assert all(type(v) is int for v in info.as_dict().values()) and info.as_dict()["launches"] == 2**40
    s = _hip.AssignStats(phases=2, total_cost=0.25).as_dict()
    assert type(s["phases"]) is int and type(s["total_cost"]) is float and len(s) == len(_hip.AssignStats._fields_)


# ---- handles, over a stand-in of the library ---------------------------------------------------------------------------
class _Lib(object):
    """Records every call; a constructor hands out the handle 7."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name.endswith("_create"):
                args[-1]._obj.value = 7
            return 0
        return call


class _Ctx(object):
    _h = 1

    def __init__(self):
        self._lib = _Lib()
        self._children = weakref.WeakSet()


class _Thing(_hip._Handle):
    _free = "pf_thing_free"

    def __init__(self, ctx, refuse=False):
        _hip._Handle.__init__(self, ctx)
        if refuse:
            raise ValueError("refused before the library was asked")
        self._create("pf_thing_create", ctx._h)


def test_handle_frees_exactly_once():
    ctx = _Ctx()
    thing = _Thing(ctx)
    assert thing in ctx._children and thing._h.value == 7
    thing.close()
    thing.close()
    del thing
    gc.collect()
    assert ctx._lib.calls == ["pf_thing_create", "pf_thing_free"]


def test_handle_is_a_context_manager():
    ctx = _Ctx()
    with _Thing(ctx) as thing:
        assert ctx._lib.calls == ["pf_thing_create"]
    assert thing._h is None and ctx._lib.calls == ["pf_thing_create", "pf_thing_free"]
    with pytest.raises(RuntimeError):
        with _Thing(ctx) as other:
            raise RuntimeError("in the body")
    assert other._h is None and ctx._lib.calls == ["pf_thing_create", "pf_thing_free"] * 2


def test_handle_whose_constructor_raised_frees_nothing():
    ctx = _Ctx()
    thing = _Thing.__new__(_Thing)
    with pytest.raises(ValueError):
        thing.__init__(ctx, refuse=True)
    thing.close()
    del thing
    gc.collect()
    never = _Thing.__new__(_Thing)  # not even a context yet
    never.close()
    del never
    assert ctx._lib.calls == []


def test_context_closes_its_children_before_itself():
    ctx = _hip.Context.__new__(_hip.Context)
    ctx._lib, ctx._h, ctx.device, ctx._children = _Lib(), 1, 0, weakref.WeakSet()
    a, b = _Thing(ctx), _Thing(ctx)
    ctx.close()
    assert a._h is None and b._h is None and ctx._h is None
    assert ctx._lib.calls == ["pf_thing_create"] * 2 + ["pf_thing_free"] * 2 + ["pf_destroy"]
    ctx.close()
    assert ctx._lib.calls[-1] == "pf_destroy" and ctx._lib.calls.count("pf_destroy") == 1


def test_pinned_release_may_be_reentered_on_one_thread(monkeypatch):
    """A collection inside the locked region of `_pinned_release` can finalise another block on the same thread."""
    monkeypatch.setattr(_hip, "_lib", _Lib())
    monkeypatch.setattr(_hip, "_pinned_free", {})
    monkeypatch.setattr(_hip, "_pinned_cached", [0])

    def reenter():
        with _hip._pinned_lock:
            _hip._pinned_release(0x1000, 4096)

    worker = threading.Thread(target=reenter, daemon=True)
    worker.start()
    worker.join(timeout=5)
    assert not worker.is_alive()
    assert _hip._pinned_free == {4096: [0x1000]} and _hip._pinned_cached == [4096]
    assert _hip._lib.calls == ["pf_host_detach"]


# ---- the mesh argument of the units ----------------------------------------------------------------------------------
_Q = np.full((2, 3), 0.25)
_TRIANGLE_UNITS = {
    "discrete_curvatures": (discrete_curvatures, "curvatures need"),
    "mesh_topology": (mesh_topology, "topology needs"),
    "orient_faces": (orient_faces, "topology needs"),
    "resample_mesh": (lambda mesh: resample_mesh(mesh, 4), "topology needs"),
    "map_distortion": (lambda mesh: map_distortion(mesh, CUBE_POINTS, vertex_map=np.arange(8)), "curvatures need"),
}
_FINITE_UNITS = ("discrete_curvatures", "resample_mesh", "map_distortion")
_SURFACE_UNITS = {
    "point_to_surface_distances": lambda mesh: point_to_surface_distances(_Q, mesh),
    "signed_point_to_surface_distances": lambda mesh: signed_point_to_surface_distances(_Q, mesh),
    "winding_numbers": lambda mesh: winding_numbers(_Q, mesh),
    "ray_mesh_intersections": lambda mesh: ray_mesh_intersections(_Q, _Q + 1.0, mesh),
}
_UNITS = dict({name: call for name, (call, _) in _TRIANGLE_UNITS.items()}, **_SURFACE_UNITS)
_POINTS_MESSAGE = "mesh points must be a non-empty (n, 3) array"


def _refused(call, mesh, message, prefix=False):
    with pytest.raises(ValueError) as e:
        call(mesh)
    assert str(e.value).startswith(message) if prefix else str(e.value) == message


class _StandIn(object):
    def __init__(self, points, faces):
        self.points, self.faces = points, faces


@pytest.mark.parametrize("unit", sorted(_UNITS))
def test_every_unit_refuses_wrong_points(unit):
    _refused(_UNITS[unit], (CUBE_POINTS[:, :2], CUBE_FACES), _POINTS_MESSAGE)
    _refused(_UNITS[unit], (np.zeros((0, 3)), CUBE_FACES), _POINTS_MESSAGE)
    # 12 points of 2 coordinates are not regrouped into 8 of 3
    _refused(_UNITS[unit], _StandIn(np.zeros((12, 2)), CUBE_FACES), _POINTS_MESSAGE)


@pytest.mark.parametrize("unit", sorted(_TRIANGLE_UNITS))
def test_triangle_units_refuse_wrong_faces(unit):
    call, word = _TRIANGLE_UNITS[unit]
    _refused(call, (CUBE_POINTS, np.zeros((0, 3), dtype=np.int32)), "mesh faces must be a non-empty (m, 3) array")
    _refused(call, (CUBE_POINTS, CUBE_QUADS), "%s triangles: faces are (m, 4), triangulate them first" % word)
    _refused(call, (CUBE_POINTS, CUBE_FACES.astype(np.float64)), "face indices must be integers")
    for bad in (8, -1):
        faces = CUBE_FACES.copy()
        faces[5, 1] = bad
        _refused(call, (CUBE_POINTS, faces), "face index out of range 0 .. 7", prefix=True)
        _refused(call, (CUBE_POINTS, faces), "face index out of range 0 .. 7: 8 points do not cover the faces")


@pytest.mark.parametrize("unit", sorted(_SURFACE_UNITS))
def test_surface_units_refuse_wrong_faces(unit):
    message = "mesh faces must be a non-empty (F, verts_per_face >= 3) array"
    _refused(_SURFACE_UNITS[unit], (CUBE_POINTS, np.zeros((0, 3), dtype=np.int32)), message)
    _refused(_SURFACE_UNITS[unit], (CUBE_POINTS, CUBE_FACES[:, :2]), message)


@pytest.mark.parametrize("unit", _FINITE_UNITS)
def test_units_that_need_finite_points(unit):
    points = CUBE_POINTS.copy()
    points[3, 1] = np.nan
    _refused(_TRIANGLE_UNITS[unit][0], (points, CUBE_FACES), "mesh points must be finite")


def test_what_the_checker_leaves_alone():
    points = CUBE_POINTS.copy()
    points[3, 1] = np.nan
    pts, faces = _meshargs.checked_mesh((points, CUBE_FACES), triangles="topology needs", indices=True)  # topology's rules
    assert np.isnan(pts[3, 1]) and np.array_equal(faces, CUBE_FACES)
    # the surface units take polygons, and leave a wrong index to the library (PF_E_ARG), whatever the dtype
    pts, faces = _meshargs.checked_mesh((CUBE_POINTS, CUBE_QUADS))
    assert np.array_equal(faces, CUBE_QUADS) and faces.dtype == np.int32
    wrong = CUBE_FACES.copy()
    wrong[0, 0] = 8
    assert np.array_equal(_meshargs.checked_mesh((CUBE_POINTS, wrong))[1], wrong)
    assert np.array_equal(_meshargs.checked_mesh((CUBE_POINTS, CUBE_FACES.astype(np.float64)))[1], CUBE_FACES)


def test_rules_are_checked_in_one_order():
    """points shape, faces shape, triangles, integer, size, range, finite."""
    points = CUBE_POINTS.copy()
    points[0, 0] = np.inf
    wrong = CUBE_FACES.copy()
    wrong[0, 0] = 8
    rules = dict(triangles="curvatures need", indices=True, finite=True)
    with pytest.raises(ValueError, match="face index out of range"):
        _meshargs.checked_mesh((points, wrong), **rules)
    with pytest.raises(ValueError, match="must be integers"):
        _meshargs.checked_mesh((points, wrong.astype(np.float64)), **rules)
    with pytest.raises(ValueError, match="need triangles"):
        _meshargs.checked_mesh((points, CUBE_QUADS.astype(np.float64)), **rules)
    with pytest.raises(ValueError, match="mesh points must be a non-empty"):
        _meshargs.checked_mesh((points[:, :2], CUBE_QUADS), **rules)


def test_accepted_forms_give_the_same_arrays():
    rules = dict(triangles="curvatures need", indices=True, finite=True)
    forms = [PolyMesh(CUBE_POINTS, CUBE_FACES), (CUBE_POINTS, CUBE_FACES), [CUBE_POINTS.tolist(), CUBE_FACES.tolist()],
             (np.asfortranarray(CUBE_POINTS), CUBE_FACES.astype(np.int64)), _StandIn(CUBE_POINTS, CUBE_FACES)]
    results = [_meshargs.checked_mesh(form, **rules) for form in forms]
    results.append(_meshargs.checked_mesh(CUBE_POINTS, CUBE_FACES, **rules))  # points, faces: two arguments (curvatures)
    results.append(_meshargs.checked_mesh(forms[0]))  # the surface units' rules
    for pts, faces in results:
        assert pts.dtype == np.float64 and faces.dtype == np.int32
        assert pts.flags.c_contiguous and faces.flags.c_contiguous
        assert np.array_equal(pts, CUBE_POINTS) and np.array_equal(faces, CUBE_FACES)


def test_results_are_one_attribute_dict():
    from pyfocusr_amd.curvature import Curvatures
    from pyfocusr_amd.map_quality import MapDistortion
    from pyfocusr_amd.topology import MeshTopology

    for cls in (Curvatures, MeshTopology, MapDistortion):
        r = cls(area=1.0)
        assert isinstance(r, dict) and isinstance(r, _meshargs.AttrDict) and r.area == 1.0 and r["area"] == 1.0
        with pytest.raises(AttributeError):
            r.missing


# ---- the shape checks of _hip ----------------------------------------------------------------------------------------
def _message(call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    return str(e.value)


def test_shape_checks_say_what_they_said():
    assert _message(_hip._same_d, np.zeros((4, 3)), np.zeros((4, 2))) == "ref and qry must be (n, d) arrays with equal d"
    assert _message(_hip._same_d, np.zeros(4), np.zeros((4, 1))) == "ref and qry must be (n, d) arrays with equal d"
    assert _message(_hip.check_knn_topk, np.zeros((4, 3)), np.zeros((4, 2)), 1) == "ref and qry must be (n, d) arrays with equal d"
    ctx = _hip.Context.__new__(_hip.Context)  # the checks come before the library is touched
    assert _message(ctx.assign, np.zeros((4, 3)), np.zeros((4, 2))) == "rows and cols must be (n, d) arrays with equal d"
    assert _message(ctx.knn1, np.zeros((4, 3)), np.zeros(4)) == "ref and qry must be (n, d) arrays with equal d"
    assert _message(_hip.DeviceCpd, np.zeros((4, 3)), np.zeros((4, 2)), ctx=_Ctx()) == "X (N,d) and Y (M,d) must share d"

    assert _message(_hip._queries, np.zeros((0, 3))) == "queries must be a non-empty (n, 3) array"
    assert _message(_hip._queries, np.zeros(3)) == "queries must be a non-empty (n, 3) array"
    assert _message(_hip._queries, np.zeros((2, 2))) == "queries must be a non-empty (n, 3) array"
    assert _message(point_to_surface_distances, np.zeros((0, 3)), None) == "query points must be a non-empty (n, 3) array"
    assert _message(ray_mesh_intersections, np.zeros(3), np.zeros(3), None) == "ray origins must be a non-empty (n, 3) array"
    rays = "origins and directions must be non-empty (n, 3) arrays of the same length"
    assert _message(_hip._rays, np.zeros((2, 3)), np.zeros((3, 3))) == rays
    assert _message(_hip._rays, np.zeros((0, 3)), np.zeros((0, 3))) == rays
    surface = _hip.DeviceSurface.__new__(_hip.DeviceSurface)
    assert _message(surface.raycast, np.zeros((2, 3)), np.zeros((3, 3))) == rays
    assert _message(surface.distance, np.zeros((0, 3))) == "queries must be a non-empty (n, 3) array"

    assert _message(_hip._upload_arrays, CUBE_POINTS, CUBE_FACES[0]) == "faces must be (F, verts_per_face)"
    assert _message(_hip._upload_arrays, CUBE_POINTS, np.zeros((0, 3)), empty_ok=False) == "faces must be a non-empty (F, verts_per_face) array"
    assert _message(_hip.DeviceSurface, CUBE_POINTS, np.zeros((0, 3)), ctx=_Ctx()) == "faces must be a non-empty (F, verts_per_face) array"
    pts, faces, v = _hip._upload_arrays(CUBE_POINTS.ravel(), CUBE_QUADS.astype(np.int64))
    assert pts.shape == (8, 3) and faces.dtype == np.int32 and faces.flags.c_contiguous and v == 4
    assert _hip._upload_arrays(CUBE_POINTS, np.zeros((0, 5)))[2] == 3


# ---- on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_handle_opens_with_with_and_closes_once():
    square, two = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]), np.array([[0, 1, 3], [0, 3, 2]], dtype=np.int32)
    basis = np.linalg.qr(np.random.default_rng(0).standard_normal((8, 2)))[0]
    ctx = _hip.Context()
    opened = []
    with _hip.DeviceMesh(CUBE_POINTS, CUBE_FACES, ctx=ctx) as mesh:
        with _hip.DeviceLaplacian(device_mesh=mesh) as graph:
            assert mesh.n == 8 and graph.n == 8 and graph.n_components == 1
            rows = graph.rows_create([0, 3])
            assert graph.download()["rowptr"][-1] == graph.nnz_w
            opened += [mesh, graph, rows]
    with _hip.DeviceSurface(CUBE_POINTS, CUBE_FACES, ctx=ctx) as surface:
        d2, face, _ = surface.distance(np.array([[0.5, 0.5, 2.0]]))
        assert abs(d2[0] - 1.0) < 1e-12 and face[0] in (10, 11)  # the two triangles of the side z = 1
        opened.append(surface)
    with _hip.DeviceSurfaceND(square, two, ctx=ctx) as flat:
        assert flat.closest(np.array([[0.25, 0.5]]))[3][0] < 1e-24
        opened.append(flat)
    with _hip.DeviceFunctionalMap(basis, basis, np.ones(8), ctx=ctx) as fmap:
        fmap.set_p2p(np.arange(8))
        assert np.array_equal(fmap.get_p2p(), np.arange(8)) and fmap.project(2, 2).shape == (2, 2)
        opened.append(fmap)
    with _hip.DeviceCpd(CUBE_POINTS, CUBE_POINTS + 0.1, ctx=ctx) as cpd:
        P1, Pt1, _ = cpd.estep(CUBE_POINTS + 0.1, 1.0)
        assert P1.shape == (8,) and abs(P1.sum() - Pt1.sum()) < 1e-12
        opened.append(cpd)
    for handle in opened:
        assert handle._h is None
        handle.close()  # silent, and frees nothing a second time
    left_open = _hip.DeviceMesh(CUBE_POINTS, CUBE_FACES, ctx=ctx)
    ctx.close()
    assert left_open._h is None and all(child._h is None for child in ctx._children)
    ctx.close()
