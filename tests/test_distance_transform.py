"""Exact Euclidean distance transforms of masks (`pf_edt_*`, pyfocusr_amd/distance_transform.py).

The CPU tests hold the numpy statement of the definition (tests/_edt_ref.py: the three stages of include/pyfocusr_hip.h) to
a global brute force, to scipy and to scipy's ball morphology; the GPU tests hold the device to that statement bit for bit,
on the smallest shapes at which a kernel can go wrong: z-lines that end on, cross and start a 64-bit word, y- and x-lines
longer than a wave and than a block, extents of 1."""
import os
import re

import numpy as np
import pytest

import _edt_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = (0.3, 0.7, 1.1, 0.37, 2.5)  # none of them representable but 2.5: every product and sum rounds


def _random_cases(n=40, seed=7):
    rng = np.random.default_rng(seed)
    for density in np.geomspace(0.02, 0.9, n):
        shape = tuple(int(e) for e in rng.integers(1, 9, size=3))
        yield rng.random(shape) < density, rng.choice(SPACINGS, size=3)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------ the reference, on the CPU
def test_staged_reference_equals_the_brute_force():
    n_features = 0
    for mask, spacing in _random_cases():
        d2, near = ref.edt_staged(mask, spacing)
        want, _ = ref.edt_brute(mask, spacing)
        assert _bits_equal(d2, want), (mask.shape, spacing)
        assert near.dtype == np.int32 and np.array_equal(near >= 0, np.isfinite(d2))
        n_features += int(mask.sum())
    assert n_features > 500


def test_nearest_is_a_minimiser_exactly():
    for mask, spacing in _random_cases(seed=8):
        d2, near = ref.edt_staged(mask, spacing)
        if not mask.any():
            continue
        assert mask.reshape(-1)[near.reshape(-1)].all()  # a feature
        c = ref.cost(mask.shape, spacing, np.arange(mask.size), near.reshape(-1))
        assert _bits_equal(c, d2.reshape(-1))


def test_unit_spacing_gives_the_lowest_flat_index():
    for mask, _ in _random_cases(seed=9):
        for spacing in (1.0, (1.0, 2.0, 3.0)):  # every sum exact
            d2, near = ref.edt_staged(mask, spacing)
            want_d2, want_near = ref.edt_brute(mask, spacing)
            assert _bits_equal(d2, want_d2) and np.array_equal(near, want_near)


def test_volumes_without_and_of_nothing_but_features():
    shape = (3, 4, 5)
    d2, near = ref.edt_staged(np.zeros(shape, dtype=bool), (0.3, 0.7, 1.1))
    assert np.all(d2 == np.inf) and np.all(near == -1)
    d2, near = ref.edt_staged(np.ones(shape, dtype=bool), (0.3, 0.7, 1.1))
    assert np.all(d2 == 0.0) and np.array_equal(near.reshape(-1), np.arange(60))
    assert not np.signbit(d2).any()


def test_signed_definition():
    for mask, spacing in _random_cases(seed=10):
        dist, d2, near = ref.edt_signed(mask, spacing)
        bdist, bd2, _ = ref.edt_signed(mask, spacing, transform=ref.edt_brute)
        assert _bits_equal(dist, bdist) and _bits_equal(d2, bd2)
        if mask.any() and not mask.all():
            assert np.all(dist[mask] < 0.0) and np.all(dist[~mask] > 0.0)
            assert np.array_equal(np.abs(dist), np.sqrt(d2))
            assert np.all(mask.reshape(-1)[near.reshape(-1)] != mask.reshape(-1))  # the other class
        elif mask.all():
            assert np.all(dist == -np.inf) and np.all(d2 == np.inf) and np.all(near == -1)
        else:
            assert np.all(dist == np.inf) and np.all(d2 == np.inf) and np.all(near == -1)


def test_reference_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for mask, spacing in _random_cases(seed=11):
        if not mask.any():
            continue
        want = ndimage.distance_transform_edt(~mask, sampling=spacing)
        got = np.sqrt(ref.edt_staged(mask, spacing)[0])
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
    print("largest relative difference from scipy: %.3g" % worst)
    assert worst <= 1e-14


def test_ball_morphology_of_the_reference_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(12)
    for radius in (1.0, 1.5, 2.0, 2.3, 3.0):
        for density in (0.03, 0.5, 0.9):
            mask = rng.random((9, 10, 11)) < density
            assert np.array_equal(ref.dilate(mask, radius), ndimage.binary_dilation(mask, structure=ref.ball(radius)))
            assert np.array_equal(ref.erode(mask, radius), ndimage.binary_erosion(mask, structure=ref.ball(radius), border_value=0))


def test_entry_points_are_declared_and_bound():
    import sys

    import pyfocusr_amd
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, res, arity in (("pf_edt_create", "int", 11), ("pf_edt_fetch", "int", 4), ("pf_edt_isosurface", "int", 6),
                             ("pf_edt_free", "void", 1)):
        m = re.search(r"%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity
        assert len(_hip.SIGNATURES[name][1]) == arity
    assert re.search(r"enum\s*\{\s*PF_EDT_UNSIGNED\s*=\s*0\s*,\s*PF_EDT_SIGNED\s*=\s*1\s*\}", header)
    assert (_hip.PF_EDT_UNSIGNED, _hip.PF_EDT_SIGNED) == (0, 1)
    for words in ("(t_z + t_y) + t_x", "the lower k' on a tie", "the lower j' on a tie", "the lower i' on a tie"):
        assert words in header
    assert callable(_hip.Context.distance_transform) and _hip.DeviceDistanceTransform._free == "pf_edt_free"
    for name in ("distance_transform", "signed_distance_of_mask", "nearest_feature", "propagate_labels", "dilate_mask", "erode_mask",
                 "open_mask", "close_mask", "mask_offset_surface"):
        assert callable(getattr(pyfocusr_amd, name))
    assert "dist2 <= radius * radius" in sys.modules["pyfocusr_amd.distance_transform"].__doc__


def test_argument_errors_come_before_the_library(monkeypatch):
    from pyfocusr_amd import _hip
    from pyfocusr_amd import distance_transform as _  # noqa: F401  (the function shadows the module's name)
    import sys

    dt = sys.modules["pyfocusr_amd.distance_transform"]
    from pyfocusr_amd.isosurface import mask_to_mesh

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")

    monkeypatch.setattr(_hip, "default_context", no_library)
    monkeypatch.setattr(_hip, "load_library", no_library)
    good = np.zeros((3, 4, 5), dtype=bool)
    good[1, 2, 3] = True
    with pytest.raises(ValueError, match="dimensions"):
        dt.distance_transform(good[0])
    with pytest.raises(ValueError, match="at least 1"):
        dt.distance_transform(good[:, :0, :])
    with pytest.raises(TypeError, match="boolean or a label map"):
        dt.distance_transform(good.astype(np.float64))
    for spacing in (0.0, -1.0, np.inf, np.nan, (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="positive and finite"):
            dt.distance_transform(good, spacing)
    with pytest.raises(ValueError, match="one number or three"):
        dt.signed_distance_of_mask(good, (1.0, 2.0))
    for spacing in (1e-200, 1e200):  # t_z would stop growing with the offset
        with pytest.raises(ValueError, match="normal doubles"):
            dt.nearest_feature(good, spacing)
    with pytest.raises(ValueError, match="dimensions"):
        dt.propagate_labels(np.zeros((4, 4), dtype=np.int32))
    for morph in (dt.dilate_mask, dt.erode_mask, dt.open_mask, dt.close_mask):
        with pytest.raises(ValueError, match="radius"):
            morph(good, -1.0)
        with pytest.raises(ValueError, match="radius"):
            morph(good, np.nan)
        with pytest.raises(ValueError, match="positive and finite"):
            morph(good, 1.0, spacing=-2.0)
    with pytest.raises(ValueError, match="distance must be finite"):
        dt.mask_offset_surface(good, np.inf)
    with pytest.raises(ValueError, match="origin"):
        dt.mask_offset_surface(good, 1.0, origin=(0.0, 1.0))
    with pytest.raises(ValueError, match="method"):
        mask_to_mesh(good, method="smooth")
    with pytest.raises(ValueError, match="at least 2"):
        mask_to_mesh(good[:, :, :1], closed=False, method="distance")
    # a mask with an empty class has no surface, and no device call finds that out
    for empty in (np.zeros((3, 3, 3), dtype=bool), np.ones((3, 3, 3), dtype=bool)):
        mesh = dt.mask_offset_surface(empty, 1.0)
        assert mesh.points.shape == (0, 3) and mesh.faces.shape == (0, 3)
    mesh, info = mask_to_mesh(np.zeros((3, 3, 3), dtype=bool), method="distance", return_info=True)
    assert mesh.points.shape == (0, 3) and info.shape == (5, 5, 5) and info.vertex_key.dtype == np.int64


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def dt():
    import sys

    import pyfocusr_amd  # noqa: F401

    return sys.modules["pyfocusr_amd.distance_transform"]


_SHAPES = [(3, 4, 64), (2, 3, 65), (3, 4, 130),  # z-lines that end on, cross and start a 64-bit word
           (3, 130, 2), (130, 2, 3), (300, 2, 2),  # y- and x-lines longer than a wave and than a block of 256
           (1, 1, 1), (1, 7, 1), (5, 1, 9)]  # extents of 1
_ANISO = (0.3, 0.7, 1.1)
_CONTENTS = ("corner", "far_corner", "none", "all", "sparse", "half", "dense", "steep", "steep_reversed", "ties2", "ties4")


def _content(shape, name):
    """(mask, spacing) of one of _CONTENTS on `shape`."""
    rng = np.random.default_rng(list(shape) + [_CONTENTS.index(name)])
    mask, spacing = np.zeros(shape, dtype=bool), _ANISO
    if name == "corner":  # full-length scans; every other z-line has no feature in stage z
        mask[0, 0, 0] = True
    elif name == "far_corner":
        mask[-1, -1, -1] = True
    elif name == "all":
        mask[:] = True
    elif name in ("sparse", "half", "dense"):
        mask = rng.random(shape) < {"sparse": 0.005, "half": 0.5, "dense": 0.99}[name]
    elif name in ("steep", "steep_reversed"):  # one axis decides where the search stops
        mask, spacing = rng.random(shape) < 0.1, (1e-3, 1.0, 1e3) if name == "steep" else (1e3, 1.0, 1e-3)
    elif name in ("ties2", "ties4"):  # features symmetric about voxels along every axis: every tie rule fires
        step = int(name[-1])
        mask[::step, ::step, ::step] = True
        spacing = (1.0, 1.0, 1.0)
    return mask, spacing


def test_the_contents_are_what_they_claim():
    """The random contents are the same in every process; the tie contents do tie."""
    a, b = _content((3, 4, 130), "half"), _content((3, 4, 130), "half")
    assert np.array_equal(a[0], b[0]) and 0.4 < a[0].mean() < 0.6
    mask, spacing = _content((5, 1, 9), "ties2")
    d2, near = ref.edt_staged(mask, spacing)
    _, lowest = ref.edt_brute(mask, spacing)
    assert np.array_equal(near, lowest) and d2[1, 0, 1] == 2.0 and near[1, 0, 1] == 0  # four features tie for (1, 0, 1)


def _assert_device_is(raw, want_dist, want_d2, want_near, n_foreground):
    assert raw["dist"].dtype == np.float64 and raw["dist2"].dtype == np.float64 and raw["nearest"].dtype == np.int32
    assert _bits_equal(raw["nearest"], want_near)
    assert _bits_equal(raw["dist2"], want_d2)
    assert _bits_equal(raw["dist"], want_dist)
    assert tuple(raw["report"][:3]) == (want_d2.size, n_foreground, want_d2.size - n_foreground) and np.all(raw["report"][3:] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _CONTENTS)
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_the_reference(ctx, shape, name):
    mask, spacing = _content(shape, name)
    d2, near = ref.edt_staged(mask, spacing)
    raw = ctx.distance_transform(mask, spacing)
    _assert_device_is(raw, np.sqrt(d2), d2, near, int(mask.sum()))
    assert raw["device_ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_signed_mode_equals_the_reference(ctx, shape):
    for name in ("half", "sparse", "corner", "ties2", "none", "all"):
        mask, spacing = _content(shape, name)
        dist, d2, near = ref.edt_signed(mask, spacing)
        _assert_device_is(ctx.distance_transform(mask, spacing, signed=True), dist, d2, near.astype(np.int32), int(mask.sum()))


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(ctx):
    mask, spacing = _content((3, 130, 2), "half")
    for signed in (False, True):
        a, b = ctx.distance_transform(mask, spacing, signed=signed), ctx.distance_transform(mask, spacing, signed=signed)
        for k in ("dist", "dist2", "nearest", "report"):
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.gpu
def test_pool_contents_change_nothing(hip, ctx):
    """The four runs of tests/test_pool_hygiene.py for this unit: plain, every pool block filled with 0xFF, with 0x00, and
    after a neighbour twice as large per axis on the same ctx."""
    from test_pool_hygiene import _drop, _flat

    rng = np.random.default_rng(5)
    mask, big = rng.random((5, 6, 70)) < 0.05, rng.random((10, 12, 140)) < 0.05
    want = ref.edt_staged(mask, _ANISO), ref.edt_signed(mask, _ANISO)

    def run(neighbour):
        if neighbour:
            ctx.distance_transform(big, _ANISO, signed=True)
        return {"unsigned": _drop(ctx.distance_transform(mask, _ANISO)), "signed": _drop(ctx.distance_transform(mask, _ANISO, signed=True))}

    lib, runs = hip.load_library(), {}
    try:
        for mode, label in ((0, "plain"), (1, "0xFF"), (2, "0x00")):
            assert lib.pf_pool_poison(mode) == 0
            out = run(False)
            if mode == 0:
                _assert_device_is(out["unsigned"], np.sqrt(want[0][0]), want[0][0], want[0][1], int(mask.sum()))
                _assert_device_is(out["signed"], want[1][0], want[1][1], want[1][2].astype(np.int32), int(mask.sum()))
            runs[label] = _flat(out)
    finally:
        lib.pf_pool_poison(0)
    runs["after a larger neighbour"] = _flat(run(True))
    plain = runs.pop("plain")
    assert len(plain) == 8
    for label, got in runs.items():
        differ = [w for (w, a), (_, b) in zip(plain, got) if a != b]
        assert len(got) == len(plain) and not differ, "%s: %s differ from the plain run" % (label, ", ".join(differ))


@pytest.mark.gpu
def test_the_library_refuses_bad_input(hip, ctx):
    import ctypes as C

    lib, h, iso = hip.load_library(), C.c_void_p(), C.c_void_p()
    mask, three = np.ones(8, dtype=np.uint8), np.ones(3)

    def create(nx, ny, nz, spacing=three, mode=0, flags=0, m=mask):
        return lib.pf_edt_create(ctx._h, hip._ptr(m), nx, ny, nz, hip._f64(np.asarray(spacing, dtype=np.float64)), mode, flags,
                                 C.byref(h), None, None)

    assert create(2, 2, 0) == -1 and b"extents" in lib.pf_last_error()
    assert create(0, 2, 2) == -1 and b"extents" in lib.pf_last_error()
    assert create(2 ** 16, 2 ** 15, 1) == -1 and b"samples" in lib.pf_last_error()  # 2^31 samples: refused before any is read
    assert create(2 ** 31, 1, 1) == -1
    for bad in (0.0, -1.0, np.inf, np.nan):
        for axis in range(3):
            spacing = np.ones(3)
            spacing[axis] = bad
            assert create(2, 2, 2, spacing) == -1 and b"positive and finite" in lib.pf_last_error()
    assert create(2, 2, 2, (1.0, 1e-200, 1.0)) == -1 and b"normal doubles" in lib.pf_last_error()
    assert create(2, 2, 2, (1e200, 1.0, 1.0)) == -1
    assert create(2, 2, 2, mode=2) == -1 and b"mode" in lib.pf_last_error()
    assert create(2, 2, 2, mode=-1) == -1
    assert create(2, 2, 2, flags=1) == -1 and b"flags" in lib.pf_last_error()
    assert not h.value

    def surface(level=0.5, origin=three):
        return lib.pf_edt_isosurface(h, level, hip._f64(origin), C.byref(iso), None, None)

    one_feature = np.zeros(8, dtype=np.uint8)
    one_feature[3] = 1
    assert create(2, 2, 2, m=one_feature) == 0 and h.value  # without report and device_ms
    assert lib.pf_edt_fetch(h, None, None, None) == 0  # nothing asked for
    assert surface(level=np.nan) == -1 and b"level" in lib.pf_last_error()
    assert surface(level=np.inf) == -1
    assert surface(origin=np.array([0.0, np.inf, 0.0])) == -1 and b"origin" in lib.pf_last_error()
    assert surface() == 0 and iso.value
    lib.pf_isosurface_free(iso)
    lib.pf_edt_free(h)
    for shape in ((2, 4, 1), (1, 4, 2), (4, 1, 2)):  # a transform, but no surface
        assert create(*shape, m=one_feature) == 0
        assert surface() == -1 and b"extents" in lib.pf_last_error()
        lib.pf_edt_free(h)
    for m, mode, word in ((np.zeros(8, dtype=np.uint8), 0, b"foreground"), (np.zeros(8, dtype=np.uint8), 1, b"foreground"),
                          (mask, 1, b"background")):  # the field is not finite
        assert create(2, 2, 2, mode=mode, m=m) == 0
        assert surface() == -1 and word in lib.pf_last_error()
        lib.pf_edt_free(h)
    assert create(2, 2, 2, m=mask) == 0  # all features, unsigned: the field is 0 everywhere, and finite
    assert surface() == 0
    lib.pf_isosurface_free(iso)
    lib.pf_edt_free(h)


@pytest.fixture(scope="module")
def organ():
    """A 96 x 100 x 130 mask: three overlapping ellipsoids, a detached one and specks."""
    shape, rng = (96, 100, 130), np.random.default_rng(3)
    mask = np.zeros(shape, dtype=bool)
    for centre, radius in (((40, 50, 60), 28.0), ((60, 45, 80), 20.0), ((30, 60, 40), 15.0), ((80, 85, 110), 9.0)):
        mask |= ref.ball_mask(shape, centre, radius, (1.0, 0.9, 0.8))
    mask |= rng.random(shape) < 2e-4
    return mask


@pytest.mark.gpu
def test_a_volume_of_a_million_samples_against_scipy(ctx, organ):
    ndimage = pytest.importorskip("scipy.ndimage")
    spacing = (0.37, 0.7, 1.1)
    raw = ctx.distance_transform(organ, spacing)
    want = ndimage.distance_transform_edt(~organ, sampling=spacing)
    worst = float(np.max(np.abs(raw["dist"] - want) / np.maximum(want, 1e-300)))
    print("largest relative difference from scipy: %.3g" % worst)
    assert worst <= 1e-14
    near = raw["nearest"].reshape(-1)
    assert near.min() >= 0 and organ.reshape(-1)[near].all()
    assert _bits_equal(ref.cost(organ.shape, spacing, np.arange(organ.size), near), raw["dist2"].reshape(-1))
    assert _bits_equal(np.sqrt(raw["dist2"]), raw["dist"])
    signed = ctx.distance_transform(organ, spacing, signed=True)
    inside = ndimage.distance_transform_edt(organ, sampling=spacing)
    assert np.max(np.abs(signed["dist"] - (want - inside)) / np.abs(want - inside)) <= 1e-14
    other = signed["nearest"].reshape(-1)
    assert np.all(organ.reshape(-1)[other] != organ.reshape(-1))
    assert _bits_equal(ref.cost(organ.shape, spacing, np.arange(organ.size), other), signed["dist2"].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("signed,level", [(True, 0.0), (True, 0.7), (True, -0.45), (False, 1.0)])
def test_the_resident_field_gives_the_surface_of_the_fetched_one(hip, ctx, signed, level):
    mask = ref.ball_mask((12, 13, 14), (5.5, 6.0, 7.2), 4.0, (1.0, 0.9, 0.8))
    spacing, origin = np.array(_ANISO), np.array([1.0, -2.0, 3.0])
    with hip.DeviceDistanceTransform(mask, spacing, signed=signed, ctx=ctx) as edt:
        dist = edt.fetch()[0]
        with edt.isosurface(level, origin) as iso:
            got = iso.fetch()
            report = iso.report
    want = ctx.isosurface(dist, level, spacing, origin)
    assert len(want["points"]) > 100
    for a, k in zip(got, ("points", "faces", "vertex_key", "face_cell")):
        assert _bits_equal(a, want[k]), k
    assert np.array_equal(report, want["report"])


@pytest.mark.gpu
def test_mask_to_mesh_by_distance(ctx):
    from pyfocusr_amd.isosurface import mask_to_mesh
    from pyfocusr_amd.topology import mesh_topology

    mask = ref.ball_mask((14, 15, 16), (6.5, 7.0, 8.2), 5.0)
    spacing, origin = (0.5, 0.7, 1.1), (1.0, 2.0, 3.0)
    for closed in (True, False):
        stairs, s_info = mask_to_mesh(mask, spacing, origin, closed=closed, return_info=True, ctx=ctx)
        mesh, info = mask_to_mesh(mask, spacing, origin, closed=closed, return_info=True, ctx=ctx, method="distance")
        assert len(mesh.faces) > 100 and info.shape == s_info.shape and np.array_equal(info.origin, s_info.origin)
        assert np.array_equal(mesh.faces, stairs.faces) and np.array_equal(info.vertex_key, s_info.vertex_key)
        assert np.array_equal(info.face_cell, s_info.face_cell)
        assert not np.array_equal(mesh.points, stairs.points)
    topo = mesh_topology(mesh, ctx=ctx)
    assert topo.n_patches == 1 and topo.n_boundary_edges == 0 and topo.n_nonmanifold_edges == 0 and topo.n_inconsistent_edges == 0
    p = topo.patches
    assert p["closed"][0] and p["orientable"][0] and p["genus"][0] == 0 and p["signed_volume"][0] > 0.0
    empty = mask_to_mesh(np.zeros((3, 3, 3), dtype=bool), ctx=ctx, method="distance")
    assert empty.points.shape == (0, 3) and empty.faces.shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("distance", [2.0, -2.0, 3.1])
def test_mask_offset_surface_lies_within_a_cell_diagonal(ctx, dt, distance):
    """Every vertex v: | min_q |v - q| - |distance| | <= one cell diagonal, q over the foreground voxel centres for a
    margin and over the background ones for a shell: the Lipschitz bound `offset_surface` states.  |distance| is at least
    two cell diagonals (0.87 each)."""
    shape, h, origin = (22, 22, 22), 0.5, np.array([1.0, 2.0, 3.0])
    mask = ref.ball_mask(shape, (10.0, 10.5, 11.0), 8.0)  # 8 voxels = 4 units; 3 voxels of background around it
    mesh = dt.mask_offset_surface(mask, distance, h, origin, ctx=ctx)
    assert len(mesh.points) > 300
    centres = origin + h * np.argwhere(mask if distance > 0 else ~mask)
    nearest = np.array([np.sqrt(np.min(np.sum((centres - v) ** 2, axis=1))) for v in mesh.points])
    diagonal = h * np.sqrt(3.0)
    worst = float(np.max(np.abs(nearest - abs(distance))))
    print("distance %g: largest deviation %.4f of a cell diagonal %.4f" % (distance, worst, diagonal))
    assert abs(distance) >= 2 * diagonal and worst <= diagonal
    from pyfocusr_amd.topology import mesh_topology

    topo = mesh_topology(mesh, ctx=ctx)
    assert topo.n_patches == 1 and topo.n_boundary_edges == 0 and topo.patches["genus"][0] == 0


@pytest.mark.gpu
def test_opening_removes_a_speck_and_closing_fills_a_pinhole(ctx, dt):
    shape = (16, 17, 18)
    ball = ref.ball_mask(shape, (7, 8, 9), 4.0)
    core = ref.ball_mask(shape, (7, 8, 9), 3.0)
    speck = ball.copy()
    speck[13, 14, 15] = True
    opened = dt.open_mask(speck, 1.0, ctx=ctx)
    assert opened.dtype == bool and not opened[13, 14, 15] and not (opened & ~ball).any() and opened[core].all()
    assert np.array_equal(opened, ref.dilate(ref.erode(speck, 1.0), 1.0))
    pinhole = ball.copy()
    pinhole[7, 8, 9] = False
    closed = dt.close_mask(pinhole, 1.0, ctx=ctx)
    assert closed[7, 8, 9] and closed[ball].all()
    assert np.array_equal(closed, ref.erode(ref.dilate(pinhole, 1.0), 1.0))
    # a radius in millimetres on anisotropic voxels, and the border: outside is background for erosion only
    spacing, rng = (0.5, 1.0, 2.0), np.random.default_rng(4)
    mask = rng.random(shape) < 0.4
    for radius in (0.0, 1.0, 2.2):
        assert np.array_equal(dt.dilate_mask(mask, radius, spacing, ctx=ctx), ref.dilate(mask, radius, spacing))
        assert np.array_equal(dt.erode_mask(~mask, radius, spacing, ctx=ctx), ref.erode(~mask, radius, spacing))
    assert not dt.erode_mask(np.ones(shape, dtype=bool), 1.0, ctx=ctx)[0].any() and dt.erode_mask(np.ones(shape, dtype=bool), 1.0, ctx=ctx)[2:-2, 2:-2, 2:-2].all()


@pytest.mark.gpu
def test_labels_and_features_follow_the_reference(ctx, dt):
    rng = np.random.default_rng(6)
    shape = (9, 20, 70)
    labels = np.where(rng.random(shape) < 0.01, rng.integers(1, 6, size=shape), 0).astype(np.int16)
    d2, near = ref.edt_staged(labels != 0, _ANISO)
    grown = dt.propagate_labels(labels, _ANISO, ctx=ctx)
    assert grown.dtype == labels.dtype and np.array_equal(grown, labels.reshape(-1)[near])
    assert np.array_equal(grown[labels != 0], labels[labels != 0]) and (grown != 0).all()
    triplets = dt.nearest_feature(labels, _ANISO, ctx=ctx)
    assert triplets.shape == shape + (3,) and np.array_equal(np.ravel_multi_index(tuple(np.moveaxis(triplets, -1, 0)), shape), near)
    nothing = np.zeros((2, 3, 4), dtype=np.int16)
    assert np.array_equal(dt.propagate_labels(nothing, ctx=ctx), nothing) and np.all(dt.nearest_feature(nothing, ctx=ctx) == -1)
    dist, index = dt.distance_transform(labels, _ANISO, return_nearest=True, ctx=ctx)
    assert _bits_equal(dist, np.sqrt(d2)) and _bits_equal(index, near)
    assert _bits_equal(dt.distance_transform(labels, _ANISO, squared=True, ctx=ctx), d2)
    signed = ref.edt_signed(labels != 0, _ANISO)
    assert _bits_equal(dt.signed_distance_of_mask(labels, _ANISO, ctx=ctx), signed[0])
    assert _bits_equal(dt.distance_transform(labels, _ANISO, signed=True, squared=True, ctx=ctx), signed[1])
