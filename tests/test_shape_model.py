"""Statistical shape models: the shape-population primitives (`pf_shapes_*`, `_hip.DeviceShapes`), generalized Procrustes
alignment and the Gram PCA (`pyfocusr_amd.shape_model`).

CPU part: the declarations, the argument checks that run before the library is loaded, `population_from_template` over a
stand-in for `Focusr`, and the behaviour of the algorithm on the numpy reference (tests/_shape_model_ref.py) alone.

GPU part (`-m gpu`): every primitive and both end-to-end calls against the reference, bit for bit - the device only adds,
subtracts, multiplies and divides in a stated order, and both sides run the same numpy SVD / eigh on inputs that are equal
bit for bit, so no tolerance stands between them.

Measured on the reference (CPU), blob_mesh(700, seed=0), S = 12, seed 0:
* one blob under similarity transforms: 1 iteration with and without scaling (the copies coincide after the first Kabsch
  step onto shape 0), change 1.2e-26 / 4.5e-24; largest deviation from the mean / RMS size 5.4e-15 with scaling, 6.7e-15
  without;
* planted modes: 8 iterations, the first two eigenvalues carry 0.99996 of the variance, principal angles between the first
  two modes and the planted pair (turned into the aligned frame) 0.0135 and 0.0200 rad."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _shape_model_ref as ref
from _map_quality_ref import tree_sum

import pyfocusr_amd
from pyfocusr_amd import _hip, shape_model
from pyfocusr_amd.meshgen import blob_mesh
from pyfocusr_amd.vtk_functions import PolyMesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_CPU = 12
# the largest deviation of an aligned copy from the mean over the RMS size, measured on the reference (module docstring);
# the bound is 100 times that, since rounding accumulates over the steps
MEASURED_DEVIATION = {True: 5.4e-15, False: 6.7e-15}
# the measured principal angles are 0.0135 and 0.0200 rad (the alignment of strongly deformed shapes is not the planted
# pose exactly); the bound is 2.5 times the larger
ANGLE_BOUND = 0.05

FUNCTIONS = {"pf_shapes_create": 6, "pf_shapes_free": 1, "pf_shapes_weight_sum": 2, "pf_shapes_center": 2, "pf_shapes_mean": 5,
             "pf_shapes_align_sums": 4, "pf_shapes_transform": 4, "pf_shapes_gram": 2, "pf_shapes_combine": 4, "pf_shapes_scores": 4,
             "pf_shapes_set_reference": 2, "pf_shapes_download": 2, "pf_shapes_device_ms": 3}


# ---- CPU: the surface ----------------------------------------------------------------------------------------------------
def test_declared_in_the_header_and_bound():
    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, n_args in FUNCTIONS.items():
        m = re.search(r"(?:int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == n_args, name
        assert len(_hip.SIGNATURES[name][1]) == n_args, name
    assert issubclass(_hip.DeviceShapes, _hip._Handle) and _hip.DeviceShapes._free == "pf_shapes_free"
    for name in ("generalized_procrustes", "ShapeModel", "build_shape_model", "population_from_template"):
        assert getattr(pyfocusr_amd, name) is getattr(shape_model, name)


def test_argument_checks_come_before_the_library(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_hip, "load_library", refuse)
    monkeypatch.setattr(_hip, "default_context", refuse)
    good = np.zeros((4, 5, 3))
    for call in (shape_model.generalized_procrustes, shape_model.build_shape_model, _hip.DeviceShapes):
        with pytest.raises(ValueError, match="same number of points"):
            call([np.zeros((5, 3)), np.zeros((6, 3))])
        with pytest.raises(ValueError, match="out of range"):
            call(np.zeros((0, 5, 3)))
        with pytest.raises(ValueError, match="at least one shape"):
            call([])
        with pytest.raises(TypeError, match="float64"):
            call(good.astype(np.float32))
        with pytest.raises(ValueError, match="C-contiguous"):
            call(np.zeros((4, 5, 6))[:, :, ::2])
        with pytest.raises(ValueError, match=r"\(S, n, 3\)"):
            call(np.zeros((4, 5, 2)))
        with pytest.raises(ValueError, match="finite"):
            call(np.full((4, 5, 3), np.nan))
        for bad in (-np.ones(5), np.array([1.0, 1.0, np.inf, 1.0, 1.0]), np.array([1.0, np.nan, 1.0, 1.0, 1.0])):
            with pytest.raises(ValueError, match="finite and not negative"):
                call(good, bad)
        with pytest.raises(ValueError, match="one entry per point"):
            call(good, np.ones(4))
        with pytest.raises(TypeError, match="float64"):
            call(good, np.ones(5, dtype=np.float32))
    for n_modes in (4, 0, 17):
        with pytest.raises(ValueError, match="n_modes"):
            shape_model.build_shape_model(good, n_modes=n_modes)
    with pytest.raises(ValueError, match="at least two"):
        shape_model.build_shape_model(np.zeros((1, 5, 3)))
    with pytest.raises(ValueError, match="max_iter"):
        shape_model.generalized_procrustes(good, max_iter=0)
    with pytest.raises(ValueError, match="positions"):
        shape_model.population_from_template(None, [None], positions="average")


class _FakeFocusr(object):
    """Records how it was built; `align_maps` leaves positions that tell the subject and the attribute apart."""
    built = []

    def __init__(self, vtk_mesh_target=None, vtk_mesh_source=None, **kwargs):
        self.target, self.source, self.kwargs = vtk_mesh_target, vtk_mesh_source, kwargs
        self.weighted_avg_transformed_points = self.surface_transformed_points = None
        self.nearest_neighbor_transformed_points = None
        type(self).built.append(self)

    def align_maps(self):
        n = len(self.source.points)
        base = np.arange(3.0 * n).reshape(n, 3) + 1000.0 * self.target.points[0, 0]
        self.weighted_avg_transformed_points = base + 0.25
        self.nearest_neighbor_transformed_points = base + 0.5
        if self.kwargs.get("return_surface_final_points"):
            self.surface_transformed_points = base + 0.75


@pytest.mark.parametrize("positions, offset", [("weighted", 0.25), ("nearest", 0.5), ("surface", 0.75)])
def test_population_from_template_over_a_stand_in(monkeypatch, positions, offset):
    import pyfocusr_amd.focusr as focusr_module

    _FakeFocusr.built = []
    monkeypatch.setattr(focusr_module, "Focusr", _FakeFocusr)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    template = PolyMesh(np.zeros((7, 3)), faces)
    subjects = [PolyMesh(np.full((9 + s, 3), float(s + 1)), faces) for s in range(4)]
    pop = shape_model.population_from_template(template, subjects, positions=positions, n_spectral_features=2)
    assert pop.shape == (4, 7, 3) and pop.dtype == np.float64 and pop.flags.c_contiguous
    assert len(_FakeFocusr.built) == 4
    for s, reg in enumerate(_FakeFocusr.built):
        assert reg.source is template and reg.target is subjects[s]  # the template is the source, the subject the target
        assert reg.kwargs["n_spectral_features"] == 2
        assert np.array_equal(pop[s], np.arange(21.0).reshape(7, 3) + 1000.0 * (s + 1) + offset)


# ---- CPU: the algorithm on the reference --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob():
    return ref.blob_points(700, 0)


@functools.lru_cache(maxsize=None)
def similarity_case(scaling):
    pop = ref.similarity_population(blob(), S_CPU, 0, scaling=scaling)
    return pop, ref.generalized_procrustes(pop, scaling=scaling, max_iter=20, tol=1e-12)


@functools.lru_cache(maxsize=None)
def planted_case():
    pop, P, m1, m2, a = ref.planted_population(blob(), S_CPU, 0)
    return pop, P, m1, m2, ref.build_shape_model(pop, scaling=False, tol=1e-12, max_iter=50)


@functools.lru_cache(maxsize=None)
def noisy_population():
    """The blob with independent noise on every vertex: S - 1 modes of comparable variance (a well-conditioned model)."""
    P = blob()
    return np.ascontiguousarray(P[None] + 0.05 * ref.rms_size(P) * np.random.default_rng(5).standard_normal((S_CPU,) + P.shape))


@functools.lru_cache(maxsize=None)
def weights_700():
    return np.random.default_rng(6).uniform(0.5, 1.5, 700)


@functools.lru_cache(maxsize=None)
def noisy_case(weighted):
    w = weights_700() if weighted else None
    return w, ref.build_shape_model(noisy_population(), weights=w, tol=1e-12, max_iter=50)


def test_tree_sums_is_tree_sum_per_column():
    x = np.random.default_rng(1).standard_normal((70000, 3)) * 10.0 ** np.random.default_rng(2).integers(-3, 4, (70000, 3))
    for n in (1, 255, 256, 257, 65537, 70000):
        got = ref.tree_sums(x[:n])
        assert [got[c] == tree_sum(x[:n, c]) for c in range(3)] == [True] * 3


@pytest.mark.parametrize("scaling", [True, False])
def test_one_blob_under_similarity_transforms(scaling):
    pop, g = similarity_case(scaling)
    assert g["converged"] and g["n_iter"] <= 20
    assert np.sqrt(g["history"][-1] / g["weight_sum"]) < 1e-12 * g["rho"]
    deviation = np.max(np.linalg.norm(g["aligned"] - g["mean"], axis=2)) / ref.rms_size(g["mean"])
    print("largest deviation from the mean / RMS size:", deviation, "iterations:", g["n_iter"])
    assert deviation <= 100 * MEASURED_DEVIATION[scaling]
    # the transforms are the alignment: A x + b gives the aligned shapes
    A = g["transforms"]
    again = np.einsum("sab,snb->sna", A[:, :3, :3], pop) + A[:, None, :3, 3]
    assert np.max(np.abs(again - g["aligned"])) <= 1e-12 * np.max(np.abs(pop))
    sizes = np.array([ref.rms_size(x) for x in g["aligned"]])
    if scaling:
        assert np.all(np.abs(sizes - 1.0) < 1e-12)  # the population did not shrink
    else:
        assert np.all(np.abs(sizes - ref.rms_size(blob())) < 1e-12 * ref.rms_size(blob()))


def test_planted_modes_are_found():
    pop, P, m1, m2, m = planted_case()
    assert m["converged"]
    ratio = m["explained_variance_ratio"]
    print("first two eigenvalues carry", ratio[:2].sum())
    assert ratio[:2].sum() >= 0.999
    # the aligned population lives in the pose of shape 0: turn the planted pair into that frame
    U, _, Vt = np.linalg.svd(P.T @ (m["mean"] - m["mean"].mean(0)))
    d = np.array([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = (U * d) @ Vt
    angles = ref.principal_angles(m["modes"][:2], np.stack([m1 @ Q, m2 @ Q]))
    print("principal angles:", angles)
    assert np.all(angles <= ANGLE_BOUND)


@pytest.mark.parametrize("weighted", [False, True])
def test_model_algebra(weighted):
    w, m = noisy_case(weighted)
    K = len(m["eigenvalues"])
    assert K == S_CPU - 1 and np.all(np.diff(m["eigenvalues"]) <= 0.0)
    gram = np.array([[ref.inner(m["modes"][i], m["modes"][j], w) for j in range(K)] for i in range(K)])
    assert np.max(np.abs(gram - np.eye(K))) <= 1e-12
    lead = np.sqrt(m["eigenvalues"][0])
    assert np.max(np.abs(m["scores"] - np.sqrt((S_CPU - 1) * m["eigenvalues"])[None] * m["vectors"].T)) <= 1e-12 * lead
    for s in (0, 7):
        b = ref.project(m, m["aligned"][s], w, align=False)
        assert np.max(np.abs(b - m["scores"][s])) <= 1e-12 * lead
        assert np.max(np.abs(ref.reconstruct(m, b) - m["aligned"][s])) <= 1e-12 * ref.rms_size(m["mean"])
    assert abs(m["explained_variance_ratio"].sum() - 1.0) <= 1e-12
    for k in range(K):  # the component of largest magnitude of every eigenvector is positive
        assert m["vectors"][k][np.argmax(np.abs(m["vectors"][k]))] > 0.0


def test_weights_change_the_mean():
    assert not np.array_equal(noisy_case(False)[1]["mean"], noisy_case(True)[1]["mean"])
    P, F = blob(), np.asarray(blob_mesh(700, seed=0).faces)
    areas = ref.vertex_areas(P, F)
    assert np.all(areas > 0.0)
    g = ref.generalized_procrustes(noisy_population(), weights=areas, tol=1e-12, max_iter=50)
    assert g["converged"] and not np.array_equal(g["mean"], noisy_case(False)[1]["mean"])


def test_model_object_on_host_arrays():
    """`ShapeModel`'s host-side methods over the reference's arrays (no device)."""
    w, m = noisy_case(False)
    model = shape_model.ShapeModel(m["mean"], m["modes"], m["eigenvalues"], m["scores"], m["explained_variance_ratio"])
    assert model.n_modes == S_CPU - 1
    assert np.array_equal(model.reconstruct(m["scores"][2]), ref.reconstruct(m, m["scores"][2]))
    assert model.reconstruct(m["scores"][:, :3]).shape == (S_CPU, 700, 3)
    assert np.allclose(model.compactness()[-1], 1.0) and np.all(np.diff(model.compactness()) > 0.0)
    drawn = model.sample(np.random.default_rng(3), 5)
    assert drawn.shape == (5, 700, 3) and np.array_equal(drawn, model.sample(np.random.default_rng(3), 5))
    mesh = blob_mesh(700, seed=0)
    moved = model.mode_on_mesh(mesh, 1, -2.0)
    assert isinstance(moved, PolyMesh) and moved is not mesh and np.array_equal(moved.faces, mesh.faces)
    assert np.array_equal(moved.points, m["mean"] + (-2.0 * np.sqrt(m["eigenvalues"][1])) * m["modes"][1])
    with pytest.raises(ValueError):
        model.mode_on_mesh(mesh, S_CPU, 1.0)
    with pytest.raises(ValueError):
        model.reconstruct(np.zeros(S_CPU))


# ---- GPU: the primitives against the reference, bit for bit ----------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    _hip.load_library()
    return _hip.default_context()


def _population(S, n, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((S, n, 3)) * np.array([1.0, 0.6, 0.3]) + 0.3 * rng.standard_normal((S, 1, 3))
    return np.ascontiguousarray(X + offset)


def _weights(kind, n, seed):
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(n)
    w = np.random.default_rng(seed + 100).uniform(0.2, 2.0, n)
    if kind == "zeros":
        w[::3] = 0.0
        w[n // 2:n // 2 + 300] = 0.0  # a whole run of the tree adds nothing
        w[n - 1] = 1.5  # (W > 0 also at n = 1 and 2)
    return w


def _every_primitive(dev, seed):
    """Every primitive once on `dev` (a `_hip.DeviceShapes` or a `ref.RefShapes`), in an order in which each sees the work
    of the ones before: a dict of every output."""
    S, n = dev.S, dev.n
    rng = np.random.default_rng(seed + 1000)
    R = np.stack([rng.uniform(0.5, 1.5) * ref.random_rotation(rng) for _ in range(S)])
    scale, t = rng.uniform(0.5, 2.0, S), rng.standard_normal((S, 3))
    modes = rng.standard_normal((19 if S >= 16 else 3, n, 3))  # not derived from the population; 19: two tiles of modes
    other = rng.standard_normal((n, 3))
    first, count = (S // 3, S - S // 3 - (1 if S > 2 else 0)) if S > 1 else (0, 1)
    out = {"W": dev.weight_sum, "centroids": dev.center()}
    out["centred"] = dev.download()
    out["mean_of_one"], out["change_of_one"] = dev.mean(0, 1)
    out["H"], out["q"], out["rho2"] = dev.align_sums()
    dev.transform(R, scale)
    out["transformed"] = dev.download()
    out["mean"], out["change"] = dev.mean()
    out["no_mean"], out["change_of_none"] = dev.mean(first, count, return_mean=False)
    out["mean_of_some"], out["change_of_some"] = dev.mean(first, count)
    dev.transform(R[::-1].copy(), None, t)
    out["moved"] = dev.download()
    out["gram"] = dev.gram()
    out["combine_1"] = dev.combine(rng.standard_normal((1, S)))
    out["combine_S"] = dev.combine(rng.standard_normal((S, S)))
    out["scores"] = dev.scores(modes)
    dev.set_reference(other)
    out["gram_other"] = dev.gram()
    out["H_other"], out["q_other"], out["rho2_other"] = dev.align_sums()
    return out


def _same_bits(got, want, where):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        if want[name] is None:
            assert got[name] is None, (where, name)
            continue
        g, w = np.asarray(got[name], dtype=np.float64), np.asarray(want[name], dtype=np.float64)
        assert g.shape == w.shape, (where, name)
        assert np.array_equal(g.view(np.int64), w.view(np.int64)), (where, name, float(np.max(np.abs(g - w))))


@functools.lru_cache(maxsize=None)
def _reference_run(S, n, kind, offset):
    X, w = _population(S, n, S * 1000 + n, offset), _weights(kind, n, n)
    want = _every_primitive(ref.RefShapes(X, w), S + n)
    assert np.array_equal(want["mean_of_one"], want["centred"][0]) and np.array_equal(want["gram"], want["gram"].T)
    return X, w, want


def _device_run(ctx, X, w, seed):
    with _hip.DeviceShapes(X, w, ctx=ctx) as dev:
        return _every_primitive(dev, seed)


N_SIZES = (1, 2, 255, 256, 257, 65535, 65536, 65537)  # a run's edge, the second level's, the third level's
S_SIZES = (1, 2, 16, 17, 33)  # (S = 3 runs with every n) both sides of a 16-wide tile of pairs, three tiles
CASES = [(3, n, "random", 0.0) for n in N_SIZES] + [(S, 257, "random", 0.0) for S in S_SIZES] + [
    (3, 257, "none", 0.0), (3, 65537, "none", 0.0), (17, 257, "zeros", 0.0), (3, 65537, "zeros", 0.0),
    (3, 257, "random", 1e6), (3, 65537, "none", 1e6), (17, 300, "random", 1e6)]  # the centroid about 1e6 sizes away


@pytest.mark.gpu
@pytest.mark.parametrize("S, n, kind, offset", CASES)
def test_every_primitive_equals_the_reference(ctx, S, n, kind, offset):
    X, w, want = _reference_run(S, n, kind, offset)
    _same_bits(_device_run(ctx, X, w, S + n), want, "first call")
    _same_bits(_device_run(ctx, X, w, S + n), want, "second call")
    if kind == "none":  # no weights are weights of 1.0
        _same_bits(_device_run(ctx, X, np.ones(n), S + n), want, "explicit ones")


@pytest.mark.gpu
@pytest.mark.parametrize("S, n", [(3, 65537), (17, 257), (33, 257), (3, 255)])
def test_both_forms_of_the_pair_sums_give_the_reference(ctx, monkeypatch, S, n):
    """The Gram and the scores with their partial sums per 256 vertices (the default at these sizes) and carried over
    65 536 vertices per block (forced: PF_SHAPES_LEVEL1_MAX=0)."""
    X, w, want = _reference_run(S, n, "random", 0.0)
    monkeypatch.setenv("PF_SHAPES_LEVEL1_MAX", "0")
    _same_bits(_device_run(ctx, X, w, S + n), want, "carried")
    monkeypatch.setenv("PF_SHAPES_LEVEL1_MAX", str(2**40))
    _same_bits(_device_run(ctx, X, w, S + n), want, "per run")


@pytest.mark.gpu
def test_pool_contents_change_nothing(ctx):
    """The pattern of tests/test_pool_hygiene.py: plain, every pool block poisoned with 0xFF and with 0x00 first, and after a
    larger neighbour on the same ctx whose blocks the pool recycles.  The same bits, which are the reference's: no element
    of a partial sum or of an output is read before it is written."""
    lib = _hip.load_library()
    cases = [(17, 257, "zeros", 0.0), (3, 65537, "none", 0.0)]
    big = _population(40, 700, 7)
    try:
        for mode in (0, 1, 2):
            assert lib.pf_pool_poison(mode) == 0
            for S, n, kind, offset in cases:
                X, w, want = _reference_run(S, n, kind, offset)
                _same_bits(_device_run(ctx, X, w, S + n), want, "poison %d" % mode)
    finally:
        lib.pf_pool_poison(0)
    _device_run(ctx, big, np.full(700, 3.0), 1)
    X, w, want = _reference_run(*cases[0])
    _same_bits(_device_run(ctx, X, w, 17 + 257), want, "after a larger neighbour")


@pytest.mark.gpu
def test_error_codes(ctx):
    lib = _hip.load_library()
    f64p = C.POINTER(C.c_double)

    def p(a):
        return None if a is None else a.ctypes.data_as(f64p)

    def create(X, S, n, w=None):
        h = C.c_void_p()
        code = lib.pf_shapes_create(ctx._h, p(X), S, n, p(w), C.byref(h))
        assert (code == 0) == bool(h)
        if h:
            lib.pf_shapes_free(h)
        return code

    X = _population(3, 40, 1)
    bad, ones = X.copy(), np.ones(40)
    bad[1, 7, 2] = np.inf
    assert create(X, 3, 40) == 0
    for S, n in ((0, 40), (-1, 40), (1025, 1), (3, 0), (3, -4), (1, 2**31)):
        assert create(X, S, n) == -1, (S, n)
    assert create(bad, 3, 40) == -1
    for value in (-1.0, np.nan, np.inf):
        w = ones.copy()
        w[5] = value
        assert create(X, 3, 40, w) == -1, value
    assert create(X, 3, 40, np.zeros(40)) == _hip.PF_E_DEGENERATE
    assert create(None, 3, 40) == -1

    with _hip.DeviceShapes(X, ones, ctx=ctx) as dev:
        before = dev.download()
        out, one = np.empty((3, 40, 3)), np.empty(1)
        for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (1, -1)):
            assert lib.pf_shapes_mean(dev._h, first, count, None, p(one)) == -1, (first, count)
        for K in (0, 4, -1):
            assert lib.pf_shapes_combine(dev._h, p(np.ones((4, 3))), K, p(np.empty((4, 40, 3)))) == -1, K
        for K in (0, 1025, -1):
            assert lib.pf_shapes_scores(dev._h, p(np.ones((1, 40, 3))), K, p(np.empty((3, 1025)))) == -1, K
        R, scale, t = np.tile(np.eye(3), (3, 1, 1)), np.ones(3), np.zeros((3, 3))
        for which in range(3):
            args = [R.copy(), scale.copy(), t.copy()]
            args[which].flat[2] = np.nan
            assert lib.pf_shapes_transform(dev._h, p(args[0]), p(args[1]), p(args[2])) == -1, which
        nan_modes, nan_coeff, nan_ref = np.ones((1, 40, 3)), np.ones((1, 3)), np.zeros((40, 3))
        nan_modes[0, 3, 1] = nan_coeff[0, 1] = nan_ref[9, 0] = np.nan
        assert lib.pf_shapes_scores(dev._h, p(nan_modes), 1, p(np.empty((3, 1)))) == -1
        assert lib.pf_shapes_combine(dev._h, p(nan_coeff), 1, p(out)) == -1
        assert lib.pf_shapes_set_reference(dev._h, p(nan_ref)) == -1
        assert lib.pf_shapes_gram(dev._h, None) == -1 and lib.pf_shapes_center(None, None) == -1
        assert b"not finite" in lib.pf_last_error() or b"NULL" in lib.pf_last_error()
        # nothing was launched: the population and the reference (zeros) are as they were
        assert np.array_equal(dev.download(), before)
        assert np.array_equal(dev.mean(0, 1)[1], tree_sum(dot_self(before[0])))


def dot_self(x):
    return ref.dot3(x, x)


# ---- GPU: the algorithm end to end -----------------------------------------------------------------------------------
def _end_to_end_population(which):
    if which == "similarity":
        return similarity_case(True)[0]
    if which == "rigid":
        return similarity_case(False)[0]
    if which == "planted":
        return planted_case()[0]
    return noisy_population()


@pytest.mark.gpu
@pytest.mark.parametrize("which, scaling, weighted", [("similarity", True, False), ("rigid", False, False), ("planted", False, False),
                                                      ("planted", True, True), ("noisy", True, True), ("noisy", False, False)])
def test_alignment_and_model_equal_the_reference(ctx, which, scaling, weighted):
    pop = _end_to_end_population(which)
    w = weights_700() if weighted else None
    options = dict(scaling=scaling, tol=1e-12, max_iter=50)
    want = ref.build_shape_model(pop, weights=w, **options)
    got = shape_model.generalized_procrustes(pop, w, ctx=ctx, **options)
    assert got.n_iter == want["n_iter"] and got.converged == want["converged"]
    _same_bits({k: getattr(got, k) for k in ("aligned", "mean", "transforms", "history")},
               {k: want[k] for k in ("aligned", "mean", "transforms", "history")}, "generalized_procrustes")
    aligned, mean, transforms, history = got  # (it unpacks)
    assert aligned is got.aligned and history is got.history
    model = shape_model.build_shape_model(pop, w, ctx=ctx, **options)
    _same_bits({k: getattr(model, k) for k in ("mean", "transforms", "eigenvalues", "modes", "scores", "explained_variance_ratio", "history")},
               {k: want[k] for k in ("mean", "transforms", "eigenvalues", "modes", "scores", "explained_variance_ratio", "history")},
               "build_shape_model")
    few = shape_model.build_shape_model(pop, w, n_modes=2, ctx=ctx, **options)
    assert few.n_modes == 2 and np.array_equal(few.modes, want["modes"][:2]) and np.array_equal(few.scores, want["scores"][:, :2])


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_projection_of_a_held_out_copy(ctx, weighted):
    w, want = noisy_case(weighted)
    model = shape_model.build_shape_model(noisy_population(), w, tol=1e-12, max_iter=50, ctx=ctx)
    rng = np.random.default_rng(8)
    copy = np.ascontiguousarray(1.2 * noisy_population()[4] @ ref.random_rotation(rng).T + np.array([3.0, -2.0, 5.0]))
    for align in (True, False):
        b = model.project(copy, align=align, ctx=ctx)
        assert np.array_equal(b, ref.project(want, copy, w, align=align))
    b = model.project(copy, ctx=ctx)
    assert np.max(np.abs(b - model.scores[4])) <= 1e-9 * np.sqrt(model.eigenvalues[0])  # the training shape's own scores
    assert np.max(np.abs(model.reconstruct(model.scores[4]) - want["aligned"][4])) <= 1e-12


@pytest.mark.gpu
def test_device_time_is_reported_on_request(ctx):
    with _hip.DeviceShapes(_population(5, 3000, 2), ctx=ctx) as dev:
        assert dev.device_ms(True) == 0.0
        dev.gram()
        assert dev.device_ms(False) > 0.0
