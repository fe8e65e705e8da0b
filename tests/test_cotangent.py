"""Cotangent Laplace-Beltrami operator: `pf_graph_build_cotan` and friends, `pyfocusr_amd.laplace_beltrami`,
`Graph(..., laplacian="cotangent")`, `Focusr(..., laplacian="cotangent")`.

CPU: the yardstick itself (`_cotan_ref`, numpy float64 in the device's summation orders) against closed forms.
GPU: the device assembly against it; the spectrum against scipy's shift-invert `eigsh` on the reference matrices; the
covariances the inverse-length operator does not have (scale, rigid motion, renumbering); the public interface.

Bounds.  A cotangent (u . v) / |u x v| carries a few ulp of relative error and eps |u||v| / |u x v| = eps / sin(theta) of
absolute error from the cancellation in the dot product (|cot| <= 1 / sin): |w_ij - ref| <= 16 eps sum_f 1 / sin(theta_f)
over the edge's faces (`w_bound`), the same summed over the row for d_i; m_i is a sum of positive areas: 8 eps m_i.
Eigenvalues: rtol 1e-8, what the general-matrix solver is held to elsewhere (test_gpu_parity); residuals 1e-10 scaled by
the operator's top."""
import numpy as np
import pytest
from scipy import sparse

import _cotan_ref as cr

EPS = cr.EPS
K = 6


# ------------------------------------------------------------------------------------------------------ meshes
def tetrahedron(a=1.0):
    pts = a / np.sqrt(8.0) * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return pts, faces


_meshes = {}


def mesh(name):
    """(points, faces), built once."""
    if name not in _meshes:
        from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

        if name == "tetra":
            _meshes[name] = tetrahedron(1.7)
        elif name == "blob700":
            m = blob_mesh(700, seed=0)
            _meshes[name] = (m.points, m.faces)
        elif name == "open700":  # 40 faces removed: boundary edges
            m = blob_mesh(700, seed=0)
            keep = np.ones(len(m.faces), dtype=bool)
            keep[np.random.default_rng(5).choice(len(m.faces), size=40, replace=False)] = False
            _meshes[name] = (m.points, m.faces[keep])
        elif name == "messy900":  # fins, flipped faces, stranded vertices
            m = messy_blob_mesh(900, seed=0)
            _meshes[name] = (m.points, m.faces)
        elif name == "blob5000":  # more than one 4096-row pad block, many SELL slices
            m = blob_mesh(5000, seed=0)
            _meshes[name] = (m.points, m.faces)
        elif name == "two_blobs":  # 700 + 900 far apart, plus 3 points no face references
            a, b = blob_mesh(700, seed=0), blob_mesh(900, seed=1)
            extra = np.array([[500.0, 0.0, 0.0], [0.0, 500.0, 0.0], [0.0, 0.0, 500.0]])
            pts = np.concatenate([a.points, extra[:1], b.points + np.array([1000.0, 0.0, 0.0]), extra[1:]])
            _meshes[name] = (pts, np.concatenate([a.faces, b.faces + 701]).astype(np.int32))
        else:
            raise KeyError(name)
    return _meshes[name]


_refs = {}


def reference(name):
    if name not in _refs:
        _refs[name] = cr.assemble(*mesh(name))
    return _refs[name]


_ref_eigs = {}


def reference_eigs(name):
    if name not in _ref_eigs:
        _ref_eigs[name] = cr.generalized_eigs(reference(name), K)
    return _ref_eigs[name]


def poly(name):
    from pyfocusr_amd import PolyMesh

    return PolyMesh(*mesh(name))


# ------------------------------------------------------------------------------------------------------ CPU
def test_reference_regular_tetrahedron():
    a = 1.7
    ref = cr.assemble(*tetrahedron(a))
    assert np.array_equal(ref["rowptr"], [0, 3, 6, 9, 12])
    np.testing.assert_allclose(ref["w"], 1.0 / np.sqrt(3.0), rtol=1e-14)  # two faces x 1/2 cot 60
    np.testing.assert_allclose(ref["mass"], a * a * np.sqrt(3.0) / 4.0, rtol=1e-14)
    L, _ = cr.matrices(ref)
    assert np.max(np.abs(L @ np.ones(4))) <= 1e-15
    np.testing.assert_allclose(ref["total_area"], a * a * np.sqrt(3.0), rtol=1e-14)


def test_reference_unit_square():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    ref = cr.assemble(pts, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    W = sparse.csr_matrix((ref["w"], ref["colidx"], ref["rowptr"]), shape=(4, 4)).toarray()
    assert abs(W[0, 2]) <= 1e-16 and abs(W[2, 0]) <= 1e-16  # the diagonal lies opposite two right angles
    for i, j in ((0, 1), (1, 2), (2, 3), (3, 0)):
        np.testing.assert_allclose([W[i, j], W[j, i]], 0.5, rtol=1e-15)  # opposite one angle of 45 degrees
    assert W[1, 3] == 0.0 and W[3, 1] == 0.0
    np.testing.assert_allclose(ref["mass"], [1.0 / 3.0, 1.0 / 6.0, 1.0 / 3.0, 1.0 / 6.0], rtol=1e-15)


def test_reference_blob_is_symmetric_positive_semidefinite():
    ref = reference("blob700")
    L, M = cr.matrices(ref)
    assert (L != L.T).nnz == 0
    rng = np.random.default_rng(0)
    for _ in range(20):
        x = rng.normal(size=L.shape[0])
        assert x @ (L @ x) >= -1e-12 * np.linalg.norm(L @ x) * np.linalg.norm(x)
    _, area, _ = cr.face_terms(*mesh("blob700"))
    np.testing.assert_allclose(ref["mass"].sum(), area.sum(), rtol=1e-13)
    np.testing.assert_allclose(ref["total_area"], area.sum(), rtol=1e-13)
    assert np.min(ref["w"]) < 0.0  # obtuse angles exist and are kept


def test_reference_refuses_degenerate_faces():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    with pytest.raises(cr.Degenerate):
        cr.assemble(pts, np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32))
    with pytest.raises(cr.Degenerate):
        cr.assemble(pts, np.array([[0, 1, 1], [0, 1, 3]], dtype=np.int32))


def test_laplacian_keyword_is_validated_before_any_device_call(monkeypatch):
    from pyfocusr_amd import Graph, _hip

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "DeviceLaplacian", no_device)
    monkeypatch.setattr(_hip, "default_context", no_device)
    with pytest.raises(ValueError):
        Graph(poly("tetra"), laplacian="x", verbose=False)
    assert Graph(poly("tetra"), verbose=False).laplacian == "inverse_length"
    assert Graph(poly("tetra"), laplacian="cotangent", verbose=False).laplacian == "cotangent"


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def devices(hip, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = hip.DeviceLaplacian(*mesh(name), ctx=ctx, cotangent=True)
        return cache[name]

    yield get
    for d in cache.values():
        d.close()


ASSEMBLY = ["tetra", "blob700", "open700", "messy900", "blob5000"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ASSEMBLY)
def test_assembly_against_reference(devices, name):
    dev, ref = devices(name), reference(name)
    h, c = dev.download(), dev.cotan_download()
    assert np.array_equal(h["rowptr"], ref["rowptr"]) and np.array_equal(h["colidx"], ref["colidx"])
    err_w = np.abs(c["w"] - ref["w"])
    bound_w = 16 * EPS * ref["w_bound"]
    rows = ref["rows"]
    row_bound = np.zeros(dev.n)
    np.add.at(row_bound, rows, bound_w)
    print(name, "max w err / bound", np.max(err_w / bound_w), "diag", np.max(np.abs(c["diag"] - ref["diag"]) / np.maximum(row_bound, 1e-300)),
          "mass", np.max(np.abs(c["mass"] - ref["mass"]) / np.maximum(ref["mass"], 1e-300)) / EPS, "eps")
    assert np.all(err_w <= bound_w)
    assert np.all(np.abs(c["diag"] - ref["diag"]) <= row_bound)
    assert np.all(np.abs(c["mass"] - ref["mass"]) <= 8 * EPS * ref["mass"])
    assert np.array_equal(dev.mass, c["mass"])
    off, sdiag, hi = cr.symmetric_operator(ref)
    np.testing.assert_allclose(dev.hi, hi, rtol=1e-13)
    np.testing.assert_allclose(dev.total_area, ref["total_area"], rtol=1e-13)
    # the stored operator: symmetric bit for bit
    assert dev.symmetric and dev.info.is_symmetric == 1 and dev.n_oneway == 0
    n = dev.n
    S = sparse.csr_matrix((-h["w"], h["colidx"], h["rowptr"]), shape=(n, n))
    assert (S != S.T).nnz == 0
    Wc = sparse.csr_matrix((c["w"], h["colidx"], h["rowptr"]), shape=(n, n))
    assert (Wc != Wc.T).nnz == 0
    np.testing.assert_allclose(-h["w"], off, rtol=1e-12, atol=1e-12 * hi)
    np.testing.assert_allclose(h["deg"], sdiag, rtol=1e-12, atol=1e-12 * hi)
    assert dev.n_isolated == ref["n_unreferenced"]
    assert np.all(c["mass"][np.diff(ref["rowptr"]) == 0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob700", "messy900", "blob5000"])
def test_two_builds_are_bit_identical(hip, ctx, devices, name):
    a = devices(name)
    b = hip.DeviceLaplacian(*mesh(name), ctx=ctx, cotangent=True)
    try:
        ha, hb, ca, cb = a.download(labels=True), b.download(labels=True), a.cotan_download(), b.cotan_download()
        for key in ha:
            assert np.array_equal(ha[key], hb[key]), key
        for key in ca:
            assert np.array_equal(ca[key], cb[key]), key
        assert a.hi == b.hi and a.total_area == b.total_area
    finally:
        b.close()


@pytest.mark.gpu
def test_assembly_errors(hip, ctx, devices):
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 3], [0, 1, 2]], dtype=np.int32), ctx=ctx, cotangent=True)  # a zero-area face
    assert e.value.code == hip.PF_E_DEGENERATE
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 3], [1, 1, 2]], dtype=np.int32), ctx=ctx, cotangent=True)
    assert e.value.code == hip.PF_E_DEGENERATE
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 2, 3]], dtype=np.int32), ctx=ctx, cotangent=True)  # a quad mesh
    assert e.value.code == -1
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 4]], dtype=np.int32), ctx=ctx, cotangent=True)
    assert e.value.code == -1
    plain = hip.DeviceLaplacian(*mesh("blob700"), ctx=ctx)
    try:
        for call in (plain.cotan_download, lambda: plain.cotan_apply(np.zeros(plain.n))):
            with pytest.raises(hip.PfError) as e:
                call()
            assert e.value.code == -1
        import ctypes as C

        assert plain._lib.pf_graph_cotan_info(plain._h, C.byref(C.c_double()), C.byref(C.c_double())) == -1
    finally:
        plain.close()
    with pytest.raises(hip.PfError):
        devices("blob700").cotan_apply(np.zeros((700, 9)))


# ---- spectrum
def check_spectrum(name, vals, vecs, hi):
    ref = reference(name)
    want, _, _ = reference_eigs(name)
    L, M = cr.matrices(ref)
    resid = np.max(np.abs(L @ vecs - (M @ vecs) * vals[None, :]))
    gram = np.max(np.abs(vecs.T @ (M @ vecs) - np.eye(len(vals))))
    print(name, "eig rel err", np.max(np.abs(vals - want) / want), "residual", resid, "/", 1e-10 * max(1.0, hi), "gram", gram)
    assert vals.shape == (K,) and vecs.shape == (len(ref["mass"]), K)
    np.testing.assert_allclose(vals, want, rtol=1e-8)
    assert resid <= 1e-10 * max(1.0, hi)
    assert gram <= 1e-10
    lead = vecs[np.argmax(np.abs(vecs), axis=0), np.arange(K)]
    assert np.all(lead > 0)  # Graph's sign convention


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob700", "open700", "blob5000"])
def test_spectrum_against_eigsh(ctx, devices, name):
    from pyfocusr_amd import laplace_beltrami_spectrum

    vals, vecs = laplace_beltrami_spectrum(poly(name), K, ctx=ctx)
    check_spectrum(name, vals, vecs, devices(name).hi)


@pytest.mark.gpu
def test_spectrum_of_two_components_and_stranded_points(ctx, devices):
    from pyfocusr_amd import laplace_beltrami_spectrum

    dev = devices("two_blobs")
    assert dev.n_components == 2 and dev.n_isolated == 3
    vals, vecs = laplace_beltrami_spectrum(poly("two_blobs"), K, ctx=ctx)
    from pyfocusr_amd.meshgen import blob_mesh

    b = blob_mesh(900, seed=1)
    own = np.sort(np.concatenate([reference_eigs("blob700")[0], cr.generalized_eigs(cr.assemble(b.points, b.faces), K)[0]]))
    print("two blobs", vals, own[:K])
    assert vals.shape == (K,)
    np.testing.assert_allclose(vals, own[:K], rtol=1e-8)
    assert np.all(vecs[[700, 1601, 1602]] == 0.0)
    ref = reference("two_blobs")
    L, M = cr.matrices(ref)
    assert np.max(np.abs(L @ vecs - (M @ vecs) * vals[None, :])) <= 1e-10 * max(1.0, dev.hi)
    assert np.max(np.abs(vecs.T @ (M @ vecs) - np.eye(K))) <= 1e-10


@pytest.mark.gpu
def test_null_vectors_are_sqrt_mass_per_component(devices):
    dev = devices("two_blobs")
    assert dev.lock_null_vectors() == 2
    got = dev.download_slots(0, 2)
    h = dev.download(labels=True)
    m = dev.mass
    for c in range(2):
        lab = np.unique(h["labels"][got[:, c] != 0.0])
        assert len(lab) == 1
        want = np.where((h["labels"] == lab[0]) & (m > 0), np.sqrt(m), 0.0)
        np.testing.assert_allclose(got[:, c], want / np.linalg.norm(want), rtol=1e-13, atol=0)
    assert np.all(got[[700, 1601, 1602]] == 0.0)
    # S annihilates them
    for c in range(2):
        assert np.max(np.abs(dev.spmv_host(np.ascontiguousarray(got[:, c])))) <= 1e-13 * dev.hi


# ---- covariances
@pytest.mark.gpu
def test_scaling_the_points_scales_the_spectrum(hip, ctx, devices):
    from pyfocusr_amd import PolyMesh, laplace_beltrami_spectrum

    pts, faces = mesh("blob700")
    a = devices("blob700")
    b = hip.DeviceLaplacian(2.0 * pts, faces, ctx=ctx, cotangent=True)
    try:
        ca, cb = a.cotan_download(), b.cotan_download()
        assert np.array_equal(ca["w"], cb["w"]) and np.array_equal(ca["diag"], cb["diag"])
        assert np.array_equal(4.0 * ca["mass"], cb["mass"])
    finally:
        b.close()
    va, _ = laplace_beltrami_spectrum(PolyMesh(pts, faces), K, ctx=ctx)
    vb, _ = laplace_beltrami_spectrum(PolyMesh(2.0 * pts, faces), K, ctx=ctx)
    np.testing.assert_allclose(vb, va / 4.0, rtol=1e-8)


@pytest.mark.gpu
def test_rigid_motion_and_renumbering_leave_the_spectrum(ctx):
    from pyfocusr_amd import PolyMesh, laplace_beltrami_spectrum

    pts, faces = mesh("blob700")
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    perm = rng.permutation(len(pts))  # new index of old vertex i
    moved = np.empty_like(pts)
    moved[perm] = pts @ q.T + np.array([3.0, -20.0, 7.5])
    va, _ = laplace_beltrami_spectrum(PolyMesh(pts, faces), K, ctx=ctx)
    vb, _ = laplace_beltrami_spectrum(PolyMesh(moved, perm[faces].astype(np.int32)), K, ctx=ctx)
    np.testing.assert_allclose(vb, va, rtol=1e-8)


# ---- public interface
@pytest.mark.gpu
def test_default_graph_is_unchanged(ctx):
    from pyfocusr_amd import Graph

    out = []
    for kw in ({}, {"laplacian": "inverse_length"}):
        np.random.seed(0)
        g = Graph(poly("blob700"), n_spectral_features=4, ctx=ctx, verbose=False, **kw)
        g.get_graph_spectrum()
        g.get_weighted_adjacency_matrix()
        out.append((g.eig_vals.copy(), np.array(g.eig_vecs), g.adjacency_matrix.data.copy()))
        assert g.mass is None
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_cotangent_graph(ctx, devices):
    from pyfocusr_amd import Graph, cotangent_laplacian, laplace_beltrami_spectrum, recursive_eig

    ref = reference("blob700")
    with pytest.raises(ValueError):
        Graph(poly("blob700"), laplacian="x", ctx=ctx, verbose=False)
    vals, vecs = laplace_beltrami_spectrum(poly("blob700"), K, ctx=ctx)
    raw = Graph(poly("blob700"), n_spectral_features=K, norm_eig_vecs=False, ctx=ctx, verbose=False, laplacian="cotangent")
    raw.get_graph_spectrum()
    np.testing.assert_allclose(raw.eig_vals, vals, rtol=1e-8)
    assert raw.eig_vecs.shape == (700, K)
    np.testing.assert_allclose(raw.eig_vecs, vecs, rtol=0, atol=1e-7 * np.max(np.abs(vecs)))
    g = Graph(poly("blob700"), n_spectral_features=K, ctx=ctx, verbose=False, laplacian="cotangent")
    g.get_graph_spectrum()
    np.testing.assert_allclose(g.eig_vals, vals, rtol=1e-8)
    lo = raw.eig_vecs.min(axis=0)
    np.testing.assert_allclose(g.eig_vecs, (raw.eig_vecs - lo) / (raw.eig_vecs.max(axis=0) - lo) - 0.5, rtol=0, atol=1e-7)
    assert g.eig_vecs.min() == -0.5 and g.eig_vecs.max() == 0.5
    # the reference-style attributes
    g.get_weighted_adjacency_matrix()
    g.get_degree_matrix()
    g.get_laplacian_matrix()
    c = devices("blob700").cotan_download()
    assert np.array_equal(g.adjacency_matrix.data, c["w"]) and np.array_equal(g.adjacency_matrix.indices, ref["colidx"])
    assert np.array_equal(g.degree_matrix.diagonal(), c["diag"]) and np.array_equal(g.mass, c["mass"])
    Lc, mass = cotangent_laplacian(poly("blob700"), ctx=ctx)
    assert np.array_equal(mass, c["mass"])
    assert (abs(Lc - (sparse.diags(c["diag"]) - g.adjacency_matrix)) > 0).nnz == 0
    want = sparse.diags(1.0 / c["mass"]) @ Lc
    assert abs(g.laplacian_matrix - want).max() <= 1e-15 * abs(want).max()
    rv, rvecs = recursive_eig(g.laplacian_matrix, k=K + 1, n_k_needed=K)
    np.testing.assert_allclose(rv, vals, rtol=1e-8)
    assert np.max(np.abs(g.laplacian_matrix @ rvecs - rvecs * rv[None, :])) <= 1e-10 * max(1.0, devices("blob700").hi)
    np.testing.assert_allclose(np.linalg.norm(rvecs, axis=0), 1.0, rtol=1e-12)


@pytest.mark.gpu
def test_mean_filter_uses_the_adjacency_matrix(ctx):
    from pyfocusr_amd import Graph

    g = Graph(poly("open700"), n_spectral_features=3, ctx=ctx, verbose=False, laplacian="cotangent")
    g.get_weighted_adjacency_matrix()
    W = g.adjacency_matrix
    values = np.random.default_rng(3).normal(size=(700, 3))
    D_inv = sparse.diags(1.0 / (1 + np.asarray(W.sum(axis=1))[:, 0]))
    average_mat = D_inv @ (W + sparse.eye(W.shape[0]))
    want = values
    for _ in range(5):
        want = average_mat @ want
    got = g.mean_filter_graph(values, iterations=5)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.max(np.abs(want)))


@pytest.mark.gpu
def test_focusr_with_cotangent_graphs(ctx):
    from pyfocusr_amd import Focusr
    from pyfocusr_amd.meshgen import blob_mesh

    np.random.seed(0)
    a, b = blob_mesh(700, seed=0), blob_mesh(800, seed=1)
    reg = Focusr(a, b, icp_register_first=False, list_features_to_calc=[], laplacian="cotangent", n_spectral_features=3,
                 n_extra_spectral=0, ctx=ctx)
    assert reg.graph_target.laplacian == "cotangent" and reg.graph_source.laplacian == "cotangent"
    reg.align_maps()
    idx = np.asarray(reg.corresponding_target_idx_for_each_source_pt)
    assert idx.shape == (800,) and idx.min() >= 0 and idx.max() < 700
    for name in ("weighted_avg_transformed_points", "nearest_neighbor_transformed_points"):
        out = getattr(reg, name)
        assert out.shape == (800, 3) and np.all(np.isfinite(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob700", "messy900"])
def test_mean_curvature_normals(ctx, name):
    from pyfocusr_amd import mean_curvature, mean_curvature_normals

    ref = reference(name)
    pts, _ = mesh(name)
    want, bound = cr.apply(ref, pts)
    got = mean_curvature_normals(poly(name), ctx=ctx)
    print(name, "max err / bound", np.max(np.abs(got - want) / np.maximum(16 * EPS * bound, 1e-300)))
    assert got.shape == (len(pts), 3)
    assert np.all(np.abs(got - want) <= 16 * EPS * bound)
    assert np.all(got[ref["mass"] == 0] == 0.0)
    assert np.array_equal(mean_curvature(poly(name), ctx=ctx), 0.5 * np.linalg.norm(got, axis=1))
    if name == "blob700":  # convex almost everywhere: sum_j w_ij (p_i - p_j) points away from the neighbours' plane, outward
        centre = pts.mean(axis=0)
        assert np.mean(np.einsum("ij,ij->i", got, pts - centre) > 0) > 0.9
