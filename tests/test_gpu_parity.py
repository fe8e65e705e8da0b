"""GPU parity tests: the HIP path, called through the C-ABI (ctypes), against the
oracle and the reference-generated golden fixtures.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
from scipy import sparse

from oracle import reference_port as orc

pytestmark = pytest.mark.gpu

MESHES = ["target_mesh", "source_mesh", "target_mesh_15k", "source_mesh_15k"]


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def devices(hip, golden, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            g = golden(name)
            cache[name] = hip.DeviceLaplacian(g["points"], g["faces"], ctx=ctx)
        return cache[name]

    return get


def mesh_of(g):
    from pyfocusr_amd import PolyMesh

    return PolyMesh(g["points"], g["faces"])


# ------------------------------------------------------------------------------- assembly
@pytest.mark.parametrize("name", MESHES)
def test_assembly_bit_exact(golden, devices, name):
    g, dev = golden(name), devices(name)
    h = dev.download(labels=True)
    assert np.array_equal(h["rowptr"], g["W_indptr"])
    assert np.array_equal(h["colidx"], g["W_indices"])
    assert np.array_equal(h["w"], g["W_data"])  # bit-exact 1/||xi-xj||
    assert np.array_equal(h["deg"], g["deg"])
    n = len(g["points"])
    W = sparse.csr_matrix((g["W_data"], g["W_indices"], g["W_indptr"]), shape=(n, n))
    assert dev.symmetric == (abs(W - W.T).nnz == 0)
    assert dev.n_isolated == int(np.sum(g["deg"] == 0))
    assert dev.nnz_l == len(g["L_data"])
    ncomp, labels = sparse.csgraph.connected_components(W + W.T, directed=False)
    sizes = np.bincount(labels)
    assert dev.n_components == int(np.sum(sizes > 1))
    # same partition
    assert len(set(zip(labels.tolist(), h["labels"].tolist()))) == ncomp


@pytest.mark.parametrize("name", MESHES)
def test_laplacian_view_bit_exact(golden, ctx, name):
    from pyfocusr_amd import Graph

    g = golden(name)
    gr = Graph(mesh_of(g), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_weighted_adjacency_matrix()
    gr.get_degree_matrix()
    gr.get_G_matrix()
    gr.get_laplacian_matrix()
    L = gr.laplacian_matrix
    assert np.array_equal(L.indptr, g["L_indptr"]) and np.array_equal(L.indices, g["L_indices"])
    assert np.array_equal(L.data, g["L_data"])
    assert np.array_equal(gr.degree_matrix_inv.diagonal(), g["d_inv"])
    A = gr.adjacency_matrix
    assert np.array_equal(A.data, g["W_data"]) and np.array_equal(A.indices, g["W_indices"])
    assert np.array_equal(gr.normed_points, g["normed_points"])


def test_assembly_hub_vertices(hip, ctx):
    """Vertices of very high degree: a fan of 6000 triangles around one hub (its row alone exceeds what a block stages in
    LDS for the per-vertex sort, so that block sorts in global memory) next to a second fan and a strip of ordinary
    triangles, in shuffled vertex order.  CSR(W), degrees and L against the oracle, bit for bit; the SELL operator through
    one product against scipy."""
    from oracle import reference_port as orc

    rng = np.random.default_rng(5)
    n_rim = 6000
    ang = np.linspace(0.0, 2.0 * np.pi, n_rim, endpoint=False)
    rim = np.stack([np.cos(ang) * (1 + 0.1 * rng.random(n_rim)), np.sin(ang), 0.05 * rng.standard_normal(n_rim)], axis=1)
    rim2 = rim * 0.5 + np.array([0.0, 0.0, 1.0])
    pts = np.concatenate([[[0.0, 0.0, 0.3]], rim, [[0.0, 0.0, 1.4]], rim2])
    hub2 = 1 + n_rim
    faces = [[0, 1 + i, 1 + (i + 1) % n_rim] for i in range(n_rim)]
    faces += [[hub2, hub2 + 1 + i, hub2 + 1 + (i + 1) % n_rim] for i in range(0, n_rim, 3)]  # an open fan: one-way edges too
    faces += [[1 + i, hub2 + 1 + i, 1 + (i + 1) % n_rim] for i in range(0, n_rim, 2)]       # joins the two fans
    faces = np.asarray(faces, dtype=np.int32)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    pts, faces = pts[perm], inv[faces].astype(np.int32)
    W, deg, d_inv, L = orc.graph_matrices(pts, faces)
    W, L = sparse.csr_matrix(W), sparse.csr_matrix(L)
    W.sort_indices()
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    try:
        h = dev.download()
        assert dev.max_degree >= n_rim
        assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices)
        assert np.array_equal(h["w"], W.data) and np.array_equal(h["deg"], deg)
        assert dev.symmetric == (abs(W - W.T).nnz == 0)
        x = rng.standard_normal(len(pts))
        y = dev.spmv_host(x, op=hip.PF_OP_RW)
        ref = L @ x
        assert np.max(np.abs(y - ref)) <= 1e-12 * np.max(np.abs(ref))
    finally:
        dev.close()


def test_assembly_piled_vertices(hip, ctx):
    """Nearly all vertices in ONE cell of the renumbering's Morton grid (a tiny sphere next to two far-away vertices that
    stretch the bounding box): the ordering by counting gives up, the build repeats it with the general sort in its one
    extra synchronisation, and the operator is the oracle's all the same."""
    from oracle import reference_port as orc
    from pyfocusr_amd.meshgen import blob_mesh

    # (a first build leaves out-of-range numbers in the allocator's cached blocks: whatever the abandoned ordering does not
    # write itself would be read as vertex indices by the kernels queued behind it)
    junk = hip.DeviceLaplacian(blob_mesh(40000, seed=30).points * 3.0, blob_mesh(40000, seed=30).faces, ctx=ctx)
    junk.close()
    m = blob_mesh(8000, seed=31)
    pts = np.concatenate([m.points * 1e-3, [[900.0, 0.0, 0.0], [0.0, -700.0, 0.0], [0.0, 0.0, 800.0]]])
    n0 = len(m.points)
    faces = np.concatenate([m.faces, [[n0, n0 + 1, n0 + 2], [0, n0, n0 + 1]]]).astype(np.int32)
    W, deg, d_inv, L = orc.graph_matrices(pts, faces)
    L = sparse.csr_matrix(L)
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    try:
        x = np.random.default_rng(3).standard_normal(len(pts))
        y = dev.spmv_host(x, op=hip.PF_OP_RW)
        ref = L @ x
        assert np.max(np.abs(y - ref)) <= 1e-12 * np.max(np.abs(ref))
        h = dev.download()
        Wc = sparse.csr_matrix(W)
        Wc.sort_indices()
        assert np.array_equal(h["rowptr"], Wc.indptr) and np.array_equal(h["colidx"], Wc.indices) and np.array_equal(h["w"], Wc.data)
    finally:
        dev.close()


def test_assembly_errors(hip, ctx):
    pts = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 1]], dtype=np.int32), ctx=ctx)
    assert e.value.code == -3
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(pts, np.array([[0, 1, 10]], dtype=np.int32), ctx=ctx)
    assert e.value.code == -1
    dup = pts.copy()
    dup[3] = dup[2]  # coincident vertices joined by an edge: 1/0
    with pytest.raises(hip.PfError) as e:
        hip.DeviceLaplacian(dup, np.array([[1, 2, 3], [4, 5, 6]], dtype=np.int32), ctx=ctx)
    assert e.value.code == -3
    bad = pts.copy()
    bad[5, 1] = np.nan
    with pytest.raises(hip.PfError):
        hip.DeviceLaplacian(bad, np.array([[4, 5, 6]], dtype=np.int32), ctx=ctx)
    hip.DeviceLaplacian(dup, np.array([[0, 1, 2], [4, 5, 6]], dtype=np.int32), ctx=ctx).close()  # duplicates not joined: fine


@pytest.mark.parametrize("seed", range(6))
def test_component_labels_random_soups(hip, ctx, seed):
    """Weakly connected components of random triangle soups (many small components, one-way edges, chains that
    snake through the index range, from_matrix graphs): every vertex is labelled with the smallest vertex index of
    its component, exactly as scipy's connected_components partitions it."""
    rng = np.random.default_rng(100 + seed)
    kind = seed % 3
    n = int(rng.integers(50, 8000 if kind == 0 else 40000))  # the library tracks at most 4096 components
    pts = rng.normal(size=(n, 3))
    if kind == 0:  # sparse soup: thousands of little components
        faces = rng.integers(0, n, size=(max(n // 4, 4), 3))
    elif kind == 1:  # strip in a random vertex order: one long chain through the index range + strays
        order = rng.permutation(n)[: n - n // 10]
        faces = np.stack([order[:-2], order[1:-1], order[2:]], axis=1)
    else:  # clusters joined by single triangles
        faces = rng.integers(0, n // 8, size=(n // 2, 3)) + (rng.integers(0, 8, size=(n // 2, 1)) * (n // 8))
        faces = np.concatenate([faces, rng.integers(0, n, size=(3, 3))])
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])].astype(np.int32)
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    h = dev.download(labels=True)
    W = sparse.csr_matrix((h["w"], h["colidx"], h["rowptr"]), shape=(n, n))
    ncomp, lab = sparse.csgraph.connected_components(W, directed=True, connection="weak")
    smallest = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    assert np.array_equal(h["labels"], smallest[lab])
    sizes = np.bincount(lab)
    has_row = np.diff(h["rowptr"]) > 0
    assert dev.n_components == int(np.sum(has_row[smallest]))  # components whose representative has a row of L
    assert dev.n_isolated == int(np.sum(~has_row))
    dev.close()


def test_assembly_quads_and_duplicates(hip, ctx):
    """Polygons with 4 vertices (VTK edge order) and a face listed twice (set semantics)."""
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(30, 3))
    faces = np.array([rng.choice(30, 4, replace=False) for _ in range(25)], dtype=np.int32)
    faces = np.concatenate([faces, faces[:5]])
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    W, deg, d_inv, L = orc.graph_matrices(pts, faces)
    h = dev.download()
    assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices)
    assert np.array_equal(h["w"], W.data) and np.array_equal(h["deg"], deg)


@pytest.mark.parametrize("seed", range(6))
def test_assembly_random_triangle_soups(hip, ctx, seed):
    """Non-manifold inputs: random faces over random points (one-way edges, directed edges shared by
    many faces, unreferenced vertices, hub vertices): W, deg and the scipy view of L stay bit-identical
    to the reference's set-semantics construction."""
    from pyfocusr_amd import Graph, PolyMesh

    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 400))
    n_faces = int(rng.integers(1, 4 * n))
    pts = rng.normal(size=(n, 3)) * rng.uniform(0.1, 50)
    faces = np.array([rng.choice(n, 3, replace=False) for _ in range(n_faces)], dtype=np.int32)
    if seed % 2:  # a hub: one vertex in many faces
        faces[: n_faces // 2, 0] = 0
        faces = faces[(faces[:, 1] != 0) & (faces[:, 2] != 0)]
    W, deg, d_inv, L = orc.graph_matrices(pts, faces)
    gr = Graph(PolyMesh(pts, faces), n_spectral_features=2, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_weighted_adjacency_matrix()
    gr.get_degree_matrix()
    gr.get_laplacian_matrix()
    A, Lg = gr.adjacency_matrix, gr.laplacian_matrix
    assert np.array_equal(A.indptr, W.indptr) and np.array_equal(A.indices, W.indices) and np.array_equal(A.data, W.data)
    assert np.array_equal(gr.degree_matrix.diagonal(), deg)
    assert np.array_equal(Lg.indptr, L.indptr) and np.array_equal(Lg.indices, L.indices) and np.array_equal(Lg.data, L.data)
    dev = gr.device
    assert dev.symmetric == (abs(W - W.T).nnz == 0) and dev.n_isolated == int(np.sum(deg == 0))
    assert dev.max_degree == int(np.diff(W.indptr).max())
    x = rng.standard_normal(n)
    y = dev.spmv_host(x, op=hip.PF_OP_RW)  # SELL storage after renumbering == the CSR it came from
    Lfull = sparse.csr_matrix(L)
    np.testing.assert_allclose(y, Lfull @ x, rtol=0, atol=1e-13 * max(1.0, np.abs(x).max()) * max(1, dev.max_degree))


# ------------------------------------------------------------------------------- operator kernels
def host_operator(g, dev):
    n = len(g["points"])
    L = sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))
    if not dev.symmetric:
        return L
    W = sparse.csr_matrix((g["W_data"], g["W_indices"], g["W_indptr"]), shape=(n, n))
    s = np.sqrt(1.0 / (g["deg"] + 1e-8))
    return (sparse.diags(s) @ (sparse.diags(g["deg"]) - W) @ sparse.diags(s)).tocsr()


@pytest.mark.parametrize("name", MESHES)
def test_spmv_and_cheb(golden, devices, hip, name):
    g, dev = golden(name), devices(name)
    n = dev.n
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n)
    L = sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))
    y = dev.spmv_host(x, op=hip.PF_OP_RW)
    ref = L @ x
    scale = abs(L) @ np.abs(x) + 1e-300
    assert np.max(np.abs(y - ref) / scale) < 4e-16
    A = host_operator(g, dev)
    if dev.symmetric:
        ys = dev.spmv_host(x, op=hip.PF_OP_SYM)
        # host S entries round differently from the device's (-W (s_i s_j)): a few ulp
        assert np.max(np.abs(ys - A @ x) / (abs(A) @ np.abs(x) + 1e-300)) < 2e-15
    # Chebyshev recurrence, degree 1, 2, 3 and 40
    dev.ws_ensure(4)
    dev.upload(0, x)
    c, e = 1.002, 0.998
    for p in (1, 2, 3, 40):
        dev.cheb(0, 1, p, c, e)
        got = dev.download_slots(1, 1)[:, 0]
        y0, y1 = x, (c * x - A @ x) / e
        for _ in range(p - 1):
            y0, y1 = y1, (2.0 / e) * (c * y1 - A @ y1) - y0
        assert np.max(np.abs(got - y1)) <= 1e-12 * np.max(np.abs(y1)), p
        assert np.array_equal(dev.download_slots(0, 1)[:, 0], x)  # src preserved
        rho = 1.3  # scaled recurrence: T_p / rho^p
        dev.cheb(0, 2, p, c, e, rho)
        np.testing.assert_allclose(dev.download_slots(2, 1)[:, 0], y1 / rho**p, rtol=1e-11, atol=1e-13 * np.max(np.abs(y1)) / rho**p)


def test_vector_kernels(golden, devices):
    dev = devices("source_mesh_15k")  # n = 14996: not a multiple of 256
    n = dev.n
    rng = np.random.default_rng(4)
    V = rng.standard_normal((n, 7))
    dev.ws_ensure(24)
    for b in range(7):
        dev.upload(b, V[:, b])
    assert np.array_equal(dev.download_slots(0, 7), V)
    w = V[:, 6]
    d = dev.dots(6, 0, 6)
    np.testing.assert_allclose(d, V[:, :6].T @ w, rtol=1e-12, atol=1e-10)
    # orth (CGS2) against an orthonormal basis
    Qb, _ = np.linalg.qr(V[:, :5])
    for b in range(5):
        dev.upload(b, Qb[:, b])
    dev.upload(8, w)
    h, nrm = dev.orth(8, 0, 5)
    np.testing.assert_allclose(h, Qb.T @ w, rtol=1e-11, atol=1e-11)
    r = w - Qb @ (Qb.T @ w)
    np.testing.assert_allclose(nrm, np.linalg.norm(r), rtol=1e-12)
    got = dev.download_slots(8, 1)[:, 0]
    assert np.max(np.abs(Qb.T @ got)) < 1e-12 * nrm
    dev.scale(8, 1.0 / nrm)
    np.testing.assert_allclose(np.linalg.norm(dev.download_slots(8, 1)), 1.0, rtol=1e-14)
    # combine with 11 output columns (two launches of 8 + 3)
    Y = rng.standard_normal((5, 11))
    dev.combine(0, 5, Y, 10)
    np.testing.assert_allclose(dev.download_slots(10, 11), Qb @ Y, rtol=0, atol=1e-13)
    dev.copy(10, 21, 2)
    assert np.array_equal(dev.download_slots(21, 2), dev.download_slots(10, 2))
    # resnorm
    np.testing.assert_allclose(dev.resnorm(0, 1, 0.37), np.linalg.norm(Qb[:, 0] - 0.37 * Qb[:, 1]), rtol=1e-13)
    # mask_isolated
    dev.upload(9, np.ones(n))
    dev.mask_isolated(9)
    z = dev.download_slots(9, 1)[:, 0]
    deg = golden("source_mesh_15k")["deg"]
    assert np.array_equal(z == 0, deg == 0) and dev.n_isolated == 2


def test_orth_one_pass_with_second_pass_on_demand(golden, devices):
    """pf_orth_begin / pf_orth_end: projection, Pythagorean norm and normalisation behind one batch of dot products; when
    the projection cancels digits (|w'| < 0.3 |w|) pf_orth_end runs the second Gram-Schmidt pass itself and says so
    (`pf_orth_redone`: a pipelined driver then repeats what it queued on the un-refined vector)."""
    dev = devices("source_mesh_15k")
    n = dev.n
    rng = np.random.default_rng(11)
    Qb, _ = np.linalg.qr(rng.standard_normal((n, 6)))
    dev.ws_ensure(12)
    for b in range(6):
        dev.upload(b, Qb[:, b])
    noise = rng.standard_normal(n)
    for label, w, expect_redo in (("random", rng.standard_normal(n), False),
                                  ("mild", Qb @ np.array([0.5, -0.3, 0.2, 0.1, 0.0, 0.4]) + 2.0 * noise / np.linalg.norm(noise), False),
                                  ("cancelling", 3.0 * Qb[:, 0] - 2.0 * Qb[:, 4] + 1e-7 * noise, True),
                                  ("inside the span", Qb @ np.arange(1.0, 7.0), True)):
        for normalize in (True, False):
            dev.upload(8, w)
            dev.orth_begin(8, 0, 6, normalize=normalize)
            h, nrm = dev.orth_end()
            assert dev.orth_redone == expect_redo, label
            r = w - Qb @ (Qb.T @ w)
            r = r - Qb @ (Qb.T @ r)
            np.testing.assert_allclose(h, Qb.T @ w, rtol=1e-12, atol=1e-12, err_msg=label)
            got = dev.download_slots(8, 1)[:, 0]
            if label == "inside the span":
                assert nrm < 1e-13 * np.linalg.norm(w)  # nothing left; the vector is not normalised (the driver stops)
                continue
            np.testing.assert_allclose(nrm, np.linalg.norm(r), rtol=1e-13 if not expect_redo else 1e-8, err_msg=label)
            scale = 1.0 / nrm if normalize else 1.0
            # orthogonal to the basis: ~eps |w| / |w'| after one pass, ~eps after two
            assert np.max(np.abs(Qb.T @ got)) < 1e-13 * np.linalg.norm(got) * (np.linalg.norm(w) / nrm if not expect_redo else 1.0)
            np.testing.assert_allclose(got, r * scale, rtol=0, atol=(1e-13 if not expect_redo else 1e-8) * np.linalg.norm(r * scale), err_msg=label)
            if normalize:
                np.testing.assert_allclose(np.linalg.norm(got), 1.0, rtol=1e-13)
    # the second pass queued with the first and run on the device's own verdict (pf_orth_device_passes; round 4: what the
    # Arnoldi driver of asymmetric graphs uses): same numbers, and what was queued BEHIND the step read the final vector
    dev.orth_device_passes(True)
    try:
        for label, w, twice in (("random", rng.standard_normal(n), False),
                                ("cancelling", 3.0 * Qb[:, 0] - 2.0 * Qb[:, 4] + 1e-7 * noise, True),
                                ("inside the span", Qb @ np.arange(1.0, 7.0), True)):
            dev.upload(8, w)
            dev.orth_begin(8, 0, 6, normalize=True)
            dev.copy(8, 9, 1)  # queued behind the step, before its result is collected: the pipelined driver's next application
            h, nrm = dev.orth_end()
            assert not dev.orth_redone and dev.orth_twice == twice, label
            r = w - Qb @ (Qb.T @ w)
            r = r - Qb @ (Qb.T @ r)
            np.testing.assert_allclose(h, Qb.T @ w, rtol=1e-12, atol=1e-12, err_msg=label)
            got = dev.download_slots(8, 2)
            assert np.array_equal(got[:, 0], got[:, 1]), label  # the copy saw the refined, normalised vector
            if label == "inside the span":
                assert nrm < 1e-13 * np.linalg.norm(w)
                continue
            np.testing.assert_allclose(nrm, np.linalg.norm(r), rtol=1e-13 if not twice else 1e-8, err_msg=label)
            assert np.max(np.abs(Qb.T @ got[:, 0])) < 1e-13 * (np.linalg.norm(w) / nrm if not twice else 1.0)
            np.testing.assert_allclose(np.linalg.norm(got[:, 0]), 1.0, rtol=1e-13)
        # a pair: one graph with the device passes, its partner without (the partner's blocks sit the second launches out)
        other = devices("target_mesh_15k")
        other.ws_ensure(12)
        Qo, _ = np.linalg.qr(rng.standard_normal((other.n, 4)))
        for b in range(4):
            other.upload(b, Qo[:, b])
        wo = Qo @ np.array([2.0, -1.0, 0.5, 0.25]) + 1e-6 * rng.standard_normal(other.n)
        w = 3.0 * Qb[:, 0] - 2.0 * Qb[:, 4] + 1e-7 * noise
        dev.upload(8, w)
        other.upload(8, wo)
        dev.orth_begin2((8, 0, 6, True), other, (8, 0, 4, True))
        h, nrm = dev.orth_end()
        ho, nrmo = other.orth_end()
        assert dev.orth_twice and not dev.orth_redone and other.orth_redone and not other.orth_twice
        np.testing.assert_allclose(h, Qb.T @ w, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ho, Qo.T @ wo, rtol=1e-12, atol=1e-12)
        for d_, Q_ in ((dev, Qb), (other, Qo)):
            got = d_.download_slots(8, 1)[:, 0]
            assert np.max(np.abs(Q_.T @ got)) < 1e-13 and abs(np.linalg.norm(got) - 1.0) < 1e-13
    finally:
        dev.orth_device_passes(False)
    # strict mode (pf_orth_strict: unfiltered / small solves): the classical threshold |w'| < 0.71 |w|
    w = Qb @ np.array([0.8, 0.0, 0.5, 0.0, 0.3, 0.0]) + 0.75 * noise / np.linalg.norm(noise)  # |w'| / |w| ~ 0.6
    for strict, expect_redo in ((False, False), (True, True), (False, False)):
        dev.orth_strict(strict)
        dev.upload(8, w)
        dev.orth_begin(8, 0, 6, normalize=True)
        h, nrm = dev.orth_end()
        assert dev.orth_redone == expect_redo
        r = w - Qb @ (Qb.T @ w)
        assert 0.5 < nrm / np.linalg.norm(w) < 0.7
        np.testing.assert_allclose(nrm, np.linalg.norm(r), rtol=1e-13)
        np.testing.assert_allclose(dev.download_slots(8, 1)[:, 0], r / np.linalg.norm(r), rtol=0, atol=1e-13)
    # an empty basis: just the norm
    dev.upload(8, noise)
    dev.orth_begin(8, 0, 0, normalize=True)
    h, nrm = dev.orth_end()
    assert len(h) == 0 and not dev.orth_redone
    np.testing.assert_allclose(nrm, np.linalg.norm(noise), rtol=1e-14)
    np.testing.assert_allclose(dev.download_slots(8, 1)[:, 0], noise / np.linalg.norm(noise), rtol=1e-14)


def test_spectral_bound_from_the_faces(golden, hip, ctx):
    """pf_graph_info.spectral_bound: for a closed triangle mesh (W symmetric, no directed edge listed twice) the
    face-by-face bound 1 + (1 + sqrt(1 - 4 P_min)) / 2 - equal to the numpy formula, above the true lambda_max of
    S = G^1/2 (D - W) G^1/2 (scipy), below 2; otherwise 2."""
    from scipy.sparse.linalg import eigsh

    from pyfocusr_amd.meshgen import blob_mesh

    def formula(points, faces):
        p = points[faces]
        w = [1.0 / np.linalg.norm(p[:, i] - p[:, (i + 1) % 3], axis=1) for i in range(3)]
        P = 2 * w[0] * w[1] * w[2] / ((w[0] + w[1]) * (w[0] + w[2]) * (w[1] + w[2]))
        return 1 + (1 + np.sqrt(max(1 - 4 * P.min(), 0.0))) / 2

    blob = blob_mesh(12000, seed=4)
    for name, pts, faces in (("target_mesh", golden("target_mesh")["points"], golden("target_mesh")["faces"]),
                             ("source_mesh", golden("source_mesh")["points"], golden("source_mesh")["faces"]),
                             ("blob", blob.points, blob.faces)):
        dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
        assert dev.symmetric and dev.nnz_w == 3 * len(faces), name
        np.testing.assert_allclose(dev.spectral_bound, formula(pts, faces), rtol=1e-11, err_msg=name)
        W = orc.weighted_adjacency(pts, faces)
        deg = np.asarray(W.sum(axis=1)).ravel()
        s = np.sqrt(1.0 / (deg + 1e-8))
        S = sparse.diags(s) @ (sparse.diags(deg) - W) @ sparse.diags(s)
        lam_max = float(eigsh(S.tocsc(), k=1, which="LA", return_eigenvectors=False)[0])
        assert lam_max < dev.spectral_bound < 1.9, (name, lam_max, dev.spectral_bound)
        dev.close()
    # not a closed manifold: one-way edges (bundled 15k meshes), a face listed twice, an open mesh -> the generic bound
    g15 = golden("target_mesh_15k")
    dev = hip.DeviceLaplacian(g15["points"], g15["faces"], ctx=ctx)
    assert not dev.symmetric and dev.spectral_bound == 2.0
    dev.close()
    dup = np.concatenate([blob.faces, blob.faces[:1]])
    dev = hip.DeviceLaplacian(blob.points, dup, ctx=ctx)
    assert dev.symmetric and dev.nnz_w == 3 * len(blob.faces) and dev.spectral_bound == 2.0
    dev.close()
    dev = hip.DeviceLaplacian(blob.points, blob.faces[:-50], ctx=ctx)  # a hole: boundary edges are one-way
    assert dev.spectral_bound == 2.0
    dev.close()


def test_null_vectors_and_finalize(golden, devices):
    for name in ("target_mesh", "source_mesh_15k"):
        g, dev = golden(name), devices(name)
        k = dev.lock_null_vectors()
        assert k == dev.n_components == 1
        v = dev.download_slots(0, 1)[:, 0]
        np.testing.assert_allclose(np.linalg.norm(v), 1.0, rtol=1e-14)
        expect = np.sqrt(g["deg"] + 1e-8) if dev.symmetric else np.ones(dev.n)
        expect = np.where(g["deg"] > 0, expect, 0.0)
        np.testing.assert_allclose(v, expect / np.linalg.norm(expect), rtol=1e-13, atol=0)
        dev.ws_ensure(4)
        dev.spmv(0, 1)
        assert np.max(np.abs(dev.download_slots(1, 1))) < 1e-15
    # finalize: unit norm, sign, min-max
    dev = devices("target_mesh")
    g = golden("target_mesh")
    rng = np.random.default_rng(5)
    X = rng.standard_normal((dev.n, 3))
    X[17, 1] = -9.0  # largest |entry| negative -> column flipped
    for b in range(3):
        dev.upload(b, X[:, b])
    s = np.sqrt(1.0 / (g["deg"] + 1e-8))
    raw = dev.finalize_vectors(0, 3, minmax=False)
    exp = X * s[:, None]
    exp /= np.linalg.norm(exp, axis=0)
    _, exp = orc.canonicalize(np.arange(3.0), exp)
    np.testing.assert_allclose(raw, exp, rtol=1e-13, atol=1e-16)
    assert raw[17, 1] > 0
    nrm = dev.finalize_vectors(0, 3, minmax=True)
    np.testing.assert_allclose(nrm, orc.minmax_normalize(exp), rtol=0, atol=1e-14)
    assert nrm.min() == -0.5 and nrm.max() == 0.5


def test_mean_filter(golden, devices):
    for name in ("target_mesh", "source_mesh_15k"):
        g, dev = golden(name), devices(name)
        n = dev.n
        W = sparse.csr_matrix((g["W_data"], g["W_indices"], g["W_indptr"]), shape=(n, n))
        ref = orc.mean_filter_graph(W, g["points"], iterations=25)
        got = dev.mean_filter(g["points"], 25)
        np.testing.assert_allclose(got, ref, rtol=1e-14, atol=0)
        one = dev.mean_filter(g["points"][:, 0].copy(), 3)
        np.testing.assert_allclose(one, orc.mean_filter_graph(W, g["points"][:, 0], iterations=3), rtol=1e-14)


# ------------------------------------------------------------------------------- eigensolver
@pytest.mark.parametrize("name,k", [("target_mesh", 6), ("source_mesh", 6), ("target_mesh", 3), ("source_mesh", 3),
                                    ("target_mesh_15k", 5), ("source_mesh_15k", 5)])
def test_spectrum_vs_reference(golden, ctx, name, k):
    """BASELINE configs C1/C2: eigenvalues within 1e-6 relative (north star; we hold 1e-8),
    eigenvectors equal up to the fixed sign convention."""
    from pyfocusr_amd import Graph

    g = golden(name)
    gr = Graph(mesh_of(g), n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    gv = g["k%d_eig_vals" % k]
    assert gr.eig_vals.shape == gv.shape  # 9 columns for source_mesh_15k (widen-and-retry)
    assert gr.eig_vecs.shape == g["k%d_eig_vecs" % k].shape
    np.testing.assert_allclose(gr.eig_vals, gv, rtol=1e-8)
    assert np.all(np.diff(gr.eig_vals) > 0)
    # tolerance = conditioning: both ARPACK's and our pairs carry residuals ~1e-10 on L; with eigenvalue
    # gaps ~3e-4 (15k, asymmetric W) that is ~3e-7 of eigenvector play, ~1e-9 on the clean 5k meshes.
    tol = 2e-9 if "15k" not in name else 5e-7
    assert np.max(np.abs(gr.eig_vecs - g["k%d_eig_vecs" % k])) < tol
    st = gr.eigs_stats
    assert st.residuals.max() < 1e-8
    gr2 = Graph(mesh_of(g), n_spectral_features=k, norm_eig_vecs=False, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr2.get_graph_spectrum()
    assert np.max(np.abs(gr2.eig_vecs - g["k%d_eig_vecs_raw" % k])) < tol
    np.testing.assert_allclose(np.linalg.norm(gr2.eig_vecs, axis=0), 1.0, rtol=1e-13)
    # true residuals against the reference's L
    n = len(g["points"])
    L = sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))
    R = L @ gr2.eig_vecs - gr2.eig_vecs * gr2.eig_vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-8


@pytest.mark.parametrize("n,k,seed", [(2000, 1, 11), (2000, 12, 12), (7000, 3, 13), (7000, 8, 14), (20000, 5, 15),
                                      (20000, 12, 16), (60000, 3, 17), (60000, 8, 18)])
def test_spectrum_sweep_vs_oracle(ctx, n, k, seed):
    """Sizes and k the bundled meshes do not cover: synthetic closed meshes against the oracle's scipy `eigs`
    (the reference's call) — eigenvalues to 1e-8 relative, eigenvectors up to sign within the conditioning of
    the pair (residual / gap), true residuals against the oracle's L."""
    from pyfocusr_amd import Graph
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    W, deg, d_inv, L = orc.graph_matrices(m.points, m.faces)
    vals, vecs = orc.canonicalize(*orc.recursive_eig(L, k + 1, k))
    gr = Graph(m, n_spectral_features=k, norm_eig_vecs=False, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    assert gr.eig_vals.shape == vals.shape
    np.testing.assert_allclose(gr.eig_vals, vals, rtol=1e-8)
    R = L @ gr.eig_vecs - gr.eig_vecs * gr.eig_vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-10
    Rref = L @ vecs - vecs * vals[None, :]
    gaps = np.minimum(np.diff(np.concatenate(([0.0], vals))), np.diff(np.concatenate((vals, [np.inf]))))
    gaps[-1] = vals[-1] - vals[-2] if k > 1 else vals[-1]  # the next eigenvalue up is unknown: use the gap below
    play = (np.linalg.norm(R, axis=0) + np.linalg.norm(Rref, axis=0)) / gaps
    err = np.max(np.abs(gr.eig_vecs - vecs), axis=0)
    assert np.all(err < 10 * play + 1e-12), (err, play)


def test_tiny_meshes(ctx):
    """n = 4 and n = 6: far below one wavefront; the solver runs unfiltered (scipy eigs refuses k >= n-1)."""
    from pyfocusr_amd import Graph, PolyMesh

    tet = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.3]], float), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))
    octa = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1.1, 0], [0, -1.2, 0], [0, 0, 1.3], [0, 0, -0.9]], float),
            np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))
    for (pts, faces), k in ((tet, 2), (tet, 3), (octa, 4)):
        gr = Graph(PolyMesh(pts, faces), n_spectral_features=k, n_rand_samples=100, ctx=ctx, verbose=False)
        gr.get_graph_spectrum()
        W, deg, d_inv, L = orc.graph_matrices(pts, faces)
        ev = np.sort(np.linalg.eigvals(L.toarray()).real)
        ev = ev[ev > 1e-10]
        np.testing.assert_allclose(gr.eig_vals, ev[:len(gr.eig_vals)], rtol=1e-10)
        assert gr.eig_vecs.shape == (len(pts), min(k, len(pts) - 1))
        R = L @ gr.eig_vecs  # eigenvectors are min-max normalised: check directions through the raw solve
        gr2 = Graph(PolyMesh(pts, faces), n_spectral_features=k, norm_eig_vecs=False, n_rand_samples=100, ctx=ctx, verbose=False)
        gr2.get_graph_spectrum()
        assert np.max(np.abs(L @ gr2.eig_vecs - gr2.eig_vecs * gr2.eig_vals[None, :])) < 1e-10


def test_recursive_eig_on_plain_scipy_matrices(golden):
    """graph.py:357-389 with matrices that do not come from `Graph`: the random-walk Laplacian of the
    fixtures (non-symmetric values), its symmetrised form, and a shifted copy without null vectors."""
    from pyfocusr_amd import recursive_eig

    g = golden("target_mesh")
    n = len(g["points"])
    L = sparse.csr_matrix((g["L_data"], g["L_indices"], g["L_indptr"]), shape=(n, n))
    vals, vecs = recursive_eig(L, k=7, n_k_needed=6)
    np.testing.assert_allclose(vals, g["k6_eig_vals"], rtol=1e-8)
    _, canon = orc.canonicalize(vals, vecs)
    assert np.max(np.abs(canon - g["k6_eig_vecs_raw"])) < 2e-9
    s = np.sqrt(1.0 / (g["deg"] + 1e-8))
    W = sparse.csr_matrix((g["W_data"], g["W_indices"], g["W_indptr"]), shape=(n, n))
    S = sparse.diags(s) @ (sparse.diags(g["deg"]) - W) @ sparse.diags(s)
    vals_s, vecs_s = recursive_eig(S, k=4, n_k_needed=3)  # symmetric: null vector is not constant -> found, then filtered
    np.testing.assert_allclose(vals_s, g["k3_eig_vals"], rtol=1e-8)
    R = S @ vecs_s - vecs_s * vals_s[None, :]
    assert np.max(np.abs(R)) < 1e-10
    vals_sh, _ = recursive_eig(L + 0.01 * sparse.eye(n), k=4, n_k_needed=3)
    np.testing.assert_allclose(vals_sh[:3], np.concatenate([[0.01], g["k3_eig_vals"][:2] + 0.01]), rtol=1e-8)
    with pytest.raises(ValueError):
        recursive_eig(sparse.csr_matrix(np.ones((3, 4))), k=2, n_k_needed=1)


def test_open_mesh_complex_spectrum(ctx):
    """An open surface (712 one-way boundary edges): complex low eigenvalues, reported like the reference
    reports them (real parts, conjugate pairs as repeated values); the ellipse filter path on the device."""
    from pyfocusr_amd import Graph, PolyMesh

    nx, ny = 100, 80
    r = np.random.default_rng(0)
    x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
    pts = np.stack([x, y, 0.3 * np.sin(x / 5) + 0.2 * np.cos(y / 7)], -1).reshape(-1, 3) + 0.05 * r.normal(size=(nx * ny, 3))
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    ref = orc.graph_spectrum(pts, faces, 5)
    gr = Graph(PolyMesh(pts, faces), n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    assert 2 * gr.device.n_oneway == abs(ref["W"] - ref["W"].T).nnz == 712 and not gr.device.symmetric
    m = min(len(gr.eig_vals), len(ref["eig_vals"]))
    assert m >= 5
    np.testing.assert_allclose(gr.eig_vals[:m], ref["eig_vals"][:m], rtol=1e-7)
    assert np.isclose(gr.eig_vals[0], gr.eig_vals[1], rtol=1e-9)
    assert np.all(np.isfinite(gr.eig_vecs)) and gr.eig_vecs.min() == -0.5 and gr.eig_vecs.max() == 0.5


@pytest.mark.parametrize("case", ["blob_with_holes", "four_components_and_strays", "thin_strip", "asymmetric_few"])
def test_spectrum_messy_meshes_vs_oracle(ctx, case):
    """Non-closed, multi-component and slightly asymmetric inputs at sizes where the automatic paths of the solver
    switch (null-vector locking, widen-and-retry, Arnoldi with complex outliers, ellipse filter): the eigenvalues
    the reference returns (scipy `eigs` in the oracle), in its column count."""
    from pyfocusr_amd import Graph, PolyMesh
    from pyfocusr_amd.meshgen import blob_mesh

    rng = np.random.default_rng(21)
    k = 5
    if case == "blob_with_holes":  # closed blob with three caps cut out: 59 one-way boundary edges and 32 vertices
        m = blob_mesh(8000, seed=5)  # left without faces (each one a null vector the reference widens k for: larger
        pts, faces = m.points, m.faces  # holes keep scipy's eigs busy for minutes)
        c = pts[faces].mean(axis=1)
        keep = np.ones(len(faces), dtype=bool)
        for centre in pts[[10, 2000, 7000]]:
            keep &= np.linalg.norm(c - centre, axis=1) > 3.0
        faces = faces[keep]
    elif case == "four_components_and_strays":
        parts = [blob_mesh(n, seed=30 + i) for i, n in enumerate((9000, 4000, 2500, 600))]
        pts = np.concatenate([p.points + 300.0 * i for i, p in enumerate(parts)] + [rng.normal(size=(4, 3))])
        off = np.cumsum([0] + [len(p.points) for p in parts])
        faces = np.concatenate([p.faces + off[i] for i, p in enumerate(parts)])
    elif case == "thin_strip":  # 400 x 12 open strip: long thin domain, many boundary edges
        nx, ny = 400, 12
        x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
        pts = np.stack([x, y, 0.5 * np.sin(x / 9.0)], -1).reshape(-1, 3) + 0.03 * rng.normal(size=(nx * ny, 3))
        idx = np.arange(nx * ny).reshape(nx, ny)
        a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
        faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    else:  # a closed mesh with a handful of faces removed: a few one-way edges, Arnoldi with a real low spectrum
        m = blob_mesh(12000, seed=6)
        pts, faces = m.points, np.delete(m.faces, [5, 900, 4000, 4001, 20000], axis=0)
    ref = orc.graph_spectrum(pts, faces, k)
    gr = Graph(PolyMesh(pts, faces), n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    m_ = min(len(gr.eig_vals), len(ref["eig_vals"]))
    assert m_ >= k
    if case == "four_components_and_strays":
        assert gr.device.n_components == 4 and gr.device.n_isolated == 4
        assert gr.eig_vals.shape == ref["eig_vals"].shape
    np.testing.assert_allclose(gr.eig_vals[:m_], ref["eig_vals"][:m_], rtol=2e-7)
    assert np.all(np.isfinite(gr.eig_vecs)) and gr.eig_vecs.min() >= -0.5 and gr.eig_vecs.max() <= 0.5


def test_paired_spectra_equal_single(golden, ctx):
    """Two graphs per kernel launch (pf_cheb2, different sizes and degrees) give bit-identical
    results to one graph per launch."""
    from pyfocusr_amd import Graph
    from pyfocusr_amd import graph as graph_mod
    from pyfocusr_amd.graph import compute_spectra

    assert graph_mod._pair_pays(*[Graph(mesh_of(golden(n)), ctx=ctx, verbose=False) for n in ("target_mesh", "source_mesh")])
    gs = [Graph(mesh_of(golden(n)), n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False)
          for n, k in (("target_mesh", 6), ("target_mesh_15k", 5))]
    compute_spectra(gs)
    for g, (n, k) in zip(gs, (("target_mesh", 6), ("target_mesh_15k", 5))):
        one = Graph(mesh_of(golden(n)), n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False)
        one.get_graph_spectrum()
        assert np.array_equal(g.eig_vals, one.eig_vals) and np.array_equal(g.eig_vecs, one.eig_vecs)
        assert g.eigs_stats.matvecs == one.eigs_stats.matvecs


def test_pair_build_side_by_side(golden, hip, ctx):
    """`pf_graph_build_device2` (two meshes assembled in shared launches, their independent chains forked onto the second
    stream): W, deg, L, the statistics and the solver-order operator equal to two single builds bit for bit - for meshes of different size, repeatedly (blocks released on one stream come back on the
    other), with other work queued in between; a bad mesh in either place fails cleanly."""
    from pyfocusr_amd.meshgen import blob_mesh

    from pyfocusr_amd import PolyMesh

    # (round 4: the two builds share their launches - pf_launch.h - where both ask for the same kernel; a torus of quads
    # beside a triangle mesh and a mesh below the counting sort's size beside a large one make the two lists of launches
    # part ways: no face bound for quads, the library sort for the small mesh)
    nu, nv = 180, 60
    uu, vv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    au, av = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
    torus = PolyMesh(np.stack([(3 + np.cos(av)) * np.cos(au), (3 + np.cos(av)) * np.sin(au), np.sin(av)], axis=-1).reshape(-1, 3),
                     np.stack([uu * nv + vv, ((uu + 1) % nu) * nv + vv, ((uu + 1) % nu) * nv + (vv + 1) % nv, uu * nv + (vv + 1) % nv],
                              axis=-1).reshape(-1, 4).astype(np.int32))
    cases = [(mesh_of(golden("target_mesh")), mesh_of(golden("source_mesh_15k"))),
             (blob_mesh(60000, seed=41), blob_mesh(20000, seed=42)),
             (blob_mesh(20000, seed=43), blob_mesh(60000, seed=44)),
             (torus, blob_mesh(20000, seed=47)),
             (blob_mesh(30000, seed=48), blob_mesh(3000, seed=49))]
    rng = np.random.default_rng(3)
    for rep in range(3):
        for ma, mb in cases:
            dm = [hip.DeviceMesh(m.points, m.faces, ctx=ctx) for m in (ma, mb)]
            pa, pb = hip.DeviceLaplacian.build_pair(*dm)
            for m, paired in ((ma, pa), (mb, pb)):
                single = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
                hp, hs = paired.download(labels=True), single.download(labels=True)
                for key in hs:
                    assert np.array_equal(hp[key], hs[key]), key
                assert (paired.symmetric, paired.n_isolated, paired.n_components, paired.max_degree, paired.n_oneway, paired.spectral_bound) == \
                       (single.symmetric, single.n_isolated, single.n_components, single.max_degree, single.n_oneway, single.spectral_bound)
                x = rng.standard_normal(m.points.shape[0])
                assert np.array_equal(paired.spmv_host(x), single.spmv_host(x))  # the solver-order SELL operator too
                single.close()
            ctx.knn1(rng.uniform(size=(2000, 3)), rng.uniform(size=(500, 3)))  # other users of the allocator in between
            pa.close()
            pb.close()
            for d in dm:
                d.close()
    good, bad = blob_mesh(3000, seed=45), blob_mesh(3000, seed=46)
    bad_faces = bad.faces.copy()
    bad_faces[7, 1] = 3000  # out of range
    for order in (0, 1):
        dm = [hip.DeviceMesh(good.points, good.faces, ctx=ctx), hip.DeviceMesh(bad.points, bad_faces, ctx=ctx)]
        with pytest.raises(hip.PfError):
            hip.DeviceLaplacian.build_pair(*(dm if order == 0 else dm[::-1]))
        ok = hip.DeviceLaplacian.build_pair(dm[0], dm[0])  # the library is in working order afterwards
        assert ok[0].n == 3000 and np.array_equal(ok[0].download()["w"], ok[1].download()["w"])
        for o in ok:
            o.close()
        for d in dm:
            d.close()


def test_pair_driver_in_c(golden, hip, ctx):
    """`pf_eigs_smallest2` (the paired, pipelined solve behind ONE C call; what `compute_spectra` uses for two symmetric
    graphs): against the reference's golden eigenpairs, against the Python pair driver on the same graphs, against two
    single C calls, with the eigenvector downloads left in flight, on a multi-component pair, and its fallbacks."""
    from pyfocusr_amd import Graph, PolyMesh
    from pyfocusr_amd import graph as graph_mod
    from pyfocusr_amd.graph import compute_spectra
    from pyfocusr_amd.meshgen import blob_mesh

    # the bundled 5k pair through the public path (C driver), then the same with the Python driver
    results = {}
    for driver in ("c", "python"):
        graph_mod.PAIR_DRIVER = driver
        try:
            gs = [Graph(mesh_of(golden(n)), n_spectral_features=6, n_rand_samples=10**9, ctx=ctx, verbose=False)
                  for n in ("target_mesh", "source_mesh")]
            before = hip.persist_state(ctx)["launches"]
            compute_spectra(gs)
            assert hip.persist_state(ctx)["launches"] > before or not hip.persist_state(ctx)["enabled"]  # (PF_PERSIST=0: tools/check_fallbacks.sh)
            results[driver] = [(g.eig_vals.copy(), g.eig_vecs.copy(), g.eigs_stats) for g in gs]
            for g in gs:
                g.device.close()
        finally:
            graph_mod.PAIR_DRIVER = "c"
    for (vc, xc, sc), (vp, xp, sp), name in zip(results["c"], results["python"], ("target_mesh", "source_mesh")):
        np.testing.assert_allclose(vc, golden(name)["k6_eig_vals"], rtol=1e-8)
        assert np.max(np.abs(xc - golden(name)["k6_eig_vecs"])) < 2e-9
        np.testing.assert_allclose(vc, vp, rtol=1e-10)
        assert np.max(np.abs(xc - xp)) < 1e-8
        assert sc.residuals.max() < 1e-10 and sc.degree == sp.degree and abs(sc.matvecs - sp.matvecs) <= 3 * sc.degree
    # the raw call: two blobs of different size, downloads in flight; equal to two single calls (same arithmetic per graph)
    ma, mb = blob_mesh(60000, seed=31), blob_mesh(35000, seed=32)
    da, db = hip.DeviceLaplacian(ma.points, ma.faces, ctx=ctx), hip.DeviceLaplacian(mb.points, mb.faces, ctx=ctx)
    (va, xa, sa), (vb, xb, sb) = da.eigs_smallest2(db, 5, 4, minmax=True, wait=False)
    da.finalize_wait()
    db.finalize_wait()
    assert xa.shape == (60000, 5) and xb.shape == (35000, 4) and sa["residuals"].max() < 1e-10 and sb["residuals"].max() < 1e-10
    for dev, vals, vecs in ((da, va, xa), (db, vb, xb)):
        v1, x1, s1 = dev.eigs_smallest(len(vals), minmax=True)
        np.testing.assert_allclose(vals, v1, rtol=1e-12)
        assert np.max(np.abs(vecs - x1)) < 1e-9
        assert np.array_equal(dev.final_rows(np.arange(0, dev.n, 997)), x1[::997])  # the resident block is the single call's
    da.close()
    db.close()
    # two components + strays in one of the graphs: locked null vectors per graph, isolated vertices masked
    a, b = blob_mesh(3000, seed=3), blob_mesh(2000, seed=4)
    pts = np.concatenate([a.points, b.points + 200.0, np.zeros((3, 3))])
    faces = np.concatenate([a.faces, b.faces + 3000])
    gs = [Graph(PolyMesh(pts, faces), n_spectral_features=4, n_rand_samples=10**9, ctx=ctx, verbose=False),
          Graph(blob_mesh(5000, seed=5), n_spectral_features=4, n_rand_samples=10**9, ctx=ctx, verbose=False)]
    compute_spectra(gs)
    ref = orc.graph_spectrum(pts, faces, 4)
    assert gs[0].eig_vals.shape == ref["eig_vals"].shape
    np.testing.assert_allclose(gs[0].eig_vals, ref["eig_vals"], rtol=1e-8)
    # what the call does not cover goes to the Python driver without a trace: a tiny graph
    for n_small, covered in ((150, True), (40, False)):
        small = [Graph(blob_mesh(n_small, seed=6), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False),
                 Graph(blob_mesh(9000, seed=7), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)]
        assert graph_mod._spectra_c(small) == covered
        if not covered:
            graph_mod._paired_spectra(*small)
        for g, seed, n in zip(small, (6, 7), (n_small, 9000)):
            m = blob_mesh(n, seed=seed)
            np.testing.assert_allclose(g.eig_vals, orc.graph_spectrum(m.points, m.faces, 3)["eig_vals"], rtol=1e-8)
    # a symmetric and an asymmetric graph in one call: Lanczos for the one, Arnoldi for the other, launches shared
    mixed = [Graph(mesh_of(golden("source_mesh_15k")), n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False),
             Graph(blob_mesh(9000, seed=7), n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False)]
    assert graph_mod._spectra_c(mixed) and [g.eigs_stats.mode for g in mixed] == [1, 0]
    np.testing.assert_allclose(mixed[0].eig_vals[:5], golden("source_mesh_15k")["k5_eig_vals"][:5], rtol=1e-8)
    m = blob_mesh(9000, seed=7)
    np.testing.assert_allclose(mixed[1].eig_vals, orc.graph_spectrum(m.points, m.faces, 5)["eig_vals"], rtol=1e-8)


def test_multi_component_and_recursive_eig(hip, ctx):
    """Two blobs + 3 unreferenced points: 2 null vectors + 3 isolated -> widen rule."""
    from pyfocusr_amd import Graph, PolyMesh, recursive_eig
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(700, seed=3), blob_mesh(900, seed=4)
    pts = np.concatenate([a.points, b.points + 200.0, np.zeros((3, 3))])
    faces = np.concatenate([a.faces, b.faces + 700])
    gr = Graph(PolyMesh(pts, faces), n_spectral_features=4, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    ref = orc.graph_spectrum(pts, faces, 4)
    assert gr.device.n_components == 2 and gr.device.n_isolated == 3
    assert gr.eig_vals.shape == ref["eig_vals"].shape
    np.testing.assert_allclose(gr.eig_vals, ref["eig_vals"], rtol=1e-8)
    gr.get_laplacian_matrix()
    vals, vecs = recursive_eig(gr.laplacian_matrix, k=5, n_k_needed=4)
    np.testing.assert_allclose(vals, ref["eig_vals"], rtol=1e-8)
    assert vecs.shape == ref["eig_vecs_raw"].shape
    # the reference's signature: any scipy sparse matrix (uploaded with pf_graph_from_matrix)
    vals2, vecs2 = recursive_eig(sparse.csr_matrix(gr.laplacian_matrix), k=5, n_k_needed=4)
    np.testing.assert_allclose(vals2, ref["eig_vals"], rtol=1e-8)
    assert vecs2.shape == vecs.shape


# ------------------------------------------------------------------------------- KNN
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 10, 16])
@pytest.mark.parametrize("n_ref,n_qry", [(1, 1), (300, 77), (5000, 5000), (1000, 70000)])
def test_knn_bit_exact(ctx, d, n_ref, n_qry):
    rng = np.random.default_rng(100 * d + n_ref)
    ref = rng.uniform(-0.5, 0.5, size=(n_ref, d))
    qry = rng.uniform(-0.5, 0.5, size=(n_qry, d))
    bidx, bd2 = orc.knn1_bruteforce(ref, qry)
    try:
        for mode in (0, 1, 2):  # by depth (the default), the grid over two axes, the box hierarchy over all axes
            ctx.knn_mode(mode)
            idx, d2 = ctx.knn1(ref, qry, return_d2=True)
            assert idx.dtype == np.int64
            assert np.array_equal(idx, bidx), mode
            assert np.array_equal(d2, bd2), mode  # same roundings: sum of squares left to right, no FMA
    finally:
        ctx.knn_mode(0)


def test_knn_radix_sorted_cells(ctx, monkeypatch):
    """The point sort of the grid search by hipCUB's radix sort (what sets of more than 16M points take; forced here by
    PF_KNN_BUCKET_MAX): same indices and distances as the counting sort's path and as brute force."""
    rng = np.random.default_rng(77)
    for n_ref, n_qry, d in ((40000, 40000, 5), (70000, 20000, 3), (20000, 50000, 2)):
        ref = rng.uniform(-0.5, 0.5, size=(n_ref, d))
        qry = ref[rng.integers(0, n_ref, n_qry)] + 0.01 * rng.standard_normal((n_qry, d))
        ctx.knn_mode(1)
        try:
            idx0, d0 = ctx.knn1(ref, qry, return_d2=True)
            monkeypatch.setenv("PF_KNN_BUCKET_MAX", "1")
            idx1, d1 = ctx.knn1(ref, qry, return_d2=True)
            monkeypatch.delenv("PF_KNN_BUCKET_MAX")
        finally:
            ctx.knn_mode(0)
        assert np.array_equal(idx0, idx1) and np.array_equal(d0, d1)
        rows = rng.integers(0, n_qry, 300)
        bidx, bd2 = orc.knn1_bruteforce(ref, qry[rows])
        assert np.array_equal(idx1[rows], bidx) and np.array_equal(d1[rows], bd2)


def test_knn_box_hierarchy(ctx):
    """pf_knn_tree.hip (the default for d >= 7) where its pruning is stressed: embedded 2-manifolds at sizes with several
    supers, exact ties on a lattice, duplicated references, queries that ARE references, clouds far apart (nothing
    prunes), one leaf / one super / a ragged last leaf - bit-identical to the grid search and to brute force on samples."""
    rng = np.random.default_rng(5)

    def surface(n, d, shift, seed):
        r = np.random.default_rng(seed)
        u, v = r.uniform(0, 1, n), r.uniform(0, 1, n)
        return np.stack([np.cos((c + 1) * u * 3.0) * np.sin((c % 3 + 1) * v * 2.0) for c in range(d)], axis=1) + shift

    cases = []
    for n, d in ((300000, 10), (70000, 7), (4097, 12), (64, 9), (65, 16), (1, 8)):
        cases.append((surface(n, d, 0.0, n), surface(min(n, 40000) + 3, d, 0.05, n + 1)))
    lat = np.round(rng.uniform(-0.5, 0.5, (20000, 8)) * 3) / 3
    cases.append((lat, np.round(rng.uniform(-0.5, 0.5, (5000, 8)) * 3) / 3))  # ties: the lowest index must win
    dup = surface(30000, 9, 0.0, 3)
    dup[15000:] = dup[:15000]
    cases.append((dup, dup[rng.integers(0, 30000, 7000)].copy()))  # duplicates; queries on references: d2 = 0, lowest index
    cases.append((surface(50000, 10, 0.0, 4), surface(3000, 10, 9.0, 5)))  # far apart
    try:
        for ref, qry in cases:
            ctx.knn_mode(2)
            ti, td = ctx.knn1(ref, qry, return_d2=True)
            ctx.knn_mode(1)
            gi, gd = ctx.knn1(ref, qry, return_d2=True)
            assert np.array_equal(ti, gi) and np.array_equal(td, gd), (ref.shape, qry.shape)
            rows = np.unique(np.linspace(0, len(qry) - 1, 40).astype(np.int64))
            bi, bd = orc.knn1_bruteforce(ref, qry[rows])
            assert np.array_equal(ti[rows], bi) and np.array_equal(td[rows], bd)
        assert np.array_equal(ctx.knn1(dup, dup[:15000].copy()), np.arange(15000))  # (mode 1 still set: the grid agrees)
        ctx.knn_mode(2)
        assert np.array_equal(ctx.knn1(dup, dup), np.concatenate([np.arange(15000), np.arange(15000)]))
        ctx.knn_tree_stats(True)
        ctx.knn1(cases[0][0], cases[0][1])
        leaves, supers = ctx.knn_tree_stats(False)
        # the point of the structure: a few dozen leaves per group of two queries out of 4688 (a brute force would scan all)
        assert 0 < leaves < 0.03 * 4688 * (len(cases[0][1]) / 2)
    finally:
        ctx.knn_mode(0)


def test_knn_ties_and_idempotence(ctx):
    rng = np.random.default_rng(7)
    ref = rng.uniform(-0.5, 0.5, size=(4000, 5))
    ref[1234] = ref[17]  # exact duplicate: lowest index must win
    ref[3999] = ref[17]
    idx, d2 = ctx.knn1(ref, ref, return_d2=True)
    expect = np.arange(4000)
    expect[1234] = 17
    expect[3999] = 17
    assert np.array_equal(idx, expect) and np.all(d2 == 0.0)
    with pytest.raises(Exception):
        ctx.knn1(np.zeros((4, 17)), np.zeros((4, 17)))


def test_knn_window_edge_cases(ctx):
    """The sorted-window search must stay exact where its pruning is stressed."""
    rng = np.random.default_rng(11)

    def check(ref, qry):
        idx, d2 = ctx.knn1(ref, qry, return_d2=True)
        bidx, bd2 = orc.knn1_bruteforce(ref, qry)
        assert np.array_equal(idx, bidx) and np.array_equal(d2, bd2)

    check(np.tile(rng.normal(size=(1, 4)), (700, 1)), rng.normal(size=(300, 4)))  # zero extent on every axis
    ref = rng.normal(size=(3000, 3))
    ref[:, 0] = np.where(rng.random(3000) < 0.5, 0.0, -0.0)  # widest axis elsewhere; signed zeros on one axis
    check(ref, rng.normal(size=(1000, 3)))
    ref = rng.normal(size=(2000, 2)) * np.array([100.0, 1e-3])
    ref[:, 0] = np.round(ref[:, 0])  # many equal keys on the sort axis, winner decided by the other axis
    check(ref, rng.normal(size=(900, 2)) * np.array([100.0, 1e-3]))
    check(rng.uniform(0, 1, size=(5000, 5)), rng.uniform(10, 11, size=(777, 5)))  # disjoint clouds: window = everything
    check(rng.normal(size=(5, 6)), rng.normal(size=(1000, 6)))  # fewer references than the probe width
    grid = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 3)
    check(grid, grid + 0.5)  # every query has 8 exactly equidistant references: lowest index must win
    check(grid[rng.permutation(len(grid))], grid + 0.5)


def test_knn_grids_of_many_rows_and_shrinking_rectangles(ctx):
    """The 1-NN kernel's group scan where its rectangle logic is stressed: grids of more than 64 rows (row batches),
    first bounds as wide as the grid (the rectangle shrinks while it is scanned), groups of queries that are far apart
    (Morton jumps, few queries), clouds that do not overlap, every group size (d <= 4: 8, d <= 8: 4, else 2)."""
    rng = np.random.default_rng(21)

    def check(ref, qry):
        idx, d2 = ctx.knn1(ref, qry, return_d2=True)
        bidx, bd2 = orc.knn1_bruteforce(ref, qry, chunk=256)
        assert np.array_equal(idx, bidx) and np.array_equal(d2, bd2)

    for d in (2, 4, 5, 8, 9, 13):
        check(rng.uniform(-0.5, 0.5, (40000, d)), rng.uniform(-0.5, 0.5, (1500, d)))  # unrelated clouds, 100 x 100 cells
    check(rng.uniform(0, 1, (30000, 4)), rng.uniform(3, 4, (900, 4)))  # disjoint: every rectangle is the grid (86 rows)
    check(rng.uniform(0, 1, (30000, 6)) * np.array([1000.0, 1.0, 1e-3, 1.0, 50.0, 1.0]), rng.uniform(0, 1, (700, 6)) * np.array([1000.0, 1.0, 1e-3, 1.0, 50.0, 1.0]))
    check(rng.uniform(0, 1, (50000, 3)), rng.uniform(0, 1, (37, 3)))  # 37 queries spread over 111 x 111 cells: groups span the grid
    ref = np.concatenate([rng.uniform(0, 0.05, (20000, 5)), rng.uniform(0.95, 1.0, (20000, 5))])  # two corners, empty middle
    check(ref, rng.uniform(0, 1, (1200, 5)))
    ref = rng.uniform(0, 1, (25000, 5))
    check(ref, ref[rng.permutation(25000)[:4000]] + 1e-4 * rng.standard_normal((4000, 5)))  # registered: the ring holds everything
    qry = rng.uniform(0, 1, (600, 5))
    qry[::7] = np.nan  # queries nothing compares with: index 0x7fffffff and an infinite distance, as before
    idx, d2 = ctx.knn1(ref, qry, return_d2=True)
    ok = ~np.isnan(qry[:, 0])
    bidx, bd2 = orc.knn1_bruteforce(ref, qry[ok], chunk=256)
    assert np.array_equal(idx[ok], bidx) and np.array_equal(d2[ok], bd2)
    assert np.all(idx[~ok] == 0x7FFFFFFF) and np.all(np.isinf(d2[~ok]))


def test_knn_property_random_shapes(ctx):
    """Property test (hypothesis): any point sets, any d <= 16 — device result == brute force, bit for bit."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    @settings(max_examples=40, deadline=None)
    @given(st.integers(1, 16), st.integers(1, 700), st.integers(1, 900), st.integers(0, 2**31 - 1),
           st.sampled_from(["uniform", "clustered", "lattice", "line"]))
    def run(d, n_ref, n_qry, seed, kind):
        rng = np.random.default_rng(seed)
        if kind == "uniform":
            ref, qry = rng.uniform(-1, 1, (n_ref, d)), rng.uniform(-1, 1, (n_qry, d))
        elif kind == "clustered":
            centres = rng.normal(size=(3, d))
            ref = centres[rng.integers(0, 3, n_ref)] + 1e-3 * rng.normal(size=(n_ref, d))
            qry = centres[rng.integers(0, 3, n_qry)] + 1e-3 * rng.normal(size=(n_qry, d))
        elif kind == "lattice":  # many exact ties
            ref, qry = rng.integers(0, 4, (n_ref, d)).astype(float), rng.integers(0, 4, (n_qry, d)) + 0.5
        else:  # all points on one line: the second grid axis is degenerate
            ref, qry = np.outer(rng.uniform(-1, 1, n_ref), np.ones(d)), np.outer(rng.uniform(-1, 1, n_qry), np.ones(d))
        idx, d2 = ctx.knn1(ref, qry, return_d2=True)
        bidx, bd2 = orc.knn1_bruteforce(ref, qry)
        assert np.array_equal(idx, bidx) and np.array_equal(d2, bd2)

    run()


@pytest.mark.parametrize("pair", ["pair_5k", "pair_15k"])
def test_knn_golden_correspondence(golden, ctx, pair):
    """focusr.py:351-353 on the reference's own spectral coordinates: indices identical
    to scipy KDTree's."""
    p = golden(pair)
    for tag in ("u", "w"):
        idx = ctx.knn1(p["coords_t_" + tag], p["coords_s_" + tag])
        assert np.array_equal(idx, p["knn_idx_" + tag])
    idx3 = ctx.knn1(p["rand_source_points"], p["rand_target_points"])
    assert np.array_equal(idx3, p["idx_spatial"])


# ------------------------------------------------------------------------------- eigsort / Focusr
class _FixedGraph(object):
    """Graph stand-in carrying golden canonical eigenpairs (what the fixtures fed the reference)."""


@pytest.mark.parametrize("pair,t,s,k,ns", [("pair_5k", "target_mesh", "source_mesh", 6, 3),
                                           ("pair_15k", "target_mesh_15k", "source_mesh_15k", 5, 5)])
def test_eigsort_and_correspondence_from_golden_eigs(golden, ctx, pair, t, s, k, ns):
    from pyfocusr_amd import Focusr, Graph, eigsort

    p, gt_, gs_ = golden(pair), golden(t), golden(s)

    def graph(gold):
        gr = Graph(mesh_of(gold), n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False)
        gr.eig_vals = gold["k%d_eig_vals" % k].copy()
        gr.eig_vecs = gold["k%d_eig_vecs" % k].copy()
        return gr

    gt, gs = graph(gt_), graph(gs_)
    sorter = eigsort(graph_target=gt, graph_source=gs, n_features=k, target_as_reference=True)
    Q = sorter.sort_eigenmaps()
    for name in ("c_lambda", "c_hist", "c_hist_f", "c_spatial", "c_spatial_f"):
        np.testing.assert_allclose(getattr(sorter, name), p[name], rtol=1e-12, err_msg=name)
    np.testing.assert_allclose(Q, p["Q"], rtol=1e-12)
    assert np.array_equal(sorter.idx_source_for_each_target_pt, p["idx_spatial"])
    assert np.array_equal(sorter.source_matches, p["source_matches"])
    assert np.array_equal(gs.eig_vecs, p["eig_vecs_s_sorted"])
    assert np.array_equal(gt.eig_vecs, p["eig_vecs_t_sorted"])

    reg = object.__new__(Focusr)
    reg._ctx = ctx
    reg.initial_correspondence_type = "kd"
    reg.graph_target, reg.graph_source, reg.Q, reg.n_spectral_features = gt, gs, Q, ns
    for tag, weighted in (("u", False), ("w", True)):
        reg.get_weighted_spectral_coords = weighted
        reg.calc_spectral_coords()
        reg.get_initial_correspondences()
        np.testing.assert_allclose(reg.source_spectral_coords, p["coords_s_" + tag], rtol=1e-12)
        # indices: recompute expectation on OUR coordinates (equal to golden up to 1e-12 weights)
        assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt,
                              orc.knn1(reg.target_spectral_coords, reg.source_spectral_coords))
        mism = np.sum(reg.corresponding_target_idx_for_each_source_pt != p["knn_idx_" + tag])
        assert mism == 0, mism
    np.testing.assert_allclose(reg.spectral_weights, p["spectral_weights"], rtol=1e-12)


@pytest.mark.parametrize("names,k,ns", [(("target_mesh", "source_mesh"), 5, 1500), (("target_mesh_15k", "source_mesh_15k"), 4, 5000),
                                         (("target_mesh", "source_mesh"), 3, 4096),
                                         # every vertex sampled: different counts per mesh (W1 on the merged breakpoints),
                                         # and more than 8192 rows (the LDS sort beyond 64 KB)
                                         (("target_mesh", "source_mesh"), 4, 10**9), (("target_mesh", "source_mesh"), 6, 10**9),
                                         (("target_mesh_15k", "source_mesh_15k"), 5, 10**9),
                                         (("target_mesh_15k", "source_mesh"), 3, 10**9)])
def test_eigsort_costs_on_device(golden, ctx, names, k, ns):
    """`pf_eigsort_costs` (c_hist, c_hist_f, c_spatial, c_spatial_f and the spatial 1-NN on the device, from the graphs'
    resident eigenvector blocks) against the host path of the same class, which the reference-generated goldens pin
    (test_eigsort_and_correspondence_from_golden_eigs): same samples, matrices to 1e-11, identical indices / matches."""
    from pyfocusr_amd import Graph, eigsort
    from pyfocusr_amd.graph import compute_spectra

    def graphs():
        np.random.seed(5)
        gs_ = [Graph(mesh_of(golden(nm)), n_spectral_features=k, n_rand_samples=ns, ctx=ctx, verbose=False) for nm in names]
        compute_spectra(gs_)
        return gs_

    results = []
    for host in (False, True):
        gt, gs = graphs()
        sorter = eigsort(gt, gs, k, target_as_reference=True)
        if host:
            _ = sorter.rand_target_points  # samples in hand: the host path runs
        else:
            assert sorter._device_costs() is not None
        Q = sorter.sort_eigenmaps()
        assert (sorter._device_result is None) == host
        results.append((sorter, Q, gs.eig_vecs.copy(), gs._final_map))
        # a second sort on the now permuted / flipped maps: the device reads the block through the recorded map
        again = eigsort(gt, gs, k, target_as_reference=True)
        if host:
            _ = again.rand_target_points
        results[-1] += (again.sort_eigenmaps(), again)
    (d, Qd, vd, fd, Qd2, d2), (h, Qh, vh, fh, Qh2, h2) = results
    for a, b in ((d, h), (d2, h2)):
        for name in ("c_lambda", "c_hist", "c_hist_f", "c_spatial", "c_spatial_f"):
            np.testing.assert_allclose(getattr(a, name), getattr(b, name), rtol=1e-11, atol=0, err_msg=name)
        assert np.array_equal(a.idx_source_for_each_target_pt, b.idx_source_for_each_target_pt)
        assert np.array_equal(a.source_matches, b.source_matches) and a.flipped_pairs == b.flipped_pairs
    np.testing.assert_allclose(Qd, Qh, rtol=1e-10)
    np.testing.assert_allclose(Qd2, Qh2, rtol=1e-10)
    assert np.array_equal(vd, vh) and np.array_equal(fd[0], fh[0]) and np.array_equal(fd[1], fh[1])
    if names == ("target_mesh", "source_mesh") and k == 6 and ns >= 5000:
        # the DEVICE path directly against the reference's own matrices (every vertex sampled: no randomness); what is left
        # between them is the 2e-9 between the two sets of eigenvectors and the device's log
        p5 = golden("pair_5k")
        assert d._device_result is not None
        for name in ("c_lambda", "c_hist", "c_hist_f", "c_spatial", "c_spatial_f"):
            np.testing.assert_allclose(getattr(d, name), p5[name], rtol=2e-6, atol=1e-12, err_msg="device vs reference: " + name)
        assert np.array_equal(d.idx_source_for_each_target_pt, p5["idx_spatial"])
        np.testing.assert_allclose(Qd, p5["Q"], rtol=2e-6)
        assert np.array_equal(d.source_matches, p5["source_matches"]) and np.array_equal(d.target_matches, p5["target_matches"])
    # lazily gathered samples are still there for whoever asks (eigsort.py:34-41)
    assert d.rand_target_eig_vecs.shape == (min(ns, d.graph_target.n_points), d.graph_target.eig_vecs.shape[1])
    assert d.rand_source_points.shape[1] == 3 and d.rand_source_points.min() == 0.0 and d.rand_source_points.max() == 1.0


def test_focusr_end_to_end_5k(golden, ctx):
    """BASELINE config C1 through the public API: own Laplacian + own eigensolve + eigsort +
    KNN; the correspondence indices equal the reference's (up to sign-fixed eigenvectors)."""
    from pyfocusr_amd import Focusr

    p, gt_, gs_ = golden("pair_5k"), golden("target_mesh"), golden("source_mesh")
    reg = Focusr(mesh_of(gt_), mesh_of(gs_), icp_register_first=False, n_spectral_features=3, n_extra_spectral=3,
                 n_coords_spectral_ordering=10000, get_weighted_spectral_coords=False, list_features_to_calc=[],
                 return_average_final_points=False, smooth_correspondences=False, ctx=ctx,
                 registration=lambda src, tgt, kind: tgt)
    np.testing.assert_allclose(reg.graph_target.eig_vals, gt_["k6_eig_vals"], rtol=1e-8)
    np.testing.assert_allclose(reg.graph_source.eig_vals, gs_["k6_eig_vals"], rtol=1e-8)
    reg.align_maps()
    np.testing.assert_allclose(reg.Q, p["Q"], rtol=1e-6)
    assert np.max(np.abs(reg.graph_source.eig_vecs - p["eig_vecs_s_sorted"])) < 2e-9
    mism = int(np.sum(reg.corresponding_target_idx_for_each_source_pt != p["knn_idx_u"]))
    assert mism == 0, "%d of 5000 correspondences differ" % mism
    assert reg.nearest_neighbor_transformed_points.shape == (5000, 3)


def test_knn_topk_and_weighted_final_locations(golden, ctx):
    """3-NN (focusr.py:409-412) and the inverse-distance average (focusr.py:401-426)."""
    from scipy.spatial import KDTree

    rng = np.random.default_rng(21)
    ref = rng.normal(size=(4000, 3))
    qry = np.concatenate([rng.normal(size=(1500, 3)), ref[:7]])  # the last 7 coincide with a reference
    for k in (2, 3, 4):
        idx, d2 = ctx.knn(ref, qry, k)
        dd, ii = KDTree(ref).query(qry, k=k)
        assert np.array_equal(idx, ii)
        np.testing.assert_allclose(np.sqrt(d2), dd, rtol=1e-14, atol=0)
    with pytest.raises(Exception):
        ctx.knn(rng.normal(size=(50, 6)), rng.normal(size=(5, 6)), 3)  # k > 1 only for d <= 4

    from pyfocusr_amd import Focusr, PolyMesh

    gt, gs, p = golden("target_mesh"), golden("source_mesh"), golden("pair_5k")
    reg = object.__new__(Focusr)
    reg._ctx = ctx
    nt = len(gt["points"])
    Wt = sparse.csr_matrix((gt["W_data"], gt["W_indices"], gt["W_indptr"]), shape=(nt, nt))
    Ws = sparse.csr_matrix((gs["W_data"], gs["W_indices"], gs["W_indptr"]), shape=(len(gs["points"]),) * 2)
    sm, proj, idx2 = orc.smoothed_correspondences(Wt, Ws, gt["points"], p["knn_idx_u"], 30, 10)
    proj[:5] = sm[[3, 77, 1500, 9, 4000]]  # force the coincident-vertex branch (focusr.py:415-419)
    reg.smoothed_target_coords, reg.source_projected_on_target = sm, proj

    class G(object):
        points = gt["points"]

    reg.graph_target = G()
    reg.get_weighted_final_node_locations()
    ref_out = orc.weighted_final_node_locations(sm, proj, gt["points"])
    np.testing.assert_allclose(reg.weighted_avg_transformed_points, ref_out, rtol=1e-12, atol=1e-12)
    assert np.array_equal(reg.weighted_avg_transformed_points[:5], gt["points"][[3, 77, 1500, 9, 4000]])


def test_focusr_default_tail_of_align_maps(golden, ctx):
    """align_maps with the reference's default post-processing switches (smoothing, weighted and
    nearest final locations, transformed meshes) against the oracle chain."""
    from pyfocusr_amd import Focusr

    p, gt_, gs_ = golden("pair_5k"), golden("target_mesh"), golden("source_mesh")
    reg = Focusr(mesh_of(gt_), mesh_of(gs_), icp_register_first=False, n_spectral_features=3, n_extra_spectral=3,
                 n_coords_spectral_ordering=10000, get_weighted_spectral_coords=False, list_features_to_calc=[],
                 graph_smoothing_iterations=30, projection_smooth_iterations=10, ctx=ctx,
                 registration=lambda src, tgt, kind: tgt)
    reg.align_maps()
    nt = len(gt_["points"])
    Wt = sparse.csr_matrix((gt_["W_data"], gt_["W_indices"], gt_["W_indptr"]), shape=(nt, nt))
    Ws = sparse.csr_matrix((gs_["W_data"], gs_["W_indices"], gs_["W_indptr"]), shape=(len(gs_["points"]),) * 2)
    sm, proj, idx2 = orc.smoothed_correspondences(Wt, Ws, gt_["points"], p["knn_idx_u"], 30, 10)
    np.testing.assert_allclose(reg.smoothed_target_coords, sm, rtol=1e-13)
    np.testing.assert_allclose(reg.source_projected_on_target, proj, rtol=1e-12)
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, idx2)
    np.testing.assert_allclose(reg.weighted_avg_transformed_points,
                               orc.weighted_final_node_locations(sm, proj, gt_["points"]), rtol=1e-10, atol=1e-10)
    assert reg.weighted_avg_transformed_mesh.points.shape == (5000, 3)
    assert np.array_equal(reg.nearest_neighbour_transformed_mesh.points, gt_["points"][idx2])
    reg.get_average_shape()
    assert reg.average_mesh.faces.shape == gs_["faces"].shape


def test_spectral_knn_on_device_resident_eigenvectors(golden, ctx):
    """focusr.py:351-353 with the coordinates taken from the blocks the eigensolves left in HBM (`spectral_knn` ->
    `pf_knn1_graphs`): indices and distances bit-identical to the host-array path, with eigsort's flips and column
    permutation (eigsort.py:108-122) folded into the call, weighted and un-weighted; sampled rows (`pf_final_rows`,
    graph.py:266-267) equal to fancy indexing of the host array; falls back when the host array was replaced."""
    from pyfocusr_amd import Focusr, Graph, eigsort
    from pyfocusr_amd.graph import compute_spectra, spectral_knn

    p, gt_, gs_ = golden("pair_15k"), golden("target_mesh_15k"), golden("source_mesh_15k")
    for ref_is_target in (True, False):
        gt = Graph(mesh_of(gt_), n_spectral_features=5, n_rand_samples=3000, ctx=ctx, verbose=False)
        gs = Graph(mesh_of(gs_), n_spectral_features=5, n_rand_samples=3000, ctx=ctx, verbose=False)
        compute_spectra([gt, gs])
        assert gs._final_map is not None and gs.eig_vecs.shape[1] == 9  # widened: 9 columns resident
        assert np.array_equal(gs.get_rand_eig_vecs(), gs.eig_vecs[gs.rand_idxs, :])
        assert np.array_equal(gt.get_rand_eig_vecs(), gt.eig_vecs[gt.rand_idxs, :])
        sorter = eigsort(gt, gs, 5, target_as_reference=ref_is_target)
        # make the assignment a genuine permutation + flips so that the folding is exercised
        sorter.sort_eigenmaps()
        moved = gs if ref_is_target else gt
        moved.eig_vecs[:, [0, 2]] = moved.eig_vecs[:, [2, 0]]  # an edit eigsort did not make ...
        assert spectral_knn(gt, gs, 5) is None and moved._final_map is None  # ... is noticed: host path
        moved._final_map = None
    gt = Graph(mesh_of(gt_), n_spectral_features=5, n_rand_samples=20000, ctx=ctx, verbose=False)
    gs = Graph(mesh_of(gs_), n_spectral_features=5, n_rand_samples=20000, ctx=ctx, verbose=False)
    compute_spectra([gt, gs])
    gs._final_map = None
    gs.eig_vecs = gs.eig_vecs[:, ::-1].copy()  # column order reversed before eigsort: it has to permute
    gs._final_map = (np.arange(9)[::-1].copy(), np.ones(9))
    sorter = eigsort(gt, gs, 5, target_as_reference=True)
    Q = sorter.sort_eigenmaps()
    assert not np.array_equal(sorter.source_matches, sorter.target_matches)  # a real permutation
    assert len(sorter.flipped_pairs) > 0
    w = np.array([0.9, 0.8, 0.1, 0.5, 0.7])
    for weights in (None, w):
        ct = gt.eig_vecs[:, :5] if weights is None else gt.eig_vecs[:, :5] * weights[None, :]
        cs = gs.eig_vecs[:, :5] if weights is None else gs.eig_vecs[:, :5] * weights[None, :]
        idx_host, d2_host = ctx.knn1(ct, cs, return_d2=True)
        idx_dev = spectral_knn(gt, gs, 5, weights)
        assert idx_dev is not None and np.array_equal(idx_dev, idx_host)
        (c_t, s_t), (c_s, s_s) = gt._final_map, gs._final_map
        ww = np.ones(5) if weights is None else weights
        idx2, d2_dev = ctx.knn1_graphs(gt.device, gs.device, c_t[:5], s_t[:5] * ww, c_s[:5], s_s[:5] * ww, return_d2=True)
        assert np.array_equal(idx2, idx_host) and np.array_equal(d2_dev, d2_host)
    # through Focusr: derived coordinates take the device path, assigned ones the host path; same indices
    reg = object.__new__(Focusr)
    reg._ctx = ctx
    reg.initial_correspondence_type = "kd"
    reg.graph_target, reg.graph_source, reg.Q, reg.n_spectral_features = gt, gs, Q, 5
    for weighted in (False, True):
        reg.get_weighted_spectral_coords = weighted
        reg.calc_spectral_coords()
        reg.get_initial_correspondences()
        a = reg.corresponding_target_idx_for_each_source_pt.copy()
        reg.target_spectral_coords = reg.target_spectral_coords.copy()  # now an ordinary attribute: host path
        reg.get_initial_correspondences()
        assert np.array_equal(a, reg.corresponding_target_idx_for_each_source_pt)
        assert np.array_equal(a, orc.knn1(reg.target_spectral_coords, reg.source_spectral_coords))
    with pytest.raises(Exception):
        ctx.knn1_graphs(gt.device, gs.device, [0, 99], [1.0, 1.0], [0, 1], [1.0, 1.0])


def test_split_pair_device_to_device(golden, ctx):
    """BASELINE config C4 on one GPU: the two ranks of `parallel.split_pair_correspondence` as threads of this process,
    device-to-device copies standing in for RCCL's all-gather (everything else is the shipped path: the resident
    blocks wrapped zero-copy as torch tensors, samples taken from the gathered device buffer, the query-sharded KNN
    reading that buffer through `pf_knn1_blocks`, int64 index shards).  On the bundled 15k pair with every vertex
    sampled the result must be the reference's: Q and all 14 996 weighted correspondence indices of pair_15k.npz."""
    import threading

    import torch

    from pyfocusr_amd import Graph
    from pyfocusr_amd.graph import compute_spectra
    from pyfocusr_amd.parallel import split_pair_correspondence

    p, gt_, gs_ = golden("pair_15k"), golden("target_mesh_15k"), golden("source_mesh_15k")
    graphs = [Graph(mesh_of(g), n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False) for g in (gt_, gs_)]
    compute_spectra(graphs)
    lock, barrier, shared, results, errors = threading.Lock(), threading.Barrier(2), {}, {}, []

    class ThreadDist(object):
        def __init__(self, rank):
            self.rank = rank

        def get_world_size(self):
            return 2

        def get_rank(self):
            return self.rank

        def all_gather_into_tensor(self, out, inp):
            shared[self.rank] = inp
            barrier.wait()
            n = inp.numel()
            for r in range(2):
                out[r * n:(r + 1) * n].copy_(shared[r].reshape(-1))  # device-to-device
            torch.cuda.synchronize()
            barrier.wait()

    class Locked(object):  # calls on one ctx must not overlap in time
        def knn1(self, ref, qry):
            with lock:
                return ctx.knn1(ref, qry)

    def knn_blocks(ref, n_ref, qry, n_qry, stride, ct, st, cs, ss):
        with lock:
            return ctx.knn1_blocks(ref.data_ptr(), n_ref, stride, qry.data_ptr(), n_qry, stride, ct, st, cs, ss)

    def run(rank):
        try:
            results[rank] = split_pair_correspondence(ThreadDist(rank), torch, graphs[rank], 5, 10**9, seed=3,
                                                      knn_blocks=knn_blocks, knn_ctx=Locked())
        except BaseException as exc:  # noqa: BLE001
            errors.append(exc)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    for rank in range(2):
        idx, Q, w = results[rank]
        np.testing.assert_allclose(Q, p["Q"], rtol=1e-5)
        np.testing.assert_allclose(w, p["spectral_weights"], rtol=1e-5)
        assert idx.dtype == np.int64 and len(idx) == 14996
        assert int(np.sum(idx != p["knn_idx_w"])) == 0
    assert np.array_equal(results[0][0], results[1][0])


def test_rccl_all_gather_of_resident_block(golden, ctx):
    """The RCCL leg of the split pair on the hardware at hand (ONE GPU, so a world of one rank): the resident eigenvector
    block wrapped zero-copy as a torch tensor, `all_gather_into_tensor` (backend "nccl" = RCCL) enqueued on the library's
    own stream through `torch.cuda.ExternalStream`, and `pf_knn1_blocks` reading the gathered buffer.  The two-rank
    control flow is covered by `test_split_pair_device_to_device` and tests/test_parallel_gloo.py."""
    import socket

    import torch
    import torch.distributed as dist

    from pyfocusr_amd import Graph
    from pyfocusr_amd.parallel import _all_gather_stack, resident_block_tensor

    g_ = golden("target_mesh")
    gr = Graph(mesh_of(g_), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", ctx.device))
    try:
        block = resident_block_tensor(torch, gr.device, ctx.device)
        assert block.data_ptr() == gr.device.final_device()[0] and tuple(block.shape) == gr.eig_vecs.shape  # zero-copy
        assert np.array_equal(block.cpu().numpy(), gr.eig_vecs)
        stream = torch.cuda.ExternalStream(ctx.stream_ptr, device=torch.device("cuda", ctx.device))
        with torch.cuda.stream(stream):
            both = _all_gather_stack(dist, torch, block)
        stream.synchronize()
        assert tuple(both.shape) == (1,) + gr.eig_vecs.shape and np.array_equal(both[0].cpu().numpy(), gr.eig_vecs)
        n, m = gr.eig_vecs.shape
        idx, d2 = ctx.knn1_blocks(both[0].data_ptr(), n, m, both[0].data_ptr() + 8 * 100 * m, n - 100, m, np.arange(3), np.ones(3),
                                  np.arange(3), np.ones(3), return_d2=True)
        assert np.array_equal(idx, np.arange(100, n)) and np.all(d2 == 0)  # every row finds itself
    finally:
        dist.destroy_process_group()


def test_tail_vs_reference_fixture(golden, ctx):
    """SURVEY f1/f2 against outputs of the REFERENCE's own methods (tests/golden/tail_5k.npz, written by
    tools/make_golden.py: tail_fixture): `Graph.mean_filter_graph` (graph.py:320-354, n x 3 and n x 1, 25 and 300
    iterations), `get_smoothed_correspondences` (focusr.py:368-396), `get_weighted_final_node_locations` incl. the
    coincident-point branch (focusr.py:401-426) and `get_nearest_neighbour_final_node_locations` (:428-431)."""
    from pyfocusr_amd import Focusr, Graph

    t, gt_, gs_ = golden("tail_5k"), golden("target_mesh"), golden("source_mesh")
    gt = Graph(mesh_of(gt_), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gs = Graph(mesh_of(gs_), n_spectral_features=3, n_rand_samples=10**9, ctx=ctx, verbose=False)
    for it in (25, 300):  # the device keeps scipy's summation order: bit-identical
        assert np.array_equal(gt.mean_filter_graph(gt.points, iterations=it), t["mf_t_points_%d" % it])
        assert np.array_equal(gs.mean_filter_graph(gs.points, iterations=it), t["mf_s_points_%d" % it])
        got = np.asarray(gt.mean_filter_graph(t["scalar_in"][:, None], iterations=it)).reshape(-1, 1)
        assert np.array_equal(got, t["mf_t_scalar_%d" % it])

    reg = object.__new__(Focusr)
    reg._ctx = ctx
    reg.graph_target, reg.graph_source = gt, gs
    reg.initial_correspondence_type = reg.final_correspondence_type = "kd"
    reg.graph_smoothing_iterations, reg.projection_smooth_iterations = 300, 40  # focusr.py:49,55 defaults
    reg.corresponding_target_idx_for_each_source_pt = t["idx_initial"].copy()
    reg.get_smoothed_correspondences()
    assert np.array_equal(reg.smoothed_target_coords, t["smoothed_target_coords"])
    assert np.array_equal(reg.source_projected_on_target, t["source_projected_on_target"])
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, t["idx_final"])
    idx3, d2 = ctx.knn(reg.smoothed_target_coords, reg.source_projected_on_target, 3)
    assert np.array_equal(idx3, t["final_top4_idx"][:, :3])
    np.testing.assert_allclose(np.sqrt(d2), t["final_top4_dist"][:, :3], rtol=2e-16 * 4, atol=0)
    reg.get_weighted_final_node_locations()
    # same 3 neighbours, same distances; the average is summed pairwise here and by np.sum/sum() there
    np.testing.assert_allclose(reg.weighted_avg_transformed_points, t["weighted_avg_transformed_points"],
                               rtol=1e-14, atol=0)
    reg.get_nearest_neighbour_final_node_locations()
    assert np.array_equal(reg.nearest_neighbor_transformed_points, t["nearest_neighbor_transformed_points"])
    reg.source_projected_on_target = t["coincident_projected"].copy()
    reg.get_weighted_final_node_locations()
    rows = t["coincident_rows"]
    assert np.array_equal(reg.weighted_avg_transformed_points[rows], t["coincident_weighted_avg"][rows])
    np.testing.assert_allclose(reg.weighted_avg_transformed_points, t["coincident_weighted_avg"], rtol=1e-14, atol=0)


def test_focusr_end_to_end_15k(golden, ctx):
    """BASELINE config C2 through the public API: own assembly (asymmetric W, isolated vertices) -> own
    eigensolve (widen-and-retry: 9 columns for the source) -> eigsort flips / permutation (eigsort.py:54-140) ->
    focusr.py:351-353 indices.  north_star: correspondence indices identical to the reference's — 0 of 14 996
    may differ, weighted and un-weighted."""
    from pyfocusr_amd import Focusr

    p, gt_, gs_ = golden("pair_15k"), golden("target_mesh_15k"), golden("source_mesh_15k")
    for tag, weighted in (("u", False), ("w", True)):
        reg = Focusr(mesh_of(gt_), mesh_of(gs_), icp_register_first=False, n_spectral_features=5, n_extra_spectral=0,
                     n_coords_spectral_ordering=20000, get_weighted_spectral_coords=weighted, list_features_to_calc=[],
                     return_average_final_points=False, smooth_correspondences=False, ctx=ctx,
                     registration=lambda src, tgt, kind: tgt)
        np.testing.assert_allclose(reg.graph_target.eig_vals, gt_["k5_eig_vals"], rtol=1e-8)
        np.testing.assert_allclose(reg.graph_source.eig_vals, gs_["k5_eig_vals"], rtol=1e-8)
        assert reg.graph_source.eig_vecs.shape == gs_["k5_eig_vecs"].shape  # 9 columns
        reg.align_maps()
        np.testing.assert_allclose(reg.Q, p["Q"], rtol=1e-5)
        assert np.max(np.abs(reg.graph_source.eig_vecs - p["eig_vecs_s_sorted"])) < 5e-7  # flips + permutation applied
        if weighted:
            np.testing.assert_allclose(reg.spectral_weights, p["spectral_weights"], rtol=1e-5)
        got = reg.corresponding_target_idx_for_each_source_pt
        bad = np.nonzero(got != p["knn_idx_" + tag])[0]
        margins = p["knn_top2_" + tag][bad, 1] - p["knn_top2_" + tag][bad, 0] if len(bad) else []
        assert len(bad) == 0, "%d of %d correspondences differ (%s); top-2 margins of the offenders: %s" % (
            len(bad), len(got), tag, np.sort(margins)[:10])


# ------------------------------------------------------------------------------- full size (C3)
def test_full_size_250k_properties(hip, ctx):
    """BASELINE config C3 size: properties that do not need a CPU solve."""
    from pyfocusr_amd import Graph
    from pyfocusr_amd.meshgen import blob_mesh

    n = 250000
    mesh = blob_mesh(n, seed=0)
    gr = Graph(mesh, n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False)
    dev = gr.device
    assert dev.symmetric and dev.n_components == 1 and dev.n_isolated == 0
    assert dev.nnz_w == 3 * len(mesh.faces) and dev.nnz_l == n + 3 * len(mesh.faces)
    # sampled rows of W bit-exact against the oracle formula
    h = dev.download()
    W = orc.weighted_adjacency(mesh.points, mesh.faces)
    assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices)
    assert np.array_equal(h["w"], W.data)
    gr.get_graph_spectrum()
    assert gr.eig_vals.shape == (5,) and np.all(np.diff(gr.eig_vals) > 0) and gr.eig_vals[0] > 1e-10
    assert gr.eigs_stats.residuals.max() < 1e-10
    assert gr.eig_vecs.min() == -0.5 and gr.eig_vecs.max() == 0.5
    # residuals against the oracle's L (rw form), on un-normalised vectors
    deg, d_inv = orc.degree_and_inverse(W)
    L = orc.laplacian(W, deg, d_inv)
    vals, vecs, _ = __import__("pyfocusr_amd.graph", fromlist=["_device_eigs"])._device_eigs(dev, 6, 5)
    R = L @ vecs - vecs * vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-10
    # KNN on the spectral coordinates: idempotence + sampled rows against brute force
    idx, d2 = ctx.knn1(gr.eig_vecs, gr.eig_vecs, return_d2=True)
    assert np.array_equal(idx, np.arange(n)) and np.all(d2 == 0)
    rng = np.random.default_rng(0)
    q = rng.uniform(-0.5, 0.5, size=(n, 5))
    idx, d2 = ctx.knn1(gr.eig_vecs, q, return_d2=True)
    sample = rng.choice(n, 300, replace=False)
    bidx, bd2 = orc.knn1_bruteforce(gr.eig_vecs, q[sample])
    assert np.array_equal(idx[sample], bidx) and np.array_equal(d2[sample], bd2)


def test_full_size_250k_vs_oracle(ctx):
    """BASELINE config C3 at full size against the oracle itself (what `bench.py` prints as `parity_at_full_size`, as a
    test): the eigenvalues of one 250k-vertex mesh against the reference's `recursive_eig` -> scipy `eigs` on the oracle's
    L (graph.py:357-389; north_star asks 1e-6, the bar here is 1e-8), its eigenvectors up to the fixed sign, and ALL 250 000
    correspondence indices of the pair - through the public path: eigsort, weights, `spectral_knn` - against
    `KDTree(target).query(source)` (focusr.py:351-353) on the very coordinates the device search consumed."""
    from scipy.spatial import KDTree

    from pyfocusr_amd import Graph, eigsort
    from pyfocusr_amd.graph import compute_spectra, spectral_knn
    from pyfocusr_amd.meshgen import blob_mesh

    n, k = 250000, 5
    meshes = [blob_mesh(n, seed=s) for s in (0, 1)]
    np.random.seed(7)
    gt, gs = [Graph(m, n_spectral_features=k, n_rand_samples=5000, ctx=ctx, verbose=False) for m in meshes]
    compute_spectra([gt, gs])
    W, deg, d_inv, L = orc.graph_matrices(meshes[0].points, meshes[0].faces)
    ref_vals, ref_vecs = orc.canonicalize(*orc.recursive_eig(L, k + 1, k))
    np.testing.assert_allclose(gt.eig_vals, ref_vals[:k], rtol=1e-8)
    # up to the sign of each column (the fixed sign rule looks at the largest entry: two near-equal extremes may pick differently
    # in the two solvers); gaps >= 7 %, residuals ~1e-12 on both sides
    mine = gt.eig_vecs + 0.5
    both = [orc.minmax_normalize(s_ * ref_vecs[:, :k]) + 0.5 for s_ in (1.0, -1.0)]
    err = np.minimum(np.max(np.abs(mine - both[0]), axis=0), np.max(np.abs(mine - both[1]), axis=0))
    assert err.max() < 1e-6, err
    Q = eigsort(gt, gs, k, target_as_reference=True).sort_eigenmaps()
    w = Q[:k] * np.max((gs.eig_vals[:k], gt.eig_vals[:k]), axis=0)  # focusr.py:481-490
    w = np.exp(-(w**2) / (2 * np.mean(w) ** 2))
    idx = spectral_knn(gt, gs, k, w)
    assert idx is not None and idx.dtype == np.int64 and idx.shape == (n,)
    tgt, src = gt.eig_vecs[:, :k] * w[None, :], gs.eig_vecs[:, :k] * w[None, :]
    _, kd = KDTree(tgt).query(src, workers=-1)
    assert int(np.sum(kd != idx)) == 0
    for g in (gt, gs):
        g.device.close()


def test_full_size_1m_k10_properties(hip, ctx):
    """BASELINE config C5 size on one GPU (1M-vertex blob pair, k=10): the size-independent properties of
    `test_full_size_250k_properties` — W bit-exact vs the oracle formula, residuals against the oracle's L,
    eigenvalue order, paired solve == what the pair path returns, KNN (d=10) idempotence and sampled rows
    against brute force."""
    from pyfocusr_amd import Graph, compute_spectra
    from pyfocusr_amd.meshgen import blob_mesh

    n, k = 1000000, 10
    meshes = [blob_mesh(n, seed=s) for s in (0, 1)]
    graphs = [Graph(m, n_spectral_features=k, n_rand_samples=10**9, norm_eig_vecs=nrm, ctx=ctx, verbose=False)
              for m, nrm in zip(meshes, (False, True))]
    dev = graphs[0].device
    assert dev.symmetric and dev.n_components == 1 and dev.n_isolated == 0
    assert dev.nnz_w == 3 * len(meshes[0].faces) and dev.nnz_l == n + 3 * len(meshes[0].faces)
    h = dev.download()
    W = orc.weighted_adjacency(meshes[0].points, meshes[0].faces)
    assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices)
    assert np.array_equal(h["w"], W.data)
    compute_spectra(graphs)
    for gr in graphs:
        assert gr.eig_vals.shape == (k,) and np.all(np.diff(gr.eig_vals) > 0) and gr.eig_vals[0] > 1e-10
        assert gr.eig_vecs.shape == (n, k)
        assert gr.eigs_stats.residuals.max() < 1e-10
    deg, d_inv = orc.degree_and_inverse(W)
    L = orc.laplacian(W, deg, d_inv)
    vecs, vals = graphs[0].eig_vecs, graphs[0].eig_vals  # raw unit-norm vectors of the seed-0 mesh
    np.testing.assert_allclose(np.linalg.norm(vecs, axis=0), 1.0, rtol=1e-12)
    R = L @ vecs - vecs * vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-10
    tv = graphs[1].eig_vecs
    assert tv.min() == -0.5 and tv.max() == 0.5
    idx, d2 = ctx.knn1(tv, tv, return_d2=True)
    assert np.array_equal(idx, np.arange(n)) and np.all(d2 == 0)
    sv = (vecs - vecs.min(axis=0)) / np.ptp(vecs, axis=0) - 0.5
    idx, d2 = ctx.knn1(tv, sv, return_d2=True)  # focusr.py:351-353 at C5 size, d = 10
    rng = np.random.default_rng(5)
    sample = rng.choice(n, 96, replace=False)
    bidx, bd2 = orc.knn1_bruteforce(tv, sv[sample], chunk=32)
    assert np.array_equal(idx[sample], bidx) and np.array_equal(d2[sample], bd2)


def test_hungarian_correspondence_small(golden, ctx):
    """focusr.py:340-349 on a mesh small enough for the O(N^3) assignment: a permutation (one-to-one), each
    source vertex close to its assigned target vertex in spectral space."""
    from pyfocusr_amd import Focusr
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(600, seed=3), blob_mesh(600, seed=4)
    reg = Focusr(a, b, icp_register_first=False, n_spectral_features=3, n_extra_spectral=0, list_features_to_calc=[],
                 initial_correspondence_type="hungarian", final_correspondence_type="hungarian", ctx=ctx,
                 registration=lambda src, tgt, kind: tgt)
    reg.align_maps()
    idx = reg.corresponding_target_idx_for_each_source_pt
    assert sorted(idx.tolist()) == list(range(600))
    with pytest.raises(ValueError):
        Focusr(a, b, icp_register_first=False, initial_correspondence_type="nearest", ctx=ctx)


def test_eigs_partial_reorthogonalisation_on_device(hip, ctx, monkeypatch):
    """`pf_eigs_smallest` on symmetric graphs runs Lanczos with partial reorthogonalisation (most steps against the null
    vectors and the last two basis vectors, `stats.local_steps`): same eigenpairs as with full Gram-Schmidt in every step
    (`PF_EIGS_PRO=0`) on a blob with two components and on a torus grid - every eigenvalue double, one thick restart, the
    kept Ritz vectors orthonormalised again."""
    from pyfocusr_amd import Graph, PolyMesh
    from pyfocusr_amd.meshgen import blob_mesh

    nu, nv = 128, 64
    uu, vv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    au, av = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
    pts = np.stack([(3 + np.cos(av)) * np.cos(au), (3 + np.cos(av)) * np.sin(au), np.sin(av)], axis=-1).reshape(-1, 3)
    a, b, c, d = uu * nv + vv, ((uu + 1) % nu) * nv + vv, ((uu + 1) % nu) * nv + (vv + 1) % nv, uu * nv + (vv + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    m1, m2 = blob_mesh(25000, seed=40744), blob_mesh(6250, seed=657489)  # (the fuzzer's case that lost its Ritz vectors once)
    two = PolyMesh(np.concatenate([m1.points, m2.points + 300.0]), np.concatenate([m1.faces, m2.faces + 25000]))
    for mesh, k, restarts in ((PolyMesh(pts, faces), 9, 1), (two, 4, 0)):
        g = Graph(mesh, n_spectral_features=k, norm_eig_vecs=False, n_rand_samples=10**9, ctx=ctx, verbose=False)
        g.get_graph_spectrum()
        monkeypatch.setenv("PF_EIGS_PRO", "0")
        vals_f, vecs_f, st_f = g.device.eigs_smallest(k)
        monkeypatch.delenv("PF_EIGS_PRO")
        vals, vecs, st = g.device.eigs_smallest(k)
        assert st_f["local_steps"] == 0 and st["local_steps"] >= 0.5 * st["outer_steps"], (st, st_f)
        assert st["restarts"] == st_f["restarts"] == restarts and abs(st["outer_steps"] - st_f["outer_steps"]) <= 4
        np.testing.assert_allclose(vals, vals_f, rtol=1e-12)
        assert st["max_residual"] < 5e-12
        np.testing.assert_allclose(g.eig_vals[:k], vals, rtol=1e-12)  # (the public path took the same solver)
        g.device.close()


@pytest.mark.parametrize("n", [31250, 420000])
def test_orth_split_two_ranges(hip, ctx, n):
    """`pf_orth_split`: one Gram-Schmidt step over TWO ranges of slots (the local steps of Lanczos with partial
    reorthogonalisation: locked null vectors + the last two basis vectors) against numpy - one pass, the device's second
    pass, and a step that cancels digits (second pass by pf_orth_end); both kernel shapes (below / from 400k rows)."""
    from pyfocusr_amd.meshgen import blob_mesh

    rng = np.random.default_rng(1)
    m = blob_mesh(n, seed=5)
    g = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    try:
        g.ws_ensure(16)
        Q, _ = np.linalg.qr(rng.standard_normal((n, 8)))
        for s in range(8):
            g.upload(s, Q[:, s])
        B = Q[:, [0, 1, 5, 6]]
        cancelling = Q[:, 6] * 1e3 + Q[:, 1] * 50 + 1e-3 * rng.standard_normal(n)
        for wvec, passes, redone, twice in ((rng.standard_normal(n), False, False, False), (rng.standard_normal(n), True, False, False),
                                            (cancelling, False, True, False), (cancelling, True, False, True)):
            g.upload(9, wvec)
            g.orth_device_passes(passes)
            g.orth_split(5, 2)  # basis: slots 0, 1 and 5, 6
            g.orth_begin(9, 0, 4, True)
            h, nrm = g.orth_end()
            got = g.download_slots(9, 1)[:, 0]
            href = B.T @ wvec
            wref = wvec - B @ href
            h2 = B.T @ wref
            wref -= B @ h2
            assert (g.orth_redone, g.orth_twice) == (redone, twice)
            np.testing.assert_allclose(h, href + h2, rtol=0, atol=1e-12 * np.max(np.abs(href)))
            assert abs(nrm - np.linalg.norm(wref)) <= 1e-12 * nrm
            assert np.max(np.abs(got - wref / np.linalg.norm(wref))) < 1e-12
            assert np.max(np.abs(Q[:, [2, 3, 4, 7]].T @ got)) > 1e-5  # the slots in between were NOT part of the basis
        # the setting is for one step: the next one takes the plain range again
        g.upload(9, rng.standard_normal(n))
        g.orth_device_passes(False)
        g.orth_begin(9, 0, 8, True)
        g.orth_end()
        assert np.max(np.abs(Q.T @ g.download_slots(9, 1)[:, 0])) < 1e-13
    finally:
        g.close()


def test_pinned_cache_keeps_the_sizes_in_use(hip, ctx, monkeypatch):
    """The cache of page-locked result blocks (`_hip.pinned_empty`): collected blocks are reused by the next request of their
    size; when the cache is full, blocks of OTHER sizes make room (a pipeline that has moved on to larger meshes keeps
    the blocks it turns over now - with the round-3 rule a 1M-vertex step paid two 84 MB hipHostMalloc per pass in half of
    the bench processes); a block larger than the whole cache goes back to the system."""
    import gc

    hip.pinned_trim()
    monkeypatch.setattr(hip, "_PINNED_CACHE_BYTES", 64 << 20)
    try:
        small = [hip.pinned_empty((1 << 20,)) for _ in range(6)]  # 6 x 8 MB
        ptrs_small = {a.ctypes.data for a in small}
        del small
        gc.collect()
        assert hip._pinned_cached[0] == 6 * (8 << 20)
        again = hip.pinned_empty((1 << 20,))
        assert again.ctypes.data in ptrs_small and hip._pinned_cached[0] == 5 * (8 << 20)  # reused, not allocated
        del again
        gc.collect()
        big = [hip.pinned_empty((3 << 20,)) for _ in range(2)]  # 2 x 24 MB: 48 + 48 > 64
        ptrs_big = {a.ctypes.data for a in big}
        del big
        gc.collect()
        # both large blocks are kept; small ones made room, largest-first among the OTHER sizes (all 8 MB here)
        assert len(hip._pinned_free.get(24 << 20, [])) == 2 and hip._pinned_cached[0] <= 64 << 20
        assert len(hip._pinned_free.get(8 << 20, [])) == 2
        b2 = [hip.pinned_empty((3 << 20,)) for _ in range(2)]
        assert {a.ctypes.data for a in b2} == ptrs_big
        del b2
        huge = hip.pinned_empty((9 << 20,))  # 72 MB > the whole cache: never kept
        del huge
        gc.collect()
        assert hip._pinned_free.get(72 << 20, []) == [] and hip._pinned_cached[0] <= 64 << 20
    finally:
        hip.pinned_trim()
    assert hip._pinned_cached[0] == 0


def test_orth_local_one_launch_bit_identical(hip, ctx):
    """A local Gram-Schmidt step in ONE launch (`k_orth_local`: dot products, the meeting of the graph's blocks at a
    counter, projection of the rows still held in registers) against the two launches of every other step
    (`pf_orth_one_launch(0)`): the same bits in w, h, the norm and the verdict.  One to four vectors, one and two slot
    ranges, a step that cancels digits (the host's second pass), with and without normalisation; a pair with unequal sizes
    and counts (the smaller graph's blocks leave the shared grid early)."""
    from pyfocusr_amd.meshgen import blob_mesh

    rng = np.random.default_rng(21)
    graphs = {}
    try:
        for n in (20000, 250000, 420000):
            m = blob_mesh(n, seed=3)
            g = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
            graphs[n] = g
            g.ws_ensure(32)
            Q, _ = np.linalg.qr(rng.standard_normal((n, 10)))
            for s_ in range(10):
                g.upload(s_, Q[:, s_])
            g._Q = Q
            g.orth_device_passes(False)
            g.orth_strict(0)
        noise = {n: rng.standard_normal(n) for n in graphs}

        def vectors(n):
            Q = graphs[n]._Q
            return (("random", noise[n]), ("cancelling", 3.0 * Q[:, 0] - 2.0 * Q[:, 8] + 1e-7 * noise[n]),
                    ("mild", Q @ np.linspace(0.5, -0.4, 10) + 0.9 * noise[n] / np.linalg.norm(noise[n])))

        seen = set()
        for n, g in graphs.items():
            for label, wvec in vectors(n):
                for split, count, normalize in ((False, 4, True), (True, 4, True), (True, 3, False), (False, 1, True), (False, 2, False)):
                    out = []
                    for fused in (False, True):
                        hip.orth_one_launch(fused)
                        g.upload(20, wvec)
                        if split:
                            g.orth_split(7, 1)  # slot 0 and slots 7, 8, ...
                        g.orth_begin(20, 0, count, normalize)
                        h, nrm = g.orth_end()
                        out.append((h.copy(), nrm, g.download_slots(20, 1), bool(g.orth_redone)))
                    (h0, n0, w0, r0), (h1, n1, w1, r1) = out
                    what = (n, label, split, count, normalize)
                    assert r0 == r1 and n0 == n1 and np.array_equal(h0, h1) and np.array_equal(w0, w1), what
                    seen.add(r1)
        assert seen == {False, True}  # single passes, and steps whose verdict sent pf_orth_end into the second pass
        for na, nb in ((250000, 20000), (420000, 250000)):
            ga, gb = graphs[na], graphs[nb]
            for (la, wa), (lb, wb) in zip(vectors(na), reversed(vectors(nb))):
                out = []
                for fused in (False, True):
                    hip.orth_one_launch(fused)
                    ga.upload(20, wa)
                    gb.upload(20, wb)
                    gb.orth_split(7, 1)
                    ga.orth_begin2((20, 0, 4, True), gb, (20, 0, 3, True))
                    ha, nrma = ga.orth_end()
                    hb, nrmb = gb.orth_end()
                    out.append((ha.copy(), nrma, ga.download_slots(20, 1), bool(ga.orth_redone), hb.copy(), nrmb, gb.download_slots(20, 1), bool(gb.orth_redone)))
                for x, y in zip(*out):
                    assert np.array_equal(np.asarray(x), np.asarray(y)), (na, nb, la, lb)
    finally:
        hip.orth_one_launch(True)
        for g in graphs.values():
            g.close()


def test_resident_kernel_bit_identical(golden, hip, ctx):
    """The whole recurrence in one resident kernel (operator in registers, x in LDS, boundary rows handed over through
    memory, pf_persist.hip) against one step per launch: same bits for both operators, single and paired, equal and
    unequal degrees (short, odd, > 256 steps: the 4-slot ring wraps many times), repeated launches on one graph (the
    ring phase carries over), graphs from 15k rows (asymmetric W: window relations symmetrised) to the bench size
    (250k pair, 1024-row windows), a 400k mesh (2048-row windows) and a 700k mesh (4096-row windows)."""
    from pyfocusr_amd.meshgen import blob_mesh

    rng = np.random.default_rng(4)
    big = [blob_mesh(250000, seed=s) for s in (0, 1)]
    m = blob_mesh(60000, seed=8)
    m2, m4 = blob_mesh(400000, seed=9), blob_mesh(700000, seed=10)
    # rows wider than the 8 entries a thread keeps in registers (the rest of such a row lives in LDS): a 30k blob with
    # extra faces between every fifth vertex and pairs of its nearest neighbours
    from scipy.spatial import cKDTree

    mw = blob_mesh(30000, seed=12)
    _, nn = cKDTree(mw.points).query(mw.points[::5], k=9)
    extra = np.concatenate([np.stack([nn[:, 0], nn[:, a], nn[:, b]], axis=1) for a, b in ((1, 2), (3, 4), (5, 6), (7, 8), (2, 5))])
    wide_faces = np.concatenate([mw.faces, extra.astype(mw.faces.dtype)])
    graphs = [hip.DeviceLaplacian(golden("source_mesh_15k")["points"], golden("source_mesh_15k")["faces"], ctx=ctx),  # RW
              hip.DeviceLaplacian(golden("target_mesh_15k")["points"], golden("target_mesh_15k")["faces"], ctx=ctx),
              hip.DeviceLaplacian(m.points, m.faces, ctx=ctx),
              hip.DeviceLaplacian(big[0].points, big[0].faces, ctx=ctx),
              hip.DeviceLaplacian(big[1].points, big[1].faces, ctx=ctx),
              hip.DeviceLaplacian(m2.points, m2.faces, ctx=ctx),
              hip.DeviceLaplacian(m4.points, m4.faces, ctx=ctx),
              hip.DeviceLaplacian(mw.points, wide_faces, ctx=ctx)]
    assert graphs[-1].max_degree > 10  # (its widest SELL slices overflow the register entries)
    try:
        for g in graphs:
            g.ws_ensure(4)
            g.upload(0, rng.standard_normal(g.n))

        def run(on, two_step=1, halves=True, hold=None):
            hip.persist_enable(on)
            hip.persist_two_step(two_step)
            hip.persist_pair_halves(halves)
            if hold is None:
                os.environ.pop("PF_PERSIST_HOLD", None)
            else:
                os.environ["PF_PERSIST_HOLD"] = str(hold)
            ctx.timing_enable(True)
            ctx.timing(reset=True)
            out = []
            for g in graphs:
                for p, rho in ((8, 1.0), (9, 1.0), (10, 1.0), (11, 1.0), (41, 1.0), (145, 1.02), (255, 1.02), (600, 1.03)):
                    g.cheb(0, 1, p, 1.03, 0.98, rho)
                    out.append(g.download_slots(1, 1).copy())
            for ia, ib, pa, pb in ((2, 1, 12, 12), (2, 0, 9, 30), (3, 4, 145, 145), (3, 4, 150, 139), (4, 2, 20, 64),
                                   (3, 4, 300, 520), (0, 1, 1, 40), (1, 0, 2, 9), (5, 3, 33, 34), (7, 2, 25, 31)):
                graphs[ia].cheb2((0, 2, pa, 1.0, 1.0, 1.0), graphs[ib], (0, 2, pb, 1.01, 0.99, 1.0))
                out.append(graphs[ia].download_slots(2, 1).copy())
                out.append(graphs[ib].download_slots(2, 1).copy())
            tm = ctx.timing(reset=True)
            ctx.timing_enable(False)
            return out, tm

        # one step per launch; resident with one step per exchange; resident with two steps per exchange where a graph
        # allows it (symmetric W, 1024-row windows: the 60k, 250k and wide-row graphs here)
        n2_before = hip.persist_state(ctx)["launches_two_step"]
        (a, tm_a), (b, tm_b) = run(False), run(True, two_step=0)
        assert hip.persist_state(ctx)["launches_two_step"] == n2_before
        c, tm_c = run(True, two_step=1)
        n2 = hip.persist_state(ctx)["launches_two_step"] - n2_before
        assert tm_a["persist_launches"] == 0 and tm_b["persist_launches"] >= 8 * len(graphs) + 6  # the path really ran
        assert tm_c["persist_launches"] == tm_b["persist_launches"] and n2 >= 6 * 4, n2  # 4 graphs alone (from their third application on)
        # the pair kernel with both halves of a block taking the graphs in the same order (b, c: opposite orders), and the
        # first fetch of a step far too early (0.2 us) and by the fixed sleep of round 2 instead of the tuned table:
        # timing knobs, never results
        (d, tm_d), (e, _), (f, _) = run(True, two_step=0, halves=False), run(True, two_step=0, hold=20), run(True, two_step=0, hold=0)
        assert tm_d["persist_launches"] == tm_b["persist_launches"]
        assert len(a) == len(b) == len(c) == len(d) == len(e) == len(f)
        for i, (x, y, z) in enumerate(zip(a, b, c)):
            assert np.all(np.isfinite(x)) and np.array_equal(x, y), i
            assert np.array_equal(x, z), ("two steps per exchange", i, float(np.max(np.abs(x - z))))
            assert np.array_equal(x, d[i]) and np.array_equal(x, e[i]) and np.array_equal(x, f[i]), ("halves / hold", i)
        hip.persist_two_step(2)  # (the paired level of earlier versions: reads as 1)
        assert hip.persist_state(ctx)["two_step"] == 1
    finally:
        hip.persist_enable(True)  # the defaults
        hip.persist_two_step(1)
        hip.persist_pair_halves(True)
        os.environ.pop("PF_PERSIST_HOLD", None)
        for g in graphs:
            g.close()


def test_resident_hold_back_calibration(hip):
    """The moment a block first asks for its neighbours' values is tried around the library's table value on a context's
    first launches of a kernel shape and then kept (pf_persist.hip: HoldCalibration): the hold-backs used move, settle
    within 12 ticks of where they began, and every launch - trial or not - returns the same bits."""
    from pyfocusr_amd.meshgen import blob_mesh

    os.environ.pop("PF_PERSIST_HOLD", None)
    ctx = hip.Context(0)  # a fresh context: nothing calibrated yet
    devs = []
    try:
        for s in (0, 1):
            m = blob_mesh(60000, seed=20 + s)
            d = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
            d.ws_ensure(4)
            d.upload(0, np.random.default_rng(s).standard_normal(d.n))
            devs.append(d)
        hip.persist_two_step(0)
        req = (0, 1, 60, 1.01, 0.99, 1.0)
        holds, outs = [], []
        for _ in range(40):
            devs[0].cheb2(req, devs[1], req)
            holds.append(hip.persist_state(ctx)["hold_ticks"])
            outs.append((devs[0].download_slots(1, 1).copy(), devs[1].download_slots(1, 1).copy()))
        assert holds[0] > 0 and len(set(holds[:12])) >= 3, holds  # the table's value and its neighbours were tried
        assert len(set(holds[-8:])) == 1 and abs(holds[-1] - holds[0]) <= 12, holds  # ... and one was kept
        for a, b in outs[1:]:
            assert np.array_equal(a, outs[0][0]) and np.array_equal(b, outs[0][1])
    finally:
        hip.persist_two_step(1)
        for d in devs:
            d.close()
        ctx.close()


def test_resident_kernel_timeout_is_survived(hip, ctx):
    """A wait of the resident kernel that gives up (forced through the library's test hook) must not cost any caller
    the result: the library reports PF_E_PERSIST_TIMEOUT once, with its stream drained and the path switched off, and
    every driver repeats the solve one step per launch - the paired Python driver, the single-graph driver
    (`Graph.get_graph_spectrum`), `recursive_eig` on a plain matrix, and the C entry `pf_eigs_smallest`."""
    from pyfocusr_amd import Graph, recursive_eig
    from pyfocusr_amd.graph import compute_spectra
    from pyfocusr_amd.meshgen import blob_mesh

    meshes = [blob_mesh(60000, seed=s) for s in (3, 4)]

    def pair():
        graphs = [Graph(m, n_spectral_features=4, n_rand_samples=10**9, ctx=ctx, verbose=False) for m in meshes]
        compute_spectra(graphs)
        vals = [g.eig_vals.copy() for g in graphs]
        for g in graphs:
            g.device.close()
        return vals

    def single():
        g = Graph(meshes[0], n_spectral_features=4, n_rand_samples=10**9, ctx=ctx, verbose=False)
        g.get_graph_spectrum()
        vals = g.eig_vals.copy()
        g.device.close()
        return [vals]

    def spread(v):  # 10 bits -> every third bit
        v = v.astype(np.uint64) & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249

    # a matrix carries no geometry to renumber by: the resident kernel covers it when its own order is local (Morton here)
    pts = meshes[1].points
    q = ((pts - pts.min(axis=0)) / np.ptp(pts, axis=0) * 1023.0).astype(np.uint64)
    order = np.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2), kind="stable")
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    L_local = sparse.csr_matrix(orc.graph_matrices(pts[order], inv[meshes[1].faces])[3])

    def plain_matrix():
        return [recursive_eig(L_local, k=5, n_k_needed=4)[0]]

    def c_call():
        dev = hip.DeviceLaplacian(meshes[0].points, meshes[0].faces, ctx=ctx)
        vals = dev.eigs_smallest(4)[0]
        dev.close()
        return [vals]

    rough = [np.delete(m.faces, [5, 900, 4000, 4001, 20000], axis=0) for m in meshes]  # a few one-way edges: Arnoldi on L

    def c_pair_asymmetric():
        da, db = (hip.DeviceLaplacian(m.points, f, ctx=ctx) for m, f in zip(meshes, rough))
        (va, _, sa), (vb, _, sb) = da.eigs_smallest2(db, 4, 4)
        assert sa["mode"] == 1 and sb["mode"] == 1
        da.close()
        db.close()
        return [va, vb]

    def python_pair():
        from pyfocusr_amd import graph as graph_mod

        graph_mod.PAIR_DRIVER = "python"
        try:
            return pair()
        finally:
            graph_mod.PAIR_DRIVER = "c"

    def resident_launches(fn):
        ctx.timing_enable(True)
        ctx.timing(reset=True)
        out = fn()
        n = ctx.timing(reset=True)["persist_launches"]
        ctx.timing_enable(False)
        return out, n

    try:
        for fn in (pair, python_pair, single, plain_matrix, c_call, c_pair_asymmetric):  # (pair: pf_eigs_smallest2)
            hip.persist_enable(True)
            good, n_good = resident_launches(fn)
            assert n_good > 0, fn.__name__  # the resident kernel is what normally runs here
            hip.persist_enable(True)
            hip.persist_test_hook(1)  # the next resident launch gives up at once
            survived, n_after = resident_launches(fn)
            assert 1 <= n_after <= 4 and n_after < n_good, (fn.__name__, n_after, n_good)  # aborted launch(es queued before the report), then the path is off
            for x, y in zip(good, survived):
                np.testing.assert_allclose(x, y, rtol=1e-9, err_msg=fn.__name__)
        # a raw filter application surfaces the distinct status code at the next synchronising call, once
        hip.persist_enable(True)
        dev = hip.DeviceLaplacian(meshes[0].points, meshes[0].faces, ctx=ctx)
        dev.ws_ensure(4)
        dev.upload(0, np.ones(dev.n))
        hip.persist_test_hook(1)
        dev.cheb(0, 1, 20, 1.0, 1.0, 1.0)
        with pytest.raises(hip.PfError) as err:
            ctx.sync()
        assert err.value.code == hip.PF_E_PERSIST_TIMEOUT
        ctx.sync()  # drained and cleared: no second report
        dev.cheb(0, 1, 20, 1.0, 1.0, 1.0)  # one step per launch now
        ref = dev.download_slots(1, 1).copy()
        hip.persist_enable(True)
        dev.cheb(0, 2, 20, 1.0, 1.0, 1.0)  # resident again (ring refilled after the abort): same bits
        assert np.array_equal(dev.download_slots(2, 1), ref)
        # the suspension ends by itself: after a timeout the next 64 x 2^(timeouts so far - 1) applications (capped) run
        # one step per launch, then the resident path is back without anybody asking
        hip.persist_test_hook(1)
        dev.cheb(0, 1, 20, 1.0, 1.0, 1.0)
        with pytest.raises(hip.PfError):
            ctx.sync()
        st = hip.persist_state(ctx)
        assert st["enabled"] == 1 and st["suspended_for"] >= 64 and st["timeouts"] >= 6
        rearms, launches = st["rearms"], st["launches"]
        for _ in range(st["suspended_for"]):
            dev.cheb(0, 1, 8, 1.0, 1.0, 1.0)
        ctx.sync()
        st = hip.persist_state(ctx)
        assert st["suspended_for"] == 0 and st["rearms"] == rearms + 1 and st["launches"] == launches  # all of them streamed
        dev.cheb(0, 2, 20, 1.0, 1.0, 1.0)
        ctx.sync()
        assert hip.persist_state(ctx)["launches"] == launches + 1 and np.array_equal(dev.download_slots(2, 1), ref)
        # a second context: the path moves to whoever uses it, once the previous owner's launches have completed
        ctx2 = hip.Context(ctx.device)
        try:
            dev2 = hip.DeviceLaplacian(meshes[1].points, meshes[1].faces, ctx=ctx2)
            dev2.ws_ensure(4)
            dev2.upload(0, np.ones(dev2.n))
            assert hip.persist_state(ctx)["owner"] == 1 and hip.persist_state(ctx2)["owner"] == -1
            switches, launches = hip.persist_state(ctx)["owner_switches"], hip.persist_state(ctx)["launches"]
            hip.persist_enable(False)
            dev2.cheb(0, 1, 20, 1.0, 1.0, 1.0)
            ref2 = dev2.download_slots(1, 1).copy()
            hip.persist_enable(True)
            dev2.cheb(0, 2, 20, 1.0, 1.0, 1.0)
            ctx2.sync()
            st = hip.persist_state(ctx2)
            assert st["owner"] == 1 and st["owner_switches"] == switches + 1 and st["launches"] == launches + 1
            assert np.array_equal(dev2.download_slots(2, 1), ref2)
            dev.cheb(0, 2, 20, 1.0, 1.0, 1.0)  # ... and back
            ctx.sync()
            assert hip.persist_state(ctx)["owner"] == 1 and hip.persist_state(ctx)["launches"] == launches + 2
            assert np.array_equal(dev.download_slots(2, 1), ref)
            dev2.close()
        finally:
            ctx2.close()
        dev.close()
    finally:
        hip.persist_test_hook(0)
        hip.persist_enable(True)


def test_eigs_smallest_single_c_call(golden, hip, ctx):
    """`pf_eigs_smallest` (the eigensolve as ONE C call; symmetric W here) against the golden eigenpairs of the reference,
    the oracle on synthetic and multi-component meshes, and its documented refusals."""
    from pyfocusr_amd import PolyMesh  # noqa: F401
    from pyfocusr_amd.meshgen import blob_mesh

    for name in ("target_mesh", "source_mesh"):
        g = golden(name)
        dev = hip.DeviceLaplacian(g["points"], g["faces"], ctx=ctx)
        vals, vecs, st = dev.eigs_smallest(6, minmax=True)
        np.testing.assert_allclose(vals, g["k6_eig_vals"], rtol=1e-8)
        assert np.max(np.abs(vecs - g["k6_eig_vecs"])) < 2e-9
        assert st["max_residual"] < 1e-10 and st["n_null"] == 1 and st["matvecs"] > 0
        raw = dev.eigs_smallest(3)[1]
        assert np.max(np.abs(raw - g["k3_eig_vecs_raw"])) < 2e-9
        dev.close()
    # two blobs + stray points: two locked null vectors, isolated vertices masked
    a, b = blob_mesh(3000, seed=3), blob_mesh(2000, seed=4)
    pts = np.concatenate([a.points, b.points + 200.0, np.zeros((3, 3))])
    faces = np.concatenate([a.faces, b.faces + 3000])
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    ref = orc.graph_spectrum(pts, faces, 4)
    vals, vecs, st = dev.eigs_smallest(4)
    np.testing.assert_allclose(vals, ref["eig_vals"][:4], rtol=1e-8)
    assert st["n_null"] == 2 and vecs.shape == (5003, 4) and np.all(vecs[-3:] == 0)
    dev.close()
    # larger: against the oracle's L
    m = blob_mesh(60000, seed=21)
    dev = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    vals, vecs, st = dev.eigs_smallest(5)
    W, deg, d_inv, L = orc.graph_matrices(m.points, m.faces)
    R = L @ vecs - vecs * vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-10 and np.all(np.diff(vals) > 0)
    np.testing.assert_allclose(np.linalg.norm(vecs, axis=0), 1.0, rtol=1e-12)
    dev.close()
    # small meshes (the strict second-pass rule of the Gram-Schmidt step applies below 4096 vertices, whatever an earlier
    # solve left on the graph): eigenvalues against the oracle, residuals, orthonormality in the D-inner product of L
    for n_small, seed in ((700, 5), (1500, 6), (3500, 7)):
        m = blob_mesh(n_small, seed=seed)
        dev = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
        dev.orth_strict(False)  # a previous driver's loose setting must not leak into the C driver
        vals, vecs, st = dev.eigs_smallest(6)
        ref = orc.graph_spectrum(m.points, m.faces, 6)
        np.testing.assert_allclose(vals, ref["eig_vals"][:6], rtol=1e-8)
        W, deg, d_inv, L = orc.graph_matrices(m.points, m.faces)
        assert np.max(np.linalg.norm(L @ vecs - vecs * vals[None, :], axis=0)) < 1e-10 and st["max_residual"] < 1e-10
        gram = vecs.T @ ((deg + 1e-8)[:, None] * vecs)  # L = G (D - W) is self-adjoint in the G^-1 inner product
        off = gram - np.diag(np.diag(gram))
        assert np.max(np.abs(off)) < 1e-9 * np.max(np.abs(np.diag(gram)))
        dev.close()
    # refusal: graphs too small for the filtered iteration (the Python driver's unfiltered mode covers them)
    t = blob_mesh(40, seed=1)
    dev = hip.DeviceLaplacian(t.points, t.faces, ctx=ctx)
    with pytest.raises(hip.PfError) as err:
        dev.eigs_smallest(5)
    assert err.value.code == hip.PF_E_STATE
    dev.close()


def test_eigs_c_call_asymmetric_w(golden, hip, ctx):
    """The general branch of the C driver (round 4: restarted Arnoldi in pf_krylov.h, what both bundled 15k meshes take -
    graph.py:178 writes directed entries, their scans have one-way edges): `pf_eigs_smallest_ex` against the reference's
    golden eigenpairs, the pair call against two single calls and against the Python generators, an open surface
    (complex low eigenvalues: ellipse filter), a messy closed blob (interval filter, ~50 outliers' worth of one-way
    edges), and the public path on top of it."""
    from pyfocusr_amd import Graph, PolyMesh
    from pyfocusr_amd import graph as graph_mod
    from pyfocusr_amd.graph import compute_spectra
    from pyfocusr_amd.meshgen import messy_blob_mesh

    devs = {}
    for name, m_out in (("target_mesh_15k", 5), ("source_mesh_15k", 9)):  # (source: 3 nulls -> the widen rule ends with 9 columns)
        g = golden(name)
        dev = devs[name] = hip.DeviceLaplacian(g["points"], g["faces"], ctx=ctx)
        assert not dev.symmetric and 0 < dev.n_oneway <= 32
        vals, vecs, st = dev.eigs_smallest(m_out, minmax=True)
        m = min(m_out, len(g["k5_eig_vals"]))
        assert st["mode"] == 1 and len(vals) == m_out and st["n_null"] == dev.n_components and st["degree"] <= 128
        np.testing.assert_allclose(vals[:m], g["k5_eig_vals"][:m], rtol=1e-8)
        assert np.max(np.abs(vecs[:, :m] - g["k5_eig_vecs"][:, :m])) < 5e-7
        assert st["residuals"].max() < 1e-9 and st["max_residual"] == st["residuals"].max()
    # the two of them in shared launches, downloads left in flight: what two single calls return
    dt, ds = devs["target_mesh_15k"], devs["source_mesh_15k"]
    before = hip.persist_state(ctx)["launches"]
    (vt, xt, stt), (vs, xs, sts) = dt.eigs_smallest2(ds, 5, 9, minmax=True, wait=False)
    assert hip.persist_state(ctx)["launches"] > before or not hip.persist_state(ctx)["enabled"]  # the resident filter kernel serves L = G (D - W) too
    dt.finalize_wait()
    ds.finalize_wait()
    for dev, vals, vecs, m_out in ((dt, vt, xt, 5), (ds, vs, xs, 9)):
        v1, x1, s1 = dev.eigs_smallest(m_out, minmax=True)
        np.testing.assert_allclose(vals, v1, rtol=1e-12)
        assert np.max(np.abs(vecs - x1)) < 1e-9
    for dev in devs.values():
        dev.close()
    # the public path takes the C driver for them (and the Python generators agree)
    results = {}
    for driver in ("c", "python"):
        graph_mod.PAIR_DRIVER = driver
        try:
            gs = [Graph(mesh_of(golden(n)), n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False)
                  for n in ("target_mesh_15k", "source_mesh_15k")]
            compute_spectra(gs)
            results[driver] = [(g.eig_vals.copy(), g.eig_vecs.copy(), g.eigs_stats) for g in gs]
            for g in gs:
                g.device.close()
        finally:
            graph_mod.PAIR_DRIVER = "c"
    for (vc, xc, sc), (vp, xp, sp) in zip(results["c"], results["python"]):
        assert getattr(sc, "mode", None) == 1 and xc.shape == xp.shape
        np.testing.assert_allclose(vc, vp, rtol=1e-9)
        assert np.max(np.abs(xc - xp)) < 5e-7
    # an open surface: 712 one-way boundary edges, complex low eigenvalues -> ellipse filter inside the C call
    nx, ny = 100, 80
    r = np.random.default_rng(0)
    x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float), indexing="ij")
    pts = np.stack([x, y, 0.3 * np.sin(x / 5) + 0.2 * np.cos(y / 7)], -1).reshape(-1, 3) + 0.05 * r.normal(size=(nx * ny, 3))
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    ref = orc.graph_spectrum(pts, faces, 5)
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    vals, vecs, st = dev.eigs_smallest(6)
    assert st["mode"] == 2 and len(vals) >= 5
    m = min(len(vals), len(ref["eig_vals"]))
    np.testing.assert_allclose(vals[:m], ref["eig_vals"][:m], rtol=1e-7)
    assert np.isclose(vals[0], vals[1], rtol=1e-9)
    dev.close()
    # a closed blob with the defect classes of the scans: interval filter, the outliers carried
    mesh = messy_blob_mesh(30000, seed=2)
    ref = orc.graph_spectrum(mesh.points, mesh.faces, 5)
    gr = Graph(mesh, n_spectral_features=5, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    assert gr.device.n_isolated == 3 and gr.device.n_oneway > 32 and gr.eigs_stats.mode == 1
    assert gr.eig_vals.shape == ref["eig_vals"].shape
    np.testing.assert_allclose(gr.eig_vals, ref["eig_vals"], rtol=1e-8)
    L = ref["L"]
    raw = gr.device.eigs_smallest(len(gr.eig_vals))[1]
    assert np.max(np.linalg.norm(L @ raw - raw * gr.eig_vals[None, :], axis=0)) < 1e-9
    gr.device.close()


def test_large_hole_needs_taller_ellipse(ctx):
    """Regression (found by a randomised sweep): a 150k blob with one large cap removed — 156 one-way boundary edges next
    to 1279 stranded vertices.  The first ellipse is too flat, the dominant subspace of the filter then holds only null
    directions; the solver must retry with a taller ellipse instead of handing an empty block to the device.  (The
    reference's widen-and-retry loop would need k > 1280 here.)"""
    from pyfocusr_amd import Graph, PolyMesh
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(150000, seed=118838)
    faces = m.faces[np.linalg.norm(m.points[m.faces].mean(1) - m.points[0], axis=1) > 6.0]
    gr = Graph(PolyMesh(m.points, faces), n_spectral_features=5, norm_eig_vecs=False, n_rand_samples=10**9, ctx=ctx, verbose=False)
    gr.get_graph_spectrum()
    assert gr.device.n_isolated == 1279 and not gr.device.symmetric
    assert len(gr.eig_vals) >= 5 and np.all(gr.eig_vals > 1e-10) and np.all(np.diff(gr.eig_vals) >= 0)
    gr.get_laplacian_matrix()
    R = gr.laplacian_matrix @ gr.eig_vecs - gr.eig_vecs * gr.eig_vals[None, :]
    res = np.linalg.norm(R, axis=0)
    real = np.ones(len(res), dtype=bool)  # a complex pair is reported as a repeated real part (reference semantics)
    dup = np.isclose(gr.eig_vals[:-1], gr.eig_vals[1:], rtol=1e-9)
    real[:-1] &= ~dup
    real[1:] &= ~dup
    assert np.all(res[real] < 1e-9)


@pytest.mark.parametrize("kind", ["unnormalised", "random_walk", "shifted"])
def test_recursive_eig_on_non_mesh_matrices(kind):
    """Regression (randomised sweep): `recursive_eig` on Laplacians that do not come from a mesh — widely varying
    weights, a spectrum whose low end is far below k/n of its top (the filter narrows itself), G = I (the locked null
    vector is the constant one), or no null vector at all."""
    from scipy.sparse.linalg import eigs, eigsh
    from scipy.spatial import cKDTree

    from pyfocusr_amd import recursive_eig

    rng = np.random.default_rng(31)
    n, nn, k = 4000, 6, 5
    P = rng.random((n, 2))
    d, j = cKDTree(P).query(P, k=nn + 1)
    W = sparse.csr_matrix((1.0 / (d[:, 1:].ravel() + 1e-3), (np.repeat(np.arange(n), nn), j[:, 1:].ravel())), shape=(n, n))
    W = W.maximum(W.T)
    far = rng.integers(0, n, size=(80, 2))
    far = far[far[:, 0] != far[:, 1]]
    E = sparse.csr_matrix((np.full(len(far), 0.05), (far[:, 0], far[:, 1])), shape=(n, n))
    W = W + E.maximum(E.T)  # connected
    deg = np.asarray(W.sum(axis=1))[:, 0]
    if kind == "unnormalised":
        A = (sparse.diags(deg) - W).tocsr()
        ref = eigsh(A, k=k + 1, sigma=-1e-2, which="LM")[0]
    elif kind == "random_walk":
        A = (sparse.diags(1.0 / deg) @ (sparse.diags(deg) - W)).tocsr()
        ref = np.real(eigs(A, k=k + 1, sigma=-1e-6, which="LM")[0])
    else:
        A = (sparse.diags(deg) - W + 0.37 * sparse.eye(n)).tocsr()
        ref = eigsh(A, k=k + 1, sigma=-1e-2, which="LM")[0]
    ref = np.sort(ref[ref > 1e-10])[:k]
    vals, vecs = recursive_eig(A, k=k + 1, n_k_needed=k)
    np.testing.assert_allclose(np.sort(vals)[:len(ref)], ref, rtol=1e-8)
    R = A @ vecs - vecs * vals[None, :]
    assert np.max(np.linalg.norm(R, axis=0)) < 1e-8 * abs(A).sum(axis=1).max()
