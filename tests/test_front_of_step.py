"""The front of a step - pair assembly, the head of the pair solve, the workspace and the resident filter's hand-off
rings - on the device (run with `-m gpu` on an MI355X):

* nothing reads memory of the library's pool before writing it: with `pf_pool_poison(1)` every block the pool hands out
  starts as 0xFF bytes (NaN), with `pf_pool_poison(2)` as zero bytes, and single, paired, multi-component, Lanczos and
  Arnoldi solves give the same bits (the other units: tests/test_pool_hygiene.py);
* the head of a pair solve in shared launches leaves each graph's arithmetic alone: `eigs_smallest2` equals two
  `eigs_smallest` calls, in both orders, with one null vector beside two;
* CSR(W) with and without rows that lose a repeated directed edge: against the oracle, alone and in pair builds, and the
  `rows_compacted` statistic tells which way a build went;
* a graph's hand-off ring, filled while the graph is built, serves application after application and solve after solve."""
import numpy as np
import pytest
from scipy import sparse

from oracle import reference_port as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def _blob(n, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    return blob_mesh(n, seed=seed)


_meshes = {}


def _mesh(name):
    """The meshes of this file by name, made once."""
    if name not in _meshes:
        from pyfocusr_amd import PolyMesh
        from pyfocusr_amd.meshgen import messy_blob_mesh

        if name == "two_components":  # two blobs of 3000 and 2000 vertices: two locked null vectors
            a, b = _blob(3000, 13), _blob(2000, 14)
            m = PolyMesh(np.concatenate([a.points, b.points + 200.0]), np.concatenate([a.faces, b.faces + 3000]).astype(np.int32))
        elif name == "messy20000":
            m = messy_blob_mesh(20000, seed=15)
        elif name == "repeated_face":  # one face three more times: three directed edges listed four times
            a = _blob(2000, 16)
            m = PolyMesh(a.points, np.concatenate([a.faces, np.repeat(a.faces[11:12], 3, axis=0)]).astype(np.int32))
        elif name == "torus_quads":
            nu, nv = 128, 64
            uu, vv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
            au, av = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
            pts = np.stack([(3 + np.cos(av)) * np.cos(au), (3 + np.cos(av)) * np.sin(au), np.sin(av)], axis=-1).reshape(-1, 3)
            quads = np.stack([uu * nv + vv, ((uu + 1) % nu) * nv + vv, ((uu + 1) % nu) * nv + (vv + 1) % nv, uu * nv + (vv + 1) % nv], axis=-1)
            m = PolyMesh(pts, quads.reshape(-1, 4).astype(np.int32))
        else:
            kind, n, seed = name.split("_")
            assert kind == "blob"
            m = _blob(int(n), int(seed))
        _meshes[name] = m
    return _meshes[name]


def _golden_mesh(golden, name):
    from pyfocusr_amd import PolyMesh

    g = golden(name)
    return PolyMesh(g["points"], g["faces"])


# ------------------------------------------------------------------------------------------------ poisoned pool
def _solve_single(hip, ctx, mesh, k):
    dev = hip.DeviceLaplacian(mesh.points, mesh.faces, ctx=ctx)
    try:
        vals, vecs, st = dev.eigs_smallest(k, minmax=True)
        return [(vals.copy(), np.array(vecs), st["matvecs"], st["residuals"].copy())]
    finally:
        dev.close()


def _solve_pair(hip, ctx, mesh_a, mesh_b, ka, kb):
    da, db = hip.DeviceLaplacian(mesh_a.points, mesh_a.faces, ctx=ctx), hip.DeviceLaplacian(mesh_b.points, mesh_b.faces, ctx=ctx)
    try:
        out = da.eigs_smallest2(db, ka, kb, minmax=True)
        return [(vals.copy(), np.array(vecs), st["matvecs"], st["residuals"].copy()) for vals, vecs, st in out]
    finally:
        da.close()
        db.close()


def _solve_spectra(ctx, meshes, k):
    from pyfocusr_amd import Graph
    from pyfocusr_amd.graph import compute_spectra

    gs = [Graph(m, n_spectral_features=k, n_rand_samples=10**9, ctx=ctx, verbose=False) for m in meshes]
    try:
        compute_spectra(gs)  # (the pair is assembled side by side and solved by the pair driver)
        return [(g.eig_vals.copy(), np.array(g.eig_vecs), g.eigs_stats.matvecs, np.asarray(g.eigs_stats.residuals).copy()) for g in gs]
    finally:
        for g in gs:
            g.device.close()


POISON_CASES = ["single_pro", "pair", "two_components", "golden_5k_spectra", "arnoldi_15k"]


@pytest.mark.parametrize("case", POISON_CASES)
def test_poisoned_pool_changes_nothing(golden, hip, ctx, case):
    """Graphs built and solved with every pool block starting as NaN / -1 give the bits of a plain run: eigenvalues,
    eigenvectors, operator applications; the residuals are finite.  (5000 vertices: partial reorthogonalisation is on,
    the resident filter is taken; source_mesh_15k is asymmetric: the Arnoldi slots.)"""
    def run():
        if case == "single_pro":
            return _solve_single(hip, ctx, _mesh("blob_5000_11"), 5)
        if case == "pair":
            return _solve_pair(hip, ctx, _mesh("blob_5000_11"), _mesh("blob_9000_12"), 5, 4)
        if case == "two_components":
            return _solve_single(hip, ctx, _mesh("two_components"), 4)
        if case == "golden_5k_spectra":
            return _solve_spectra(ctx, [_golden_mesh(golden, "target_mesh"), _golden_mesh(golden, "source_mesh")], 6)
        return _solve_single(hip, ctx, _golden_mesh(golden, "source_mesh_15k"), 5)

    lib = hip.load_library()
    results = {}
    try:
        for on in (0, 1, 2):  # off, 0xFF bytes, zero bytes
            assert lib.pf_pool_poison(on) == 0
            results[on] = run()
    finally:
        lib.pf_pool_poison(0)
    for on in (1, 2):
        assert len(results[0]) == len(results[on])
        for (v0, x0, m0, r0), (v1, x1, m1, r1) in zip(results[0], results[on]):
            assert len(v0) > 0 and np.array_equal(v0, v1)
            assert np.array_equal(x0, x1)
            assert m0 == m1
            assert np.all(np.isfinite(r0)) and np.all(np.isfinite(r1)) and np.all(np.isfinite(x1))


# ------------------------------------------------------------------------------------------------ the pair's head
@pytest.mark.parametrize("names", [("blob_5000_11", "blob_9000_12"), ("blob_9000_12", "blob_5000_11"),
                                   ("blob_5000_11", "two_components"), ("two_components", "blob_5000_11")])
def test_pair_head_equals_single_solves(hip, ctx, names):
    """`eigs_smallest2` - null vectors, norms, scalings, start vectors and first Gram-Schmidt steps of both graphs in
    shared launches - against one `eigs_smallest` per graph: the same bits, whichever graph comes first, and with one
    null vector beside two (the launches the shorter list lacks go out alone)."""
    ma, mb = _mesh(names[0]), _mesh(names[1])
    pair = _solve_pair(hip, ctx, ma, mb, 5, 4)
    for m, k, (vals, vecs, matvecs, res) in zip((ma, mb), (5, 4), pair):
        (v1, x1, m1, r1), = _solve_single(hip, ctx, m, k)
        assert len(vals) == k and np.array_equal(vals, v1)
        assert np.array_equal(vecs, x1)
        assert matvecs == m1
        assert np.array_equal(res, r1)


# ------------------------------------------------------------------------------------------------ assembly
ASSEMBLY = [("blob_3000_21", False), ("blob_20000_22", False), ("messy20000", True), ("repeated_face", True), ("torus_quads", False)]

_oracle = {}


def _oracle_matrices(name):
    if name not in _oracle:
        m = _mesh(name)
        W, deg, d_inv, L = orc.graph_matrices(m.points, m.faces)
        W, L = sparse.csr_matrix(W), sparse.csr_matrix(L)
        W.sort_indices()
        L.sort_indices()
        _oracle[name] = (W, deg, L)
    return _oracle[name]


def _assert_equals_oracle(dev, name):
    W, deg, L = _oracle_matrices(name)
    h = dev.download()
    assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices)
    assert np.array_equal(h["w"], W.data)
    assert np.array_equal(h["deg"], deg)
    # L = G (D - W): its diagonal, and its off-diagonals in the pattern of W
    rows = np.repeat(np.arange(L.shape[0]), np.diff(L.indptr))
    off = L.indices != rows
    assert np.array_equal(h["l_diag"], L.diagonal())
    assert np.array_equal(L.indices[off], W.indices) and np.array_equal(h["l_offdiag"], L.data[off])


@pytest.mark.parametrize("name,shrinks", ASSEMBLY)
def test_assembly_with_and_without_shrinking_rows(hip, ctx, name, shrinks):
    """CSR(W), deg and L of a single build against the oracle, bit for bit; `rows_compacted` says whether a row lost a
    repeated directed edge - no row of a closed manifold mesh does, and the build then skips the compaction pass."""
    m = _mesh(name)
    dev = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    try:
        assert dev.rows_compacted is shrinks
        _assert_equals_oracle(dev, name)
    finally:
        dev.close()


@pytest.mark.parametrize("names", [("blob_20000_22", "messy20000"), ("messy20000", "blob_20000_22"),
                                   ("blob_3000_21", "repeated_face"), ("repeated_face", "torus_quads")])
def test_pair_build_of_clean_and_shrinking_meshes(hip, ctx, names):
    """One launch of the sort and of the compaction serves a mesh that takes the short path and one that does not: each
    graph of the pair equals its single build key by key, its operator included, and the oracle."""
    rng = np.random.default_rng(7)
    ms = [_mesh(n) for n in names]
    dm = [hip.DeviceMesh(m.points, m.faces, ctx=ctx) for m in ms]
    pair = hip.DeviceLaplacian.build_pair(*dm)
    try:
        for name, m, paired in zip(names, ms, pair):
            single = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
            try:
                hp, hs = paired.download(labels=True), single.download(labels=True)
                for key in hs:
                    assert np.array_equal(hp[key], hs[key]), key
                assert paired.rows_compacted is single.rows_compacted is dict(ASSEMBLY)[name]
                assert (paired.symmetric, paired.n_isolated, paired.n_components, paired.max_degree, paired.n_oneway, paired.spectral_bound) == \
                       (single.symmetric, single.n_isolated, single.n_components, single.max_degree, single.n_oneway, single.spectral_bound)
                x = rng.standard_normal(m.points.shape[0])
                assert np.array_equal(paired.spmv_host(x), single.spmv_host(x))
            finally:
                single.close()
            _assert_equals_oracle(paired, name)
    finally:
        for p in pair:
            p.close()
        for d in dm:
            d.close()


# ------------------------------------------------------------------------------------------------ ring reuse
def test_ring_filled_at_build_is_reused(hip, ctx):
    """Filter applications and whole solves back to back on ONE graph, with the resident path switched off and on again in
    between: every result equals the streaming path's (one step per launch), bit for bit - the ring the build filled is
    as good at the last application as at the first."""
    m = _mesh("blob_5000_11")
    dev = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    hi, cut, degree = dev.spectral_bound, 0.02, 24
    c, e = 0.5 * (hi + cut), 0.5 * (hi - cut)

    def apply(seed):
        dev.start_vector(0, seed)
        dev.cheb(0, 1, degree, c, e)
        return dev.download_slots(1, 1)[0].copy()

    def solve():
        vals, vecs, st = dev.eigs_smallest(5, minmax=True)
        return vals.copy(), np.array(vecs), st

    try:
        dev.ws_ensure(2)
        before = hip.persist_state(ctx)["launches"]
        resident = [apply(1), apply(2)]
        assert hip.persist_state(ctx)["launches"] >= before + 2  # the resident path took both
        solves = [solve()]
        hip.persist_enable(False)
        streamed = [apply(1), apply(2)]
        solves.append(solve())
        hip.persist_enable(True)
        resident += [apply(1), apply(2)]
        solves.append(solve())
        solves.append(solve())
    finally:
        hip.persist_enable(True)
        dev.close()
    for i, y in enumerate(resident):
        assert np.all(np.isfinite(y)) and np.array_equal(y, streamed[i % 2])
    vals0, vecs0, st0 = solves[1]  # the streaming path's solve
    for vals, vecs, st in solves:
        assert np.array_equal(vals, vals0) and np.array_equal(vecs, vecs0)
        assert st["matvecs"] == st0["matvecs"]
