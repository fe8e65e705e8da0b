"""Exact k-nearest-neighbour search (`pf_knn_topk`, `pyfocusr_amd.neighbours`) against tests/_knn_ref.py.

CPU: the entry point is declared and bound; the argument checks need no library; the inverse-distance average on a
hand-made case and against the reference's per-point loop.  GPU: indices AND squared distances bit for bit
(`np.array_equal`) against the brute force at every depth the hierarchy kernel is instantiated for, at the edges of
leaves (64 points) and supers (4096), beyond 64 supers, for ragged query groups, exact ties, queries far outside and on
the references, NaN queries, the wide depths 17 .. 128; agreement with `knn`, `knn1` and `knn1_wide`; repeatability and
the refusals; `Focusr.get_weighted_final_node_locations(6)` and `soft_p2p_from_functional_map`.
"""
import functools
import os
import re

import numpy as np
import pytest

import _knn_ref as kr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def cloud(n, d, seed=0):
    return np.random.default_rng(100000 * seed + 1000 * d + n).standard_normal((n, d))


# ------------------------------------------------------------------------------------------------------ CPU
def test_entry_point_is_declared_and_bound():
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_knn_topk\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_knn_topk is not declared in the header"
    assert len(m.group(1).split(",")) == 9
    _, argtypes = _hip.SIGNATURES["pf_knn_topk"]
    assert len(argtypes) == 9


REFUSED = [
    ("k = 0", (10, 3), (5, 3), 0),
    ("k = 65", (100, 3), (5, 3), 65),
    ("k > n_ref", (10, 3), (5, 3), 11),
    ("d = 129", (10, 129), (5, 129), 1),
    ("1-D ref", (10,), (5, 3), 1),
    ("1-D qry", (10, 3), (5,), 1),
    ("unequal d", (10, 3), (5, 4), 1),
]


@pytest.mark.parametrize("what,ref_shape,qry_shape,k", REFUSED, ids=[r[0] for r in REFUSED])
def test_argument_checks_need_no_library(monkeypatch, what, ref_shape, qry_shape, k):
    from pyfocusr_amd import _hip, k_nearest_neighbours

    def never(*a, **kw):
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(_hip, "default_context", never)
    ref, qry = np.zeros(ref_shape), np.zeros(qry_shape)
    with pytest.raises(ValueError):
        k_nearest_neighbours(ref, qry, k)
    with pytest.raises(ValueError):
        _hip.Context.knn_topk(object.__new__(_hip.Context), ref, qry, k)  # (no device behind it: the checks come first)


def test_inverse_distance_average_by_hand():
    from pyfocusr_amd import inverse_distance_average

    values = np.array([[7.0, 0.0, 0.0], [0.0, 7.0, 0.0], [0.0, 0.0, 7.0], [1.5, -2.5, 3.5]])
    idx = np.array([[0, 1, 2], [2, 3, 1], [3, 0, 3]])
    d2 = np.array([[1.0, 4.0, 16.0],   # distances 1, 2, 4: weights 1, 1/2, 1/4 of 7/4 = 4/7, 2/7, 1/7
                   [0.25, 0.0, 9.0],   # a zero distance: that neighbour's values exactly
                   [0.0, 0.0, 0.0]])   # several: the first
    out = inverse_distance_average(values, idx, d2)
    assert out.shape == (3, 3)
    np.testing.assert_allclose(out[0], [4.0, 2.0, 1.0], rtol=4 * np.finfo(np.float64).eps, atol=0)
    assert np.array_equal(out[1], values[3])
    assert np.array_equal(out[2], values[3])


def test_inverse_distance_average_matches_the_reference_loop():
    from oracle import reference_port as orc
    from pyfocusr_amd import inverse_distance_average

    rng = np.random.default_rng(5)
    target, pts_t = rng.standard_normal((200, 3)), rng.standard_normal((200, 3))
    qry = np.concatenate([rng.standard_normal((197, 3)), target[[4, 90, 150]]])  # three coincide with a vertex
    idx, d2 = kr.brute(target, qry, 6)
    out = inverse_distance_average(pts_t, idx, d2)
    np.testing.assert_allclose(out, orc.weighted_final_node_locations(target, qry, pts_t, n_closest_pts=6), rtol=1e-12, atol=0)
    assert np.array_equal(out[197:], pts_t[[4, 90, 150]])


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def check(ctx, ref, qry, ks, brute=kr.brute):
    """The device's rows for every k of `ks` against ONE brute force at the largest (a shorter list is its prefix)."""
    ridx, rd2 = brute(ref, qry, max(ks))
    for k in ks:
        idx, d2 = ctx.knn_topk(ref, qry, k)
        assert idx.dtype == np.int64 and d2.dtype == np.float64 and idx.shape == d2.shape == (len(qry), k)
        assert np.array_equal(idx, ridx[:, :k]), "indices, k = %d" % k
        assert np.array_equal(d2, rd2[:, :k]), "distances, k = %d" % k
    return ridx, rd2


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 17))
def test_every_instantiated_depth(ctx, d):
    check(ctx, cloud(1000, d), cloud(203, d, seed=1), (1, 5, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("n_ref", [1, 2, 63, 64, 65, 100, 4095, 4096, 4097, 8200])
def test_leaf_and_super_edges(ctx, n_ref):
    # k = 64 at 65 and 100 references: the copies that fill the last leaf would show up as neighbours
    check(ctx, cloud(n_ref, 3), cloud(130, 3, seed=1), sorted({1, min(7, n_ref), min(64, n_ref)}))


@pytest.mark.gpu
def test_more_than_64_supers(ctx):
    n_ref = 262144 + 70  # 65 supers: the loop over the super boxes makes a second trip
    check(ctx, cloud(n_ref, 2), cloud(40, 2, seed=1), (1, 64), brute=kr.brute_argmin)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 14])  # groups of 4 and of 2 queries
@pytest.mark.parametrize("n_qry", [1, 2, 3, 5, 257])
def test_ragged_groups(ctx, d, n_qry):
    check(ctx, cloud(900, d), cloud(n_qry, d, seed=1), (1, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 3])
def test_exact_ties_on_a_lattice(ctx, d):
    ref = np.round(cloud(3000, d) * 8.0) / 8.0
    qry = np.round(cloud(300, d, seed=1) * 8.0) / 8.0
    _, rd2 = check(ctx, ref, qry, (1, 7, 64))
    assert np.mean(rd2[:, 1:] == rd2[:, :-1]) > 0.2  # (the case is what it claims to be: many equal distances)


@pytest.mark.gpu
def test_exact_ties_of_tiled_points(ctx):
    base = cloud(2000, 3)
    ref = np.tile(base, (5, 1))
    rows = np.random.default_rng(3).choice(2000, 700, replace=False)
    ridx, rd2 = check(ctx, ref, base[rows], (7,))
    assert np.array_equal(ridx[:, :5], rows[:, None] + 2000 * np.arange(5)[None, :])  # the five copies, ascending
    assert np.all(rd2[:, :5] == 0.0) and np.all(rd2[:, 5] > 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 8])
def test_queries_outside_and_on_the_references(ctx, d):
    ref = cloud(3000, d)
    width = ref.max(axis=0) - ref.min(axis=0)
    far = cloud(60, d, seed=1) + 10.0 * width * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    qry = np.concatenate([far, ref[::50]])
    ridx, rd2 = check(ctx, ref, qry, (1, 6, 64))
    assert np.array_equal(ridx[60:, 0], np.arange(0, 3000, 50)) and np.all(rd2[60:, 0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 20])
def test_nan_queries_have_no_neighbour(ctx, d):
    ref, qry = cloud(1500, d), cloud(210, d, seed=1).copy()
    bad = np.arange(0, 210, 70)
    qry[bad, np.arange(len(bad)) % d] = np.nan
    clean = np.setdiff1d(np.arange(210), bad)
    ridx, rd2 = kr.brute(ref, qry[clean], 5)
    idx, d2 = ctx.knn_topk(ref, qry, 5)
    assert np.all(idx[bad] == kr.NO_NEIGHBOUR) and np.all(d2[bad] == np.inf)
    assert np.array_equal(idx[clean], ridx) and np.array_equal(d2[clean], rd2)


@pytest.mark.gpu
def test_agrees_with_the_searches_that_exist(ctx):
    for d in (1, 2, 3, 4):
        ref, qry = cloud(2500, d), cloud(300, d, seed=1)
        for k in (1, 2, 3, 4):
            a, b = ctx.knn_topk(ref, qry, k), ctx.knn(ref, qry, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for d, one in [(2, "knn1"), (5, "knn1"), (9, "knn1"), (16, "knn1"), (17, "knn1_wide"), (40, "knn1_wide"), (128, "knn1_wide")]:
        ref, qry = cloud(2500, d), cloud(300, d, seed=1)
        idx, d2 = ctx.knn_topk(ref, qry, 1)
        ridx, rd2 = getattr(ctx, one)(ref, qry, return_d2=True)
        assert np.array_equal(idx[:, 0], ridx) and np.array_equal(d2[:, 0], rd2), (d, one)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [17, 24, 33, 128])
@pytest.mark.parametrize("n_ref", [50, 700])
def test_wide(ctx, d, n_ref):
    check(ctx, cloud(n_ref, d), cloud(90, d, seed=1), sorted({1, 3, min(64, n_ref)}))


@pytest.mark.gpu
def test_two_calls_give_the_same_bits_and_indices_alone(ctx):
    for d in (3, 10, 30):
        ref, qry = cloud(5000, d), cloud(400, d, seed=1)
        a, b = ctx.knn_topk(ref, qry, 16), ctx.knn_topk(ref, qry, 16)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(ctx.knn_topk(ref, qry, 16, return_d2=False), a[0])  # d2_out = NULL


@pytest.mark.gpu
def test_refusals_of_the_library_leave_the_context_usable(hip, ctx):
    i64p, f64p = hip.C.POINTER(hip.C.c_int64), hip.C.POINTER(hip.C.c_double)
    ref, qry = cloud(100, 3), cloud(10, 3, seed=1)
    wide = np.zeros((100, 129))
    idx, d2 = np.empty((10, 65), dtype=np.int64), np.empty((10, 65))

    def raw(r, n_ref, q, d, k, out=idx):
        hip._check(ctx._lib.pf_knn_topk(ctx._h, r.ctypes.data_as(f64p) if r is not None else None, n_ref, q.ctypes.data_as(f64p), 10, d, k,
                                        out.ctypes.data_as(i64p) if out is not None else None, d2.ctypes.data_as(f64p)))

    for r, n_ref, q, d, k in [(ref, 100, qry, 3, 0), (ref, 100, qry, 3, 65), (ref, 20, qry, 3, 21), (ref, 100, qry, 0, 1),
                              (wide, 100, wide, 129, 1), (ref, 0, qry, 3, 1)]:
        with pytest.raises(hip.PfError):
            raw(r, n_ref, q, d, k)
    with pytest.raises(hip.PfError):
        raw(None, 100, qry, 3, 1)
    with pytest.raises(hip.PfError):
        raw(ref, 100, qry, 3, 1, out=None)
    check(ctx, ref, qry, (1, 64))


@pytest.mark.gpu
def test_focusr_weighted_final_locations_with_six_neighbours(golden, ctx):
    """The recipe of test_gpu_parity.test_knn_topk_and_weighted_final_locations with n_closest_pts = 6."""
    from scipy import sparse

    from oracle import reference_port as orc
    from pyfocusr_amd import Focusr

    gt, gs, p = golden("target_mesh"), golden("source_mesh"), golden("pair_5k")
    reg = object.__new__(Focusr)
    reg._ctx = ctx
    nt = len(gt["points"])
    Wt = sparse.csr_matrix((gt["W_data"], gt["W_indices"], gt["W_indptr"]), shape=(nt, nt))
    Ws = sparse.csr_matrix((gs["W_data"], gs["W_indices"], gs["W_indptr"]), shape=(len(gs["points"]),) * 2)
    sm, proj, _ = orc.smoothed_correspondences(Wt, Ws, gt["points"], p["knn_idx_u"], 30, 10)
    proj[:5] = sm[[3, 77, 1500, 9, 4000]]  # force the coincident-vertex branch (focusr.py:415-419)
    reg.smoothed_target_coords, reg.source_projected_on_target = sm, proj

    class G(object):
        points = gt["points"]

    reg.graph_target = G()
    reg.get_weighted_final_node_locations(n_closest_pts=6)
    ref_out = orc.weighted_final_node_locations(sm, proj, gt["points"], n_closest_pts=6)
    np.testing.assert_allclose(reg.weighted_avg_transformed_points, ref_out, rtol=1e-12, atol=0)
    assert np.array_equal(reg.weighted_avg_transformed_points[:5], gt["points"][[3, 77, 1500, 9, 4000]])
    with pytest.raises(ValueError, match="64"):
        reg.get_weighted_final_node_locations(n_closest_pts=65)


@pytest.mark.gpu
def test_soft_p2p_from_functional_map(ctx):
    import _cotan_ref as cr
    from pyfocusr_amd import inverse_distance_average, soft_p2p_from_functional_map
    from pyfocusr_amd.meshgen import blob_mesh

    K = 20
    m = blob_mesh(700, seed=0)
    pts, faces = np.asarray(m.points, dtype=np.float64), np.asarray(m.faces, dtype=np.int32)
    _, vecs, _ = cr.generalized_eigs(cr.assemble(pts, faces), K)
    phi_t = np.ascontiguousarray(vecs)
    rng = np.random.default_rng(8)
    phi_s = phi_t[rng.permutation(len(phi_t))]
    Cm = np.linalg.qr(rng.standard_normal((K, K)))[0]
    Q = phi_s[:, 0:1] * Cm[0:1, :]
    for a in range(1, K):  # one term per basis function, ascending: what the function states
        Q = Q + phi_s[:, a:a + 1] * Cm[a:a + 1, :]
    idx, d2 = soft_p2p_from_functional_map(phi_t, phi_s, Cm, 5, ctx=ctx)
    ridx, rd2 = kr.brute(phi_t, Q, 5)
    assert np.array_equal(idx, ridx) and np.array_equal(d2, rd2)
    moved = inverse_distance_average(pts, idx, d2)
    assert moved.shape == (len(phi_s), 3) and np.all(np.isfinite(moved))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,d", [(1, 3), (2, 8)], ids=["grid-d3", "hierarchy-d8"])
def test_buffers_grow_and_are_reused_on_a_fresh_context(hip, mode, d):
    """The k-NN state of a context that has never searched: 200 points, then 5000 (every buffer grows), then 200 again
    (the grown buffers serve a smaller problem), different clouds each time.  In the hierarchy run a `knn_topk` between
    the second and the third search builds its own hierarchy in the same buffers.  Bits of the brute force every time."""
    ctx = hip.Context(0)
    try:
        ctx.knn_mode(mode)
        for step, n in enumerate((200, 5000, 200)):
            ref, qry = cloud(n, d, seed=10 + step), cloud(n, d, seed=20 + step)
            idx, d2 = ctx.knn1(ref, qry, return_d2=True)
            bidx, bd2 = kr.brute_argmin(ref, qry, 1)
            assert np.array_equal(idx, bidx[:, 0]) and np.array_equal(d2, bd2[:, 0]), "search %d, n = %d" % (step, n)
            if mode == 2 and step == 1:
                check(ctx, cloud(1000, d, seed=30), cloud(1000, d, seed=31), (5,))
    finally:
        ctx.close()
