"""The device kernels of the tail of `align_maps`, called one by one against plain references of the same operation:

  1. the top-k nearest-neighbour search (`pf_knn`, k = 2..4, d <= 4: the twelve `k_knn_grid<D, K, 64, 512>` instantiations)
     against the left-to-right brute force of tests/_knn_ref.py - indices and squared distances bit for bit;
  2. the graph mean filter (`pf_mean_filter`) against the scipy product it imitates (`oracle.reference_port.
     mean_filter_graph`) - bit for bit, non-finite values included;
  3. the eigsort cost matrices (`pf_eigsort_costs`) against their definition (tests/_eigsort_ref.py), computed from the rows
     that are resident on the device, within bounds derived from the sums themselves.

The references are tested first, on the CPU (the tests without the `gpu` mark).  The sizes are the smallest at which the
path named in each test is taken.  The eigsort tests print their observed error against the derived bound
(`pytest -s`); the figures of one run are kept in profiles/tail_kernels.md.
"""
import functools

import numpy as np
import pytest
from scipy import sparse

import _eigsort_ref as er
import _knn_ref as kr
from oracle import reference_port as orc

gpu = pytest.mark.gpu

PF_E_ARG, PF_E_STATE = -1, -4


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


# ======================================================================================== 0. the references, on the CPU
def test_knn_reference_orders_ties_by_index():
    """A tie group larger than k: five references at distance 1 of the query, one nearer, one farther."""
    ref = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 0.5], [-1.0, 0.0], [0.0, -1.0], [3.0, 0.0], [1.0, 0.0]])
    qry = np.array([[0.0, 0.0], [3.0, 0.0]])
    for k in (1, 2, 3, 4):
        idx, d2 = kr.brute(ref, qry, k)
        assert np.array_equal(idx[0], [2, 0, 1, 3][:k]) and np.array_equal(d2[0], [0.25, 1.0, 1.0, 1.0][:k])
        assert np.array_equal(idx[1], [5, 1, 6, 2][:k]) and np.array_equal(d2[1], [0.0, 4.0, 4.0, 9.25][:k])
        fidx, fd2 = kr.brute_argmin(ref, qry, k)
        assert np.array_equal(fidx, idx) and np.array_equal(fd2, d2)


def test_knn_reference_equals_kdtree_without_ties():
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(1)
    for d in (1, 2, 3, 4):
        ref, qry = rng.uniform(-1, 1, (3000, d)), rng.uniform(-1, 1, (400, d))
        for k in (2, 3, 4):
            idx, d2 = kr.brute(ref, qry, k)
            assert np.all(np.diff(d2, axis=1) > 0)  # tie-free
            assert np.array_equal(idx, cKDTree(ref).query(qry, k=k)[1])
            fidx, fd2 = kr.brute_argmin(ref, qry, k, chunk=97)
            assert np.array_equal(fidx, idx) and np.array_equal(fd2, d2)
    lat = np.round(rng.uniform(-1, 1, (2000, 3)) * 4) / 4  # lattice: ties everywhere - the two forms of the brute force agree
    q = np.round(rng.uniform(-1, 1, (300, 3)) * 4) / 4
    a, b = kr.brute(lat, q, 4), kr.brute_argmin(lat, q, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_w1_reference_forms_agree():
    """scipy's `wasserstein_distance` (the definition in pf_eigsort.hip's header) against the merged-breakpoint integral
    summed exactly: unequal, coprime, equal and tied samples, plain and flipped.  scipy integrates |F_t - F_s| along x: each
    CDF value is an integer quotient (one rounding, eps/2 absolute), their difference and its product with the step round
    once more each, and the steps sum to the samples' range: 2 eps * range; then its own sum of n terms."""
    rng = np.random.default_rng(2)
    cases = [(2, 3), (3, 2), (7, 7), (255, 257), (1024, 1025), (64, 4096), (500, 500)]
    for mt, ms in cases:
        for tied in (False, True):
            t, s = rng.uniform(-0.5, 0.5, mt), rng.uniform(-0.5, 0.5, ms)
            if tied:
                t, s = np.round(t * 8) / 8, np.round(s * 8) / 8
            t[0], s[0] = -0.5, 0.5  # log meets 0 + eps on the plain side of t and on the flipped side of s
            for flip in (False, True):
                ref = er.w1_fsum(t, s, flip)
                got = er.w1_scipy(t, s, flip)
                # (the samples' range is at most 2 max|log|; scipy's logs are libm's: 1 ulp, as `w1_bound` counts a device's)
                tol = er.w1_bound(ref, log_ulps_device=1.0) + 2 * er.EPS * 2 * ref["max_abs_log"]
                assert abs(got - ref["value"]) <= tol, (mt, ms, tied, flip, got, ref["value"], tol)
                assert ref["n_terms"] == mt + ms - np.gcd(mt, ms)
    # a sample against itself is at distance 0, against its shift by c at distance c (in log space: use the definition's inverse)
    t = rng.uniform(-0.4, 0.4, 300)
    assert er.w1_fsum(t, t)["value"] == 0.0
    shifted = np.exp(np.log(t + 0.5 + er.EPS) + 0.25) - 0.5 - er.EPS
    assert abs(er.w1_fsum(t, shifted)["value"] - 0.25) < 1e-13


def test_spatial_reference():
    rng = np.random.default_rng(3)
    t, s = rng.uniform(-0.5, 0.5, 1000), rng.uniform(-0.5, 0.5, 1000)
    v, b = er.spatial_fsum(t, s)
    assert abs(v - np.sqrt(np.sum((s - t) ** 2)) / 1000) <= b
    vf, bf = er.spatial_fsum(t, s, flip=True)
    assert abs(vf - np.sqrt(np.sum((-s - t) ** 2)) / 1000) <= bf
    assert er.spatial_fsum(t, t)[0] == 0.0
    p = rng.normal(size=(50, 3))
    n = er.minmax_points(p)
    assert n.min() == 0.0 and n.max() == 1.0


# ======================================================================================== 1. top-k search
def _chunk(n_ref):
    return max(16, 3_000_000 // n_ref)


def check_topk(ctx, ref, qry, ks=(2, 3, 4), want=None):
    """The device's k nearest for every k against the first k of the brute force's four (or of `want`)."""
    widx, wd2 = want if want is not None else kr.brute_argmin(ref, qry, min(4, len(ref)), chunk=_chunk(len(ref)))
    for k in ks:
        idx, d2 = ctx.knn(ref, qry, k)
        assert idx.dtype == np.int64 and idx.shape == (len(qry), k)
        assert np.array_equal(idx, widx[:, :k]), (ref.shape, qry.shape, k, int(np.sum(idx != widx[:, :k])))
        assert np.array_equal(d2, wd2[:, :k]), (ref.shape, qry.shape, k)
    return widx, wd2


@functools.lru_cache(maxsize=None)
def _uniform_case(d):
    rng = np.random.default_rng(40 + d)
    ref, qry = rng.uniform(-0.5, 0.5, (10000, d)), rng.uniform(-0.5, 0.5, (1500, d))
    return ref, qry, kr.brute_argmin(ref, qry, 4, chunk=_chunk(10000))


@gpu
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_topk_every_instantiation(ctx, d, k):
    """Unrelated uniform clouds, 10000 references (a 50 x 50 grid; one row of 50 cells for d = 1) and 1500 queries."""
    ref, qry, want = _uniform_case(d)
    check_topk(ctx, ref, qry, ks=(k,), want=want)


@gpu
@pytest.mark.parametrize("d", [1, 3])
def test_topk_block_tails(ctx, d):
    """The block is one wave of 64 lanes and tail lanes replay the last query; fewer references than cells, so the rings
    of phase 1 run out before k candidates are found."""
    rng = np.random.default_rng(50 + d)
    for k in (2, 3, 4):
        for n_ref in sorted({k, k + 1, 5, 64}):
            ref = rng.uniform(-1, 1, (n_ref, d))
            for n_qry in (1, 63, 64, 65, 129):
                check_topk(ctx, ref, rng.uniform(-1, 1, (n_qry, d)), ks=(k,))


@gpu
def test_topk_ties(ctx):
    """Equal distances are ordered by index: lattices (8, 4, 2 equidistant references per query) in natural and in permuted
    order, every reference five times with queries that are references, one point 700 times."""
    rng = np.random.default_rng(60)
    g3 = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(12.0), indexing="ij"), -1).reshape(-1, 3)
    g2 = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij"), -1).reshape(-1, 2)
    g1 = np.arange(300.0)[:, None]
    for grid in (g3, g2, g1):
        check_topk(ctx, grid, grid + 0.5)
        perm = rng.permutation(len(grid))
        check_topk(ctx, grid[perm], grid + 0.5)
    base = rng.uniform(-1, 1, (2000, 3))
    ref = np.tile(base, (5, 1))  # point p at p, p + 2000, ..., p + 8000
    rows = rng.integers(0, 2000, 700)
    for k in (2, 3, 4):
        idx, d2 = ctx.knn(ref, base[rows].copy(), k)
        assert np.all(d2 == 0.0)
        assert np.array_equal(idx, rows[:, None] + 2000 * np.arange(k)[None, :])
    one = np.tile(rng.normal(size=(1, 4)), (700, 1))  # zero extent on every axis: one cell holds everything
    qry = rng.normal(size=(130, 4))
    widx, _ = check_topk(ctx, one, qry)
    assert np.array_equal(widx, np.tile(np.arange(4), (130, 1)))


@functools.lru_cache(maxsize=None)
def _cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "disjoint_10k":  # every rectangle is the whole grid: 50 x 50 cells > 512, the block-wide LDS scan
        ref, qry = rng.uniform(0, 1, (10000, 3)), rng.uniform(3, 4, (600, 3))
    elif name == "disjoint_30k":  # 86 grid rows > 8 and 30000 references > 4 tiles of 128: the rectangle refresh runs
        ref, qry = rng.uniform(0, 1, (30000, 4)), rng.uniform(3, 4, (600, 4))
    elif name == "disjoint_1d":  # the one-row grid scanned as a whole
        ref, qry = rng.uniform(0, 1, (10000, 1)), rng.uniform(3, 4, (300, 1))
    elif name == "two_corners":  # an empty middle: the rings find nothing, the first bounds are as wide as the grid
        ref = np.concatenate([rng.uniform(0, 0.05, (15000, 3)), rng.uniform(0.95, 1.0, (15000, 3))])
        qry = rng.uniform(0, 1, (800, 3))
    elif name == "anisotropic":  # the grid axes are the two widest; the third is six orders of magnitude narrower
        scale = np.array([1000.0, 1.0, 1e-3, 1.0])
        ref, qry = rng.uniform(0, 1, (30000, 4)) * scale, rng.uniform(0, 1, (700, 4)) * scale
    elif name == "registered":  # the lane-private path: every square lies inside the ring phase 1 has scanned
        ref = rng.uniform(0, 1, (25000, 3))
        qry = ref[rng.permutation(25000)[:3000]] + 1e-4 * rng.standard_normal((3000, 3))
    else:
        raise KeyError(name)
    return ref, qry, kr.brute_argmin(ref, qry, 4, chunk=_chunk(len(ref)))


@gpu
@pytest.mark.parametrize("name", ["disjoint_10k", "disjoint_30k", "disjoint_1d", "two_corners", "anisotropic", "registered"])
def test_topk_ring_growth_and_shared_scan(ctx, name):
    ref, qry, want = _cloud(name)
    check_topk(ctx, ref, qry, want=want)


@gpu
def test_topk_nan_queries(ctx):
    """A query with a NaN coordinate compares with nothing: k indices 0x7fffffff and k infinite distances; its neighbours in
    the block are not disturbed."""
    ref, qry, (widx, wd2) = _cloud("registered")
    qry = qry[:600].copy()
    qry[::7, 1] = np.nan
    qry[7::70] = np.nan
    ok = ~np.isnan(qry).any(axis=1)
    for k in (2, 3, 4):
        idx, d2 = ctx.knn(ref, qry, k)
        assert np.array_equal(idx[ok], widx[:600][ok][:, :k]) and np.array_equal(d2[ok], wd2[:600][ok][:, :k])
        assert np.all(idx[~ok] == kr.NO_NEIGHBOUR) and np.all(np.isposinf(d2[~ok]))


@gpu
def test_topk_switches_that_must_not_matter(ctx, monkeypatch):
    """The radix sort of the cells (PF_KNN_BUCKET_MAX=1), the 1-NN pruning modes, and 1-NN searches on the same context
    (the same device buffers) before and after."""
    ref, qry, want = _uniform_case(3)
    ref2, qry2, want2 = _cloud("disjoint_10k")
    b1 = orc.knn1_bruteforce(ref, qry)
    assert np.array_equal(b1[0], want[0][:, 0]) and np.array_equal(b1[1], want[1][:, 0])  # (the two brute forces agree)

    def one_nn():
        idx, d2 = ctx.knn1(ref, qry, return_d2=True)
        assert idx.shape == (len(qry),) and np.array_equal(idx, b1[0]) and np.array_equal(d2, b1[1])

    one_nn()
    monkeypatch.setenv("PF_KNN_BUCKET_MAX", "1")
    try:
        check_topk(ctx, ref, qry, want=want)
        check_topk(ctx, ref2, qry2, want=want2)
    finally:
        monkeypatch.delenv("PF_KNN_BUCKET_MAX")
    one_nn()
    try:
        for mode in (1, 2):
            ctx.knn_mode(mode)
            check_topk(ctx, ref, qry, want=want)
            one_nn()
            check_topk(ctx, ref2, qry2, ks=(3,), want=want2)
    finally:
        ctx.knn_mode(0)
    one_nn()


def _raw_knn1(hip, ctx, ref, qry, slots):
    """`pf_knn1` through the raw entry with output arrays of slots * n_qry entries filled with a sentinel."""
    from pyfocusr_amd._hip import _f64, _i64p

    idx = np.full(slots * len(qry), -77, dtype=np.int64)
    d2 = np.full(slots * len(qry), -77.0)
    rc = hip._lib.pf_knn1(ctx._h, _f64(ref), len(ref), _f64(qry), len(qry), ref.shape[1], idx.ctypes.data_as(_i64p), _f64(d2))
    return rc, idx, d2


@gpu
def test_topk_refusals_leave_the_context_usable(hip, ctx):
    """k = 5, k > n_ref, k = 2 with d = 5, and a `pf_knn` refused for a NULL pointer after it has named its k: each is
    followed by a correct 1-NN search on the same context, which writes n_qry entries and not one more."""
    from pyfocusr_amd._hip import _f64, _i64p

    rng = np.random.default_rng(70)
    ref, qry = rng.uniform(-1, 1, (20000, 3)), rng.uniform(-1, 1, (300, 3))
    bidx, bd2 = orc.knn1_bruteforce(ref, qry)
    small = rng.uniform(-1, 1, (3, 3))

    def one_nn_is_right():
        rc, idx, d2 = _raw_knn1(hip, ctx, ref, qry, 4)
        assert rc == 0
        assert np.array_equal(idx[:300], bidx) and np.array_equal(d2[:300], bd2)
        assert np.all(idx[300:] == -77) and np.all(d2[300:] == -77.0)
        assert np.array_equal(ctx.knn1(small, qry), orc.knn1_bruteforce(small, qry)[0])

    one_nn_is_right()
    for refuse in (lambda: ctx.knn(ref, qry, 5), lambda: ctx.knn(small, qry, 4), lambda: ctx.knn(ref, qry, 0),
                   lambda: ctx.knn(rng.uniform(-1, 1, (500, 5)), rng.uniform(-1, 1, (50, 5)), 2)):
        with pytest.raises(hip.PfError) as e:
            refuse()
        assert e.value.code == PF_E_ARG
        one_nn_is_right()
    # the raw entry with a NULL reference pointer and k = 3
    idx = np.full(4 * 300, -77, dtype=np.int64)
    d2 = np.full(4 * 300, -77.0)
    rc = hip._lib.pf_knn(ctx._h, None, len(ref), _f64(qry), len(qry), 3, 3, idx.ctypes.data_as(_i64p), _f64(d2))
    assert rc == PF_E_ARG
    assert np.all(idx == -77) and np.all(d2 == -77.0)
    one_nn_is_right()
    check_topk(ctx, ref, qry, ks=(3,))
    one_nn_is_right()


# ======================================================================================== 2. mean filter
def _hub_fan(n_stranded=0):
    """The fan of tests/test_gpu_parity.py::test_assembly_hub_vertices: a hub row of 6000 entries, a second, open fan
    (one-way edges) and a strip that joins them, in shuffled vertex order; optionally unreferenced points appended."""
    rng = np.random.default_rng(5)
    n_rim = 6000
    ang = np.linspace(0.0, 2.0 * np.pi, n_rim, endpoint=False)
    rim = np.stack([np.cos(ang) * (1 + 0.1 * rng.random(n_rim)), np.sin(ang), 0.05 * rng.standard_normal(n_rim)], axis=1)
    rim2 = rim * 0.5 + np.array([0.0, 0.0, 1.0])
    pts = np.concatenate([[[0.0, 0.0, 0.3]], rim, [[0.0, 0.0, 1.4]], rim2])
    hub2 = 1 + n_rim
    faces = [[0, 1 + i, 1 + (i + 1) % n_rim] for i in range(n_rim)]
    faces += [[hub2, hub2 + 1 + i, hub2 + 1 + (i + 1) % n_rim] for i in range(0, n_rim, 3)]
    faces += [[1 + i, hub2 + 1 + i, 1 + (i + 1) % n_rim] for i in range(0, n_rim, 2)]
    faces = np.asarray(faces, dtype=np.int32)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    pts, faces = pts[perm], inv[faces].astype(np.int32)
    if n_stranded:
        pts = np.concatenate([pts, rng.normal(size=(n_stranded, 3))])
    return pts, faces, int(inv[0])  # (the hub's index after the shuffle)


def _mesh(name):
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    if name == "hub_fan":
        return _hub_fan()[:2]
    if name == "piled":  # test_assembly_piled_vertices: nearly all vertices in one cell of the renumbering's grid
        m = blob_mesh(8000, seed=31)
        pts = np.concatenate([m.points * 1e-3, [[900.0, 0.0, 0.0], [0.0, -700.0, 0.0], [0.0, 0.0, 800.0]]])
        n0 = len(m.points)
        return pts, np.concatenate([m.faces, [[n0, n0 + 1, n0 + 2], [0, n0, n0 + 1]]]).astype(np.int32)
    if name.startswith("messy_"):
        m = messy_blob_mesh(int(name[6:]), seed=3)
        return m.points, m.faces
    if name == "unreferenced":
        m = blob_mesh(1500, seed=4)
        return np.concatenate([m.points, np.random.default_rng(4).normal(size=(40, 3)) * 50.0]), m.faces
    if name == "two_blobs":
        a, b = blob_mesh(1200, seed=5), blob_mesh(700, seed=6)
        return np.concatenate([a.points, b.points + 200.0]), np.concatenate([a.faces, b.faces + 1200]).astype(np.int32)
    if name.startswith("blob_"):
        m = blob_mesh(int(name[5:]), seed=7)
        return m.points, m.faces
    if name == "triangle":
        return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.5]]), np.array([[0, 1, 2]], dtype=np.int32)
    raise KeyError(name)


MF_GRAPHS = ["hub_fan", "piled", "messy_900", "messy_5000", "unreferenced", "two_blobs", "blob_4095", "blob_4096", "blob_4097",
             "triangle"]


def _oracle_w(pts, faces):
    """W as the reference assembles it; the kernel's contract (scipy's term order) is stated for a W without diagonal
    entries, which every mesh here gives (a face that repeats a vertex is refused by the assembly)."""
    W = sparse.csr_matrix(orc.weighted_adjacency(pts, faces))
    assert W.diagonal().sum() == 0.0 and not np.any(W.tocoo().row == W.tocoo().col)
    return W


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_mean_filter(dev, W, rng, ncols_list=(1, 2, 3, 4, 7, None), iterations=(0, 1, 2, 25)):
    n = dev.n
    stranded = np.asarray(W.sum(axis=1))[:, 0] == 0
    for ncols in ncols_list:  # None: a 1-D input
        vals = rng.standard_normal(n) if ncols is None else rng.standard_normal((n, ncols))
        for it in iterations:
            got = dev.mean_filter(vals, it)
            want = orc.mean_filter_graph(W, vals, iterations=it)
            assert got.shape == vals.shape
            assert np.array_equal(got, want), (ncols, it, float(np.max(np.abs(got - want))))
            if it == 0:
                assert same_bits(got, vals)
            assert np.array_equal(got[stranded], vals[stranded])  # a vertex without edges keeps its value exactly
    return int(stranded.sum())


@gpu
@pytest.mark.parametrize("name", MF_GRAPHS)
def test_mean_filter_equals_scipy_product(hip, ctx, name):
    """ncols 1 and 3 are compile-time instantiations, 2, 4 and 7 take the run-time-column kernel; 0 iterations return the
    input's bits.  W has no diagonal entry in any of these graphs, so the comparison is `np.array_equal`."""
    pts, faces = _mesh(name)
    W = _oracle_w(pts, faces)
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    try:
        h = dev.download()
        assert np.array_equal(h["rowptr"], W.indptr) and np.array_equal(h["colidx"], W.indices) and np.array_equal(h["w"], W.data)
        n_stranded = check_mean_filter(dev, W, np.random.default_rng(len(pts)))
        if name in ("messy_900", "messy_5000"):
            assert n_stranded == 3 and not dev.symmetric
        if name == "unreferenced":
            assert n_stranded == 40
        if name == "hub_fan":
            assert dev.max_degree >= 6000 and not dev.symmetric
    finally:
        dev.close()


@gpu
def test_mean_filter_cached_rows_and_pair_build(hip, ctx):
    """The filter's rows are built on first use and reused: several column counts in turn on one graph give the bits of a
    fresh graph per call; graphs assembled side by side (`pf_graph_build_device2`) filter like graphs built alone."""
    rng = np.random.default_rng(80)
    (pa, fa), (pb, fb) = _mesh("messy_5000"), _mesh("blob_4097")
    Wa, Wb = _oracle_w(pa, fa), _oracle_w(pb, fb)
    inputs = [rng.standard_normal((len(pa), c)) for c in (3, 1, 7, 2, 3)]
    one = hip.DeviceLaplacian(pa, fa, ctx=ctx)
    try:
        in_turn = [one.mean_filter(v, 3) for v in inputs]
    finally:
        one.close()
    for v, got in zip(inputs, in_turn):
        fresh = hip.DeviceLaplacian(pa, fa, ctx=ctx)
        try:
            assert same_bits(fresh.mean_filter(v, 3), got)
        finally:
            fresh.close()
        assert np.array_equal(got, orc.mean_filter_graph(Wa, v, iterations=3))
    ma, mb = hip.DeviceMesh(pa, fa, ctx=ctx), hip.DeviceMesh(pb, fb, ctx=ctx)
    ga, gb = hip.DeviceLaplacian.build_pair(ma, mb)
    try:
        check_mean_filter(ga, Wa, rng, ncols_list=(3, 2, None), iterations=(1, 25))
        check_mean_filter(gb, Wb, rng, ncols_list=(1, 7), iterations=(2,))
    finally:
        ga.close()
        gb.close()
        ma.close()
        mb.close()


@gpu
def test_mean_filter_non_finite_values(hip, ctx):
    """+inf at a neighbour of the hub, -inf at an ordinary vertex, NaN at a stranded vertex, a few -0.0: after 1 and 2
    iterations the result equals the scipy product's, non-finite values where it has them and nowhere else - the padding
    rows and the padding entries (0 * own value) leak nothing."""
    pts, faces, hub = _hub_fan(n_stranded=5)
    W = _oracle_w(pts, faces)
    n = len(pts)
    nbr = W.indices[W.indptr[hub]:W.indptr[hub + 1]]
    stranded = np.arange(n - 5, n)  # the appended points: in no face
    no_out_edge = np.where(np.asarray(W.sum(axis=1))[:, 0] == 0)[0]  # (the open fan leaves rim vertices without one, too)
    assert len(nbr) >= 6000 and np.isin(stranded, no_out_edge).all() and not np.isin(stranded, faces).any()
    ordinary = np.setdiff1d(np.arange(n), np.concatenate([nbr, no_out_edge, [hub]]))
    far, far2 = int(ordinary[123]), int(ordinary[4567])
    dev = hip.DeviceLaplacian(pts, faces, ctx=ctx)
    rng = np.random.default_rng(81)
    try:
        for ncols in (1, 3, 2, None):
            vals = rng.standard_normal(n) if ncols is None else rng.standard_normal((n, ncols))
            vals[nbr[17]] = np.inf
            vals[far] = -np.inf
            vals[stranded[2]] = np.nan
            vals[[int(nbr[40]), int(stranded[0]), far2]] = -0.0
            for it in (0, 1, 2):
                got = dev.mean_filter(vals, it)
                with np.errstate(invalid="ignore"):
                    want = orc.mean_filter_graph(W, vals, iterations=it)
                assert np.array_equal(got, want, equal_nan=True), (ncols, it)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
                assert np.array_equal(np.signbit(got), np.signbit(want) if it else np.signbit(vals)), (ncols, it)
                if it == 0:
                    assert same_bits(got, vals)
                if it == 1:  # one step reaches the neighbours only
                    assert np.isfinite(got[np.setdiff1d(stranded, stranded[2])]).all()
                    assert 0 < np.sum(~np.isfinite(got)) < 40 * (1 if ncols is None else ncols)
                assert np.all(np.isnan(got[stranded[2]]))
        # +inf in every row of at most t entries, for every t: wherever a SELL slice mixes row widths its narrower rows -
        # the ones that end in padding entries - are among them, and a padding entry that reached the sum would turn
        # their inf into NaN (0 * inf)
        width = np.diff(W.indptr)
        for i, t in enumerate(np.unique(width)[:-1]):
            ncols = (1, 3, 2)[i % 3]
            vals = rng.standard_normal((n, ncols))
            vals[width <= t] = np.inf
            got = dev.mean_filter(vals, 1)
            want = orc.mean_filter_graph(W, vals, iterations=1)
            assert np.array_equal(got, want, equal_nan=True), (int(t), ncols, int(np.sum(np.isnan(got))), int(np.sum(np.isnan(want))))
            assert not np.isnan(want).any() and np.isposinf(got[width <= t]).all()
    finally:
        dev.close()


# ======================================================================================== 3. eigsort costs
ES_COUNTS = [(2, 3), (3, 2), (255, 257), (1024, 1025), (2048, 2048), (2049, 4096), (8192, 8193), (16384, 3000), (3000, 16384)]


@pytest.fixture(scope="module")
def es_graphs(hip, ctx):
    """Two mesh graphs (17000 and 3000 vertices) with 16 random vectors finalised (min-max normalised to [-0.5, 0.5]): the
    reference input of every test below is what is then resident, read back with `final_rows` / `point_rows`."""
    from pyfocusr_amd.meshgen import blob_mesh

    out = []
    for n, seed in ((17000, 1), (3000, 0)):
        m = blob_mesh(n, seed=seed)
        g = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
        rng = np.random.default_rng(90 + seed)
        g.ws_ensure(16)
        for slot in range(16):
            g.upload(slot, rng.standard_normal(n))
        g.finalize_vectors(0, 16, minmax=True)
        g.all_rows = g.final_rows(np.arange(n))
        out.append(g)
    yield out
    for g in out:
        g.close()


def _es_maps(k, rng):
    """Column maps that permute, repeat a column (k >= 3) and flip signs."""
    col_t = rng.permutation(16)[:k].astype(np.int32)
    col_s = rng.permutation(16)[:k].astype(np.int32)
    if k >= 3:
        col_s[2] = col_s[0]
    sign_t = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    sign_s = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    sign_t[0], sign_s[-1] = -1.0, -1.0
    return col_t, sign_t, col_s, sign_s


def _es_rows(g, m, cols, rng):
    """m rows drawn with repeats (exact ties in the sort), the argmin and argmax rows of the columns used among them (where
    the log meets 0 + eps, on the plain or on the flipped side); a tiny sample is drawn without repeats so that it has an
    extent on every axis."""
    if m < 8:
        return rng.choice(g.n, m, replace=False).astype(np.int64)
    rows = rng.integers(0, g.n, m).astype(np.int64)
    ext = np.unique(np.concatenate([np.argmin(g.all_rows[:, cols], axis=0), np.argmax(g.all_rows[:, cols], axis=0)]))[: m // 4]
    rows[rng.choice(m, len(ext), replace=False)] = ext
    return rows


def _es_reference(gt, gs, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s):
    T = gt.final_rows(rows_t)[:, col_t] * sign_t
    S = gs.final_rows(rows_s)[:, col_s] * sign_s
    idx = orc.knn1_bruteforce(er.minmax_points(gs.point_rows(rows_s)), er.minmax_points(gt.point_rows(rows_t)))[0]
    val, bound = np.empty((4, k, k)), np.empty((4, k, k))
    for i in range(k):
        for j in range(k):
            for f in (0, 1):
                w = er.w1_fsum(T[:, i], S[:, j], flip=bool(f))
                val[f, i, j], bound[f, i, j] = w["value"], er.w1_bound(w)
                val[2 + f, i, j], bound[2 + f, i, j] = er.spatial_fsum(T[:, i], S[idx, j], flip=bool(f))
    return val, bound, idx


def check_es(ctx, gt, gs, mt, ms, k, rng, label):
    col_t, sign_t, col_s, sign_s = _es_maps(k, rng)
    rows_t, rows_s = _es_rows(gt, mt, col_t, rng), _es_rows(gs, ms, col_s, rng)
    out, idx = ctx.eigsort_costs(gt, gs, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s)
    again, idx2 = ctx.eigsort_costs(gt, gs, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s)
    val, bound, widx = _es_reference(gt, gs, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s)
    ratio = np.abs(out - val) / bound
    print("eigsort_costs %s (mt, ms, k) = (%d, %d, %d): max |error| / bound: c_hist %.3f, c_hist_f %.3f, c_spatial %.3f, c_spatial_f %.3f; "
          "max relative error %.2e" % (label, mt, ms, k, ratio[0].max(), ratio[1].max(), ratio[2].max(), ratio[3].max(),
                                       float(np.max(np.abs(out - val) / np.abs(val)))))
    assert np.array_equal(idx, widx)
    assert same_bits(out, again) and np.array_equal(idx, idx2)
    assert np.all(np.isfinite(out)) and np.all(val > 0)
    for m, name in enumerate(("c_hist", "c_hist_f", "c_spatial", "c_spatial_f")):
        assert np.all(np.abs(out[m] - val[m]) <= bound[m]), (name, mt, ms, k, float(ratio[m].max()))
    return out


@gpu
@pytest.mark.parametrize("mt,ms", ES_COUNTS)
def test_eigsort_costs_against_the_definition(ctx, es_graphs, mt, ms):
    """The four matrices within the bounds of tests/_eigsort_ref.py (`w1_bound`, `spatial_fsum`: derived from the sums, the
    device log's stated 1 ulp included), the 1-NN indices exactly, two calls the same bits.  ms > 3000 repeats rows of the
    3000-vertex source graph."""
    gt, gs = es_graphs
    rng = np.random.default_rng(mt * 31 + ms)
    for k in (1, 3) + ((16,) if (mt, ms) == (255, 257) else ()):
        check_es(ctx, gt, gs, mt, ms, k, rng, "plain")


@gpu
def test_eigsort_costs_refusals(hip, ctx, es_graphs):
    """PF_E_ARG / PF_E_STATE before anything is launched; the context serves the next call."""
    gt, gs = es_graphs
    rng = np.random.default_rng(95)
    col, sign = np.arange(16, dtype=np.int32), np.ones(16)
    rows = rng.integers(0, 3000, 100)

    def refused(code, *args):
        with pytest.raises(hip.PfError) as e:
            ctx.eigsort_costs(*args)
        assert e.value.code == code, e.value

    refused(PF_E_ARG, gt, gs, rng.integers(0, 3000, 16385), rows, 2, col, sign, col, sign)
    refused(PF_E_ARG, gt, gs, rows, rng.integers(0, 3000, 16385), 2, col, sign, col, sign)
    refused(PF_E_ARG, gt, gs, rows, rows, 17, np.arange(17, dtype=np.int32) % 16, np.ones(17), np.arange(17, dtype=np.int32) % 16, np.ones(17))
    refused(PF_E_ARG, gt, gs, rows, rows, 0, col, sign, col, sign)
    bad = rows.copy()
    bad[50] = gt.n
    refused(PF_E_ARG, gt, gs, bad, rows, 2, col, sign, col, sign)
    bad[50] = -1
    refused(PF_E_ARG, gt, gs, rows, bad, 2, col, sign, col, sign)
    bad[50] = gs.n  # in range for the target (17000 rows), not for the source (3000)
    refused(PF_E_ARG, gt, gs, rows, bad, 2, col, sign, col, sign)
    bad_col = col.copy()
    bad_col[1] = 16
    refused(PF_E_ARG, gt, gs, rows, rows, 2, bad_col, sign, col, sign)
    bad_col[1] = -1
    refused(PF_E_ARG, gt, gs, rows, rows, 2, col, sign, bad_col, sign)
    # a graph from a matrix has no points; a graph without a finalised block has nothing to read
    M = sparse.random(500, 500, density=0.01, random_state=3, format="csr")
    M = (M + M.T + sparse.eye(500)).tocsr()
    M.sort_indices()
    gm = hip.DeviceLaplacian(matrix=(M.indptr, M.indices, M.data), ctx=ctx)
    m = __import__("pyfocusr_amd.meshgen", fromlist=["blob_mesh"]).blob_mesh(400, seed=9)
    fresh = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    try:
        gm.ws_ensure(16)
        for slot in range(16):
            gm.upload(slot, rng.standard_normal(500))
        gm.finalize_vectors(0, 16, minmax=True)
        small = rng.integers(0, 400, 100)
        refused(PF_E_STATE, gm, gs, small, rows, 2, col, sign, col, sign)
        refused(PF_E_STATE, gt, gm, rows, small, 2, col, sign, col, sign)
        refused(PF_E_STATE, fresh, gs, small, rows, 2, col, sign, col, sign)
        refused(PF_E_STATE, gt, fresh, rows, small, 2, col, sign, col, sign)
    finally:
        gm.close()
        fresh.close()
    check_es(ctx, gt, gs, 255, 257, 3, rng, "after the refusals")


@gpu
def test_eigsort_costs_degenerate_extent(hip, ctx, es_graphs):
    """A sample without extent along an axis (a planar mesh, a sample of one row) normalises to NaN there and its points have
    no nearest neighbour: one ValueError that names the extent, from the device path and from the host path alike, and the
    context serves the next call."""
    from pyfocusr_amd import eigsort
    from pyfocusr_amd.meshgen import blob_mesh

    gt, gs = es_graphs
    rng = np.random.default_rng(96)
    col, sign = np.arange(16, dtype=np.int32), np.ones(16)
    m = blob_mesh(2000, seed=11)
    flat_pts = m.points.copy()
    flat_pts[:, 2] = 1.25
    flat = hip.DeviceLaplacian(flat_pts, m.faces, ctx=ctx)
    try:
        flat.ws_ensure(16)
        for slot in range(16):
            flat.upload(slot, rng.standard_normal(2000))
        flat.finalize_vectors(0, 16, minmax=True)
        rows_f, rows_s = rng.integers(0, 2000, 300), rng.integers(0, 3000, 257)
        with pytest.raises(ValueError, match=r"degenerate extent.*target sample \(300 points\) has no extent along z"):
            ctx.eigsort_costs(flat, gs, rows_f, rows_s, 3, col, sign, col, sign)
        check_es(ctx, gt, gs, 255, 257, 1, rng, "after a planar target")
        with pytest.raises(ValueError, match=r"degenerate extent.*source sample \(300 points\) has no extent along z"):
            ctx.eigsort_costs(gs, flat, rows_s, rows_f, 3, col, sign, col, sign)
        with pytest.raises(ValueError, match=r"degenerate extent.*target sample \(1 points\) has no extent along x, y, z"):
            ctx.eigsort_costs(gt, gs, np.array([5]), rows_s, 2, col, sign, col, sign)
        with pytest.raises(ValueError, match=r"degenerate extent.*source sample \(1 points\) has no extent along x, y, z"):
            ctx.eigsort_costs(gt, gs, rows_s, np.array([7]), 2, col, sign, col, sign)
        check_es(ctx, gt, gs, 255, 257, 3, rng, "after the degenerate samples")

        # the host path of the class (samples in hand)
        class G(object):  # (the sample properties name the graph's samplers before they look at what is in hand)
            verbose = False
            get_rand_normalized_points = get_rand_eig_vecs = None

        sorter = eigsort(G(), G(), 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            sorter.rand_target_points = orc.rand_normalized_points(flat_pts, rows_f)
        sorter.rand_source_points = orc.rand_normalized_points(m.points, rows_f)
        sorter.rand_target_eig_vecs = rng.uniform(-0.5, 0.5, (300, 2))
        sorter.rand_source_eig_vecs = rng.uniform(-0.5, 0.5, (300, 2))
        with pytest.raises(ValueError, match=r"degenerate extent.*target sample \(300 points\) has no extent along z"):
            sorter.calc_c_spatial()
        sorter.rand_target_points = orc.rand_normalized_points(m.points, rows_s % 2000)
        sorter.rand_target_eig_vecs = rng.uniform(-0.5, 0.5, (257, 2))
        sorter.calc_c_spatial()  # the same object with a proper sample: the host path runs through
        assert np.all(np.isfinite(sorter.c_spatial)) and np.all(sorter.c_spatial > 0)
    finally:
        flat.close()
