"""The Krylov vector kernels of csrc/pf_operator.hip, pf_orth.hip, pf_reduce.hip, pf_finalize.hip and pf_rows.hip called one by one, each against an exact reference (tests/_exact.py).

Graphs come from random sparse matrices (`pf_graph_from_matrix`): any row count, empty rows, rows wider than one
SELL-64 slice.  A matrix graph keeps the caller's row order up to a degree sort inside windows of at most 4096 aligned
rows, so a row planted in caller chunk c sits in solver chunk c: the vectors carry an O(1) entry in the first and last
row of every 4096-row chunk (and in rows 0 and n - 1) over a background of small values, and a lost, doubled or
misrouted chunk costs far more than the rounding bound.

Every kernel's reductions run over all n_pad rows, so every test also checks that the slots it wrote still have zero
padding rows: dots(s, s) against the exact |s|^2 of the n real rows (`assert_padding_zero`).
"""
import numpy as np
import pytest
from scipy import sparse

import _exact as ex
import _window_ref
from oracle import reference_port as orc

pytestmark = pytest.mark.gpu

SMALL_N = [1, 2, 63, 64, 65, 4095, 4096, 4097, 12289]
N_BELOW, N_ABOVE = 397312, 397313  # n_pad 397312 < 400000 <= 401408: the last narrow and the first wide orth shape


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def random_matrix(n, seed, symmetric=False):
    """CSR with a diagonal on most rows, 0-5 off-diagonal entries per row, every 37th row empty (isolated, no diagonal
    either) and every 1000th row (from row 7) with 70-100 entries: wider than one SELL-64 slice."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 6, n)
    wide = np.arange(7, n, 1000)
    deg[wide] = rng.integers(70, 101, len(wide))
    deg = np.minimum(deg, n - 1)
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, len(rows))
    vals = -rng.uniform(0.1, 1.0, len(rows))
    M = sparse.csr_matrix((vals, (rows, cols)), shape=(n, n))
    M.setdiag(0.0)
    if symmetric:
        M = (M + M.T) * 0.5
    empty = np.zeros(n, bool)
    empty[5::37] = True
    keep = sparse.diags((~empty).astype(float))
    M = (keep @ M @ keep).tocsr()
    M.eliminate_zeros()
    d = np.where(empty, 0.0, rng.uniform(1.0, 3.0, n))
    M = (M + sparse.diags(d)).tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def planted(rng, n, cols=None):
    """Background of ~1e-3, O(1) entries of random sign in rows 0 and n - 1 and the first and last row of every chunk."""
    shape = (n,) if cols is None else (n, cols)
    v = 1e-3 * rng.standard_normal(shape)
    idx = np.unique(np.concatenate([[0, n - 1], np.arange(0, n, 4096), np.minimum(np.arange(4095, n + 4095, 4096), n - 1)]))
    big = rng.uniform(1.0, 2.0, (len(idx),) + shape[1:]) * np.where(rng.random((len(idx),) + shape[1:]) < 0.5, -1.0, 1.0)
    v[idx] = big
    return v


@pytest.fixture(scope="module")
def graphs(hip, ctx):
    cache = {}

    def get(n, symmetric=False):
        key = (n, symmetric)
        if key not in cache:
            M = random_matrix(n, seed=n + 7 * symmetric, symmetric=symmetric)
            g = hip.DeviceLaplacian(matrix=(M.indptr, M.indices, M.data), ctx=ctx)
            g.M = M
            # does the resident filter kernel cover this graph?  Random columns: a 1024-row window of a graph with thousands
            # of rows reads more outside rows than its list holds, so only the graphs of a few dozen rows are covered and
            # every filter application on the others runs one step per launch - exactly where the restatement says so
            ref = _window_ref.analyse(M, rings=False)
            g.resident_covered = g.window_info()["state"] == 1
            assert g.resident_covered == ref.covered, (n, symmetric, int(ref.ghosts.max()), int(ref.candidates.max()))
            cache[key] = g
        return cache[key]

    yield get
    for g in cache.values():
        g.close()


def upload_cols(g, first, V):
    V = np.asarray(V).reshape(g.n, -1)
    for b in range(V.shape[1]):
        g.upload(first + b, V[:, b])


def assert_close_bound(got, want, bound, what):
    err = abs(float(got) - float(want))
    assert err <= bound, (what, got, want, err, bound)


def assert_padding_zero(g, *slots):
    """dots(s, s) over all n_pad rows equals |s|^2 of the n real rows within the bound: the padding rows are 0."""
    depth = ex.reduction_depth(g.n)
    for s in slots:
        x = g.download_slots(s, 1)[:, 0]
        assert_close_bound(g.dots(s, s, 1)[0], ex.exact_sumsq(x), ex.dot_bound(x, x, depth), ("padding", g.n, s))


# ------------------------------------------------------------------------------------------------------------- dots
@pytest.mark.parametrize("n", SMALL_N)
def test_dots_exact(graphs, n):
    """pf_dots (k_dot_partial + k_dot_finish): counts 0, 1, 7, 8, 63, 64, 65 against the exact dot products, from one
    chunk (n <= 4096, partly padding) to 4 chunks (12289 rows: a last chunk with one real row)."""
    g = graphs(n)
    rng = np.random.default_rng(n)
    g.ws_ensure(70)
    w = planted(rng, n)
    V = planted(rng, n, 65)
    g.upload(0, w)
    upload_cols(g, 1, V)
    depth = ex.reduction_depth(n)
    for count in (0, 1, 7, 8, 63, 64, 65):
        d = g.dots(0, 1, count)
        assert d.shape == (count,)
        for b in range(count):
            assert_close_bound(d[b], ex.exact_dot(V[:, b], w), ex.dot_bound(V[:, b], w, depth), (n, count, b))
    assert_padding_zero(g, 0, 1, 65)


# ------------------------------------------------------------------------------------------------------------- orth
def orth_reference(V, w):
    """Two classical Gram-Schmidt passes: exact dot products (h1, h2), float64 updates (their rounding, ~eps |w|, is far
    inside the tolerances).  -> h1 + h2, |w after one pass|, w after two passes."""
    h1 = np.array([ex.exact_dot(V[:, b], w) for b in range(V.shape[1])])
    w1 = w - V @ h1
    h2 = np.array([ex.exact_dot(V[:, b], w1) for b in range(V.shape[1])])
    w2 = w1 - V @ h2
    return h1 + h2, np.linalg.norm(w1), w2


def orth_inputs(rng, n, count):
    """An orthonormal basis (a planted one would share the O(1) rows of w: w' would cancel) and two vectors with planted
    rows: one that needs one pass (|w'| / |w| ~ 0.7) and one whose projection cancels 5 digits (the second pass is due;
    its rounding, count 2^-53 |w| / |w'| < 1e-9, stays inside the two-pass tolerance)."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, count)))
    noise = planted(rng, n)
    noise /= np.linalg.norm(noise)
    coef = rng.uniform(-1.0, 1.0, count)
    mild = Q @ coef + np.linalg.norm(coef) * noise
    c2 = 3.0 * coef + np.sign(coef)
    cancelling = Q @ c2 + 1e-5 * np.linalg.norm(c2) * noise
    return Q, {"mild": mild, "cancelling": cancelling}


def check_orth_result(g, slot, h, nrm, w, ref, normalize, passes2, label):
    """Against the exact reference with test_orth_one_pass_with_second_pass_on_demand's tolerances: h to 1e-12; the norm
    to 1e-13 after one pass (Pythagoras) and 1e-8 after two; w' to 1e-13 / 1e-8 of its norm."""
    href, nrm1, w2 = ref
    np.testing.assert_allclose(h, href, rtol=1e-12, atol=1e-12 * np.max(np.abs(href)), err_msg=label)
    want_nrm = np.linalg.norm(w2) if passes2 else nrm1
    np.testing.assert_allclose(nrm, want_nrm, rtol=1e-8 if passes2 else 1e-13, err_msg=label)
    got = g.download_slots(slot, 1)[:, 0]
    scale = 1.0 / want_nrm if normalize else 1.0
    tol = 1e-8 if passes2 else 1e-13
    np.testing.assert_allclose(got, w2 * scale, rtol=0, atol=tol * np.linalg.norm(w2 * scale), err_msg=label)
    assert_padding_zero(g, slot)


ORTH_CASES = [(n, c) for n in (65, 4097, 12289) for c in (1, 2, 3, 4, 5, 7, 63, 64) if c <= n // 2] + [
    (4097, 65), (12289, 65), (4097, 255), (4097, 256), (12289, 256)]


@pytest.mark.parametrize("n,count", ORTH_CASES)
def test_orth_exact(hip, graphs, n, count):
    """pf_orth_begin / pf_orth_end below 400k rows against two exact classical Gram-Schmidt passes: counts 1-4 (k_orth_local
    with orth_one_launch on, k_orth_dots<1> / k_orth_project<1> with it off), 5 (the first count past k_orth_local), counts
    that are not a multiple of 4, 255 (the largest fused count) and 256 (PF_ORTH_MAX: pf_dots_device + k_multi_axpy, two
    passes always); normalize on and off, the device's second pass (orth_device_passes), a split basis (orth_split: junk in
    the slots between the two ranges), a step that needs no second pass and one that does."""
    g = graphs(n)
    rng = np.random.default_rng(1000 * n + count)
    Q, ws = orth_inputs(rng, n, count)
    fallback = count >= 256
    s = count // 2
    F = count + 2  # split layout: Q[:, :s] at F.., junk at F+s.., Q[:, s:] at first2
    first2 = F + count + 2
    g.ws_ensure(first2 + count + 1)
    upload_cols(g, 1, Q)
    if not fallback:
        upload_cols(g, F, Q[:, :s])
        upload_cols(g, F + s, planted(rng, n, count - s))
        upload_cols(g, first2, Q[:, s:])
    refs = {label: orth_reference(Q, w) for label, w in ws.items()}
    try:
        for one_launch in (True, False):
            hip.orth_one_launch(one_launch)
            for device_passes in (False, True):
                g.orth_device_passes(device_passes)
                for split in ((False, True) if not fallback else (False,)):
                    for normalize in (True, False):
                        for label, w in ws.items():
                            what = (n, count, one_launch, device_passes, split, normalize, label)
                            g.upload(0, w)
                            if split:
                                g.orth_split(first2, s)
                                g.orth_begin(0, F, count, normalize)
                            else:
                                g.orth_begin(0, 1, count, normalize)
                            h, nrm = g.orth_end()
                            second = label == "cancelling" and not fallback
                            if fallback:
                                assert not g.orth_redone and not g.orth_twice, what
                            else:
                                assert (g.orth_redone, g.orth_twice) == (second and not device_passes, second and device_passes), what
                            check_orth_result(g, 0, h, nrm, w, refs[label], normalize, second or fallback, str(what))
    finally:
        hip.orth_one_launch(True)
        g.orth_device_passes(False)


@pytest.fixture(scope="module")
def big_pair(graphs):
    """The graphs at 397312 and 397313 rows with an orthonormal basis of 65 vectors in slots 1..65 of each."""
    out = {}
    for n in (N_BELOW, N_ABOVE):
        g = graphs(n)
        rng = np.random.default_rng(n)
        Q, ws = orth_inputs(rng, n, 65)
        g.ws_ensure(70)
        upload_cols(g, 1, Q)
        w = ws["mild"]
        h1 = np.array([ex.exact_dot(Q[:, b], w) for b in range(65)])  # (count c: the first c of these)
        out[n] = (g, Q, w, h1)
    return out


def pair_reference(Q, w, h1, count):
    V = Q[:, :count]
    w1 = w - V @ h1[:count]
    h2 = V.T @ w1  # (~eps |w|: its own rounding is far inside the tolerances)
    return h1[:count] + h2, np.linalg.norm(w1), w1 - V @ h2


def test_orth_large_single_shapes(hip, big_pair):
    """One graph at 397312 rows (n_pad < 400000: k_orth_dots<1> / k_orth_project<1>) and at 397313 rows (n_pad 401408:
    k_orth_dots<4> / k_orth_project<8>), counts 2, 6 and 65 (6, 65: not multiples of VB = 4), one launch on and off."""
    try:
        for one_launch in (True, False):
            hip.orth_one_launch(one_launch)
            for n, (g, Q, w, h1) in big_pair.items():
                for count in (2, 6, 65):
                    g.upload(0, w)
                    g.orth_begin(0, 1, count, True)
                    h, nrm = g.orth_end()
                    assert not g.orth_redone
                    check_orth_result(g, 0, h, nrm, w, pair_reference(Q, w, h1, count), True, False, str((n, count, one_launch)))
    finally:
        hip.orth_one_launch(True)


@pytest.mark.parametrize("order", ["below_first", "above_first"])
def test_orth_pair_across_the_shape_switch(hip, big_pair, order):
    """pf_orth_begin2 of a 397312-row and a 397313-row graph: the switch keys on the larger n_pad, so BOTH run
    k_orth_dots<4> / k_orth_project<8> (or k_orth_local when both counts are <= 4) and the smaller graph's blocks leave
    the shared grid early.  Unequal counts (2 and 4, 3 and 6, 6 and 65) in both orders; each graph against its own exact
    reference."""
    na, nb = (N_BELOW, N_ABOVE) if order == "below_first" else (N_ABOVE, N_BELOW)
    (ga, Qa, wa, h1a), (gb, Qb, wb, h1b) = big_pair[na], big_pair[nb]
    try:
        for one_launch in (True, False):
            hip.orth_one_launch(one_launch)
            for ca, cb in ((2, 4), (3, 6), (6, 65), (65, 6)):
                ga.upload(0, wa)
                gb.upload(0, wb)
                ga.orth_begin2((0, 1, ca, True), gb, (0, 1, cb, True))
                ha, nrma = ga.orth_end()
                hb, nrmb = gb.orth_end()
                assert not ga.orth_redone and not gb.orth_redone
                what = (na, nb, ca, cb, one_launch)
                check_orth_result(ga, 0, ha, nrma, wa, pair_reference(Qa, wa, h1a, ca), True, False, str(what + ("a",)))
                check_orth_result(gb, 0, hb, nrmb, wb, pair_reference(Qb, wb, h1b, cb), True, False, str(what + ("b",)))
    finally:
        hip.orth_one_launch(True)


# ------------------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("n", [65, 4097, 12289])
def test_gram_exact(graphs, n):
    """pf_gram (k_gram_partial, one block row per pair + k_dot_finish): 1x1, 3x5, 9x13 and 64x64, the two slot blocks
    disjoint and overlapping; G[i, j] = <slot first_a + i, slot first_b + j> (orientation checked on non-square and on
    disjoint square blocks)."""
    g = graphs(n)
    rng = np.random.default_rng(n + 1)
    V = planted(rng, n, 130)
    g.ws_ensure(130)
    upload_cols(g, 0, V)
    depth = ex.reduction_depth(n)
    for (fa, ca, fb, cb) in ((0, 1, 1, 1), (0, 3, 10, 5), (2, 3, 3, 5), (0, 9, 20, 13), (5, 9, 8, 13), (0, 64, 64, 64), (3, 64, 30, 64)):
        if n < 4097 and ca == 64:
            continue
        G = g.gram(fa, ca, fb, cb)
        assert G.shape == (ca, cb)
        A, B = V[:, fa:fa + ca], V[:, fb:fb + cb]
        bound = depth * ex.EPS * (np.abs(A).T @ np.abs(B)) * (1 + 1e-6)  # (|A|^T |B| in float64: 1e-6 covers its rounding)
        want = np.stack([ex.exact_rowdots(A.T, B[:, j]) for j in range(cb)], axis=1)
        bad = np.argwhere(np.abs(G - want) > bound)
        assert len(bad) == 0, (n, fa, ca, fb, cb, bad[:5], G[tuple(bad[0])] if len(bad) else None)
        if ca == cb and ca > 1 and fa + ca <= fb:
            assert not np.allclose(G, G.T)  # (disjoint blocks: a transposed result would fail above)
    assert_padding_zero(g, 0, 129)


# ------------------------------------------------------------------------------------------------------ resnorm(s)
@pytest.mark.parametrize("n", [65, 4097, 12289])
def test_resnorms_exact(graphs, n):
    """pf_resnorms (k_resnorms_partial in batches of PF_RESNORMS_MAX = 64 vectors: counts 1, 63, 64, 65, 130 take one,
    two and three batches) and pf_resnorm (the same kernel, one vector), a distinct lambda per vector so that a lambda taken from
    the wrong batch or slot fails.  Bound on the squared norm: (depth + 5) 2^-53 sum (|ax| + |lam x|)^2 (each residual
    carries two roundings)."""
    g = graphs(n)
    rng = np.random.default_rng(n + 2)
    AX, X = planted(rng, n, 130), planted(rng, n, 130)
    g.ws_ensure(262)
    upload_cols(g, 0, AX)
    upload_cols(g, 130, X)
    lams = 0.25 + 0.01 * np.arange(130)
    depth = ex.reduction_depth(n) + 5

    def check(got, b, what):
        want2 = ex.exact_resnorm2(AX[:, b], X[:, b], lams[b])
        m = np.abs(AX[:, b]) + abs(lams[b]) * np.abs(X[:, b])
        assert_close_bound(got * got, want2, depth * ex.EPS * float(m @ m) + 4 * ex.EPS * want2, what)

    for count in (1, 63, 64, 65, 130):
        r = g.resnorms(0, 130, lams[:count])
        assert r.shape == (count,)
        for b in range(count):
            check(r[b], b, (n, count, b))
    for b in (0, 63, 64, 129):
        check(g.resnorm(b, 130 + b, lams[b]), b, (n, "single", b))
    assert_padding_zero(g, 0, 259)


# -------------------------------------------------------------------------------- one statement of every sum
@pytest.mark.parametrize("n", [65, 4097, 12289, N_BELOW, N_ABOVE])
def test_kernels_that_share_a_sum_agree_bit_for_bit(request, hip, graphs, n):
    """The kernels that form the same sum (csrc/pf_sums.h: chunk, block and column sum) return the same bits, not close
    ones.  n = 65, 4097, 12289 (one chunk, two, four with one real row in the last), the mild vector of orth_inputs (planted
    rows) against a basis of 5:  dots(w, first, 5) == the row of gram(w, first, 5) (k_dot_partial, k_gram_partial) == the h
    of a one-pass Gram-Schmidt step of count 5 (k_orth_dots<1> + k_orth_project<1>);  at count 4 the h of the step in one
    launch (k_orth_local) == the h of the two launches == dots;  resnorm == the matching entry of resnorms.  At 397312 and
    397313 rows (big_pair: k_orth_dots<1> / k_orth_project<1> and k_orth_dots<4> / k_orth_project<8>): the h of a count-6
    step == dots(w, 1, 6)."""
    if n >= N_BELOW:
        g, _, w, _ = request.getfixturevalue("big_pair")[n]
        g.upload(0, w)
        d = g.dots(0, 1, 6)
        g.orth_begin(0, 1, 6, True)
        h, _ = g.orth_end()
        assert not g.orth_redone and not g.orth_twice
        assert np.array_equal(h, d), (n, h - d)
        return
    g = graphs(n)
    rng = np.random.default_rng(n + 9)
    Q, ws = orth_inputs(rng, n, 5)
    w = ws["mild"]
    g.ws_ensure(12)
    g.upload(0, w)
    upload_cols(g, 1, Q)
    d = g.dots(0, 1, 5)
    G = g.gram(0, 1, 1, 5)
    assert G.shape == (1, 5) and np.array_equal(G[0], d), (n, G[0] - d)
    try:
        g.orth_device_passes(False)
        for count, modes in ((5, (True,)), (4, (True, False))):
            for one_launch in modes:
                hip.orth_one_launch(one_launch)
                g.upload(0, w)
                g.orth_begin(0, 1, count, False)
                h, _ = g.orth_end()
                assert not g.orth_redone and not g.orth_twice, (n, count, one_launch)  # (one pass: h is that pass's)
                assert np.array_equal(h, d[:count]), (n, count, one_launch, h - d[:count])
    finally:
        hip.orth_one_launch(True)
    AX, X = planted(rng, n, 3), planted(rng, n, 3)
    upload_cols(g, 6, AX)
    upload_cols(g, 9, X)
    lams = np.array([0.25, -1.5, 3.0])
    r = g.resnorms(6, 9, lams)
    for b in range(3):
        assert g.resnorm(6 + b, 9 + b, lams[b]) == r[b], (n, b)


# ------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("n", [65, 4097])
def test_combine_exact(graphs, n):
    """pf_combine (k_combine, 8 output columns per launch): m = 1, 2, 17 source vectors, k = 1, 7, 8, 9, 17 output
    columns (one, one full, two and three launches), the destination range right behind and right in front of the
    sources; every element within (m + 1) 2^-53 sum |src_b Y[b, c]| of its exact value."""
    g = graphs(n)
    rng = np.random.default_rng(n + 3)
    g.ws_ensure(60)
    for m in (1, 2, 17):
        S = planted(rng, n, m)
        for k in (1, 7, 8, 9, 17):
            Y = rng.standard_normal((m, k))
            for src, dst in ((20, 20 + m), (20, 20 - k)):
                upload_cols(g, src, S)
                behind = dst + k != src  # the slot right behind the destination range, when it is not a source
                if behind:
                    g.upload(dst + k, np.full(n, 7.0))
                g.combine(src, m, Y, dst)
                got = g.download_slots(dst, k)
                for c in range(k):
                    want = ex.exact_rowdots(S, Y[:, c])
                    bound = (m + 1) * ex.EPS * (np.abs(S) @ np.abs(Y[:, c]))
                    assert np.all(np.abs(got[:, c] - want) <= bound), (n, m, k, src, dst, c)
                assert np.array_equal(g.download_slots(src, m), S)  # sources intact
                if behind:
                    assert np.all(g.download_slots(dst + k, 1) == 7.0)
                assert_padding_zero(g, dst, dst + k - 1)


# ------------------------------------------------------------------------------------------------- scale / axpy
@pytest.mark.parametrize("n", [1, 4097, 12289])
def test_scale_and_axpy(graphs, n):
    """pf_scale (k_scale over n_pad rows): alpha 0, -1 and 1e-300 give numpy's products bit for bit.  pf_axpy
    (k_multi_axpy with negated coefficients): counts 0, 1, 9, each element within (count + 1) 2^-53 (|w| + sum |c_b v_b|)
    of the exact w + sum c_b v_b."""
    g = graphs(n)
    rng = np.random.default_rng(n + 4)
    g.ws_ensure(12)
    x = planted(rng, n)
    for alpha in (0.0, -1.0, 1e-300):
        g.upload(0, x)
        g.scale(0, alpha)
        assert np.array_equal(g.download_slots(0, 1)[:, 0], x * alpha), alpha
        if alpha != 1e-300:  # (squares of 1e-300 underflow: no exact reference)
            assert_padding_zero(g, 0)
    V = planted(rng, n, 9)
    upload_cols(g, 2, V)
    for count in (0, 1, 9):
        coef = rng.standard_normal(count)
        g.upload(0, x)
        g.axpy(0, 2, count, coef)
        got = g.download_slots(0, 1)[:, 0]
        A = np.concatenate([x[:, None], V[:, :count]], axis=1)
        y = np.concatenate([[1.0], coef])
        want = ex.exact_rowdots(A, y)
        bound = (count + 1) * ex.EPS * (np.abs(A) @ np.abs(y))
        assert np.all(np.abs(got - want) <= bound), count
        assert_padding_zero(g, 0)


# ------------------------------------------------------------------------------------------------------- operator
def operator_cases(hip, graphs):
    """(label, graph, op, scipy operator): a random matrix graph (op RW: A itself), a symmetric one (op SYM: the same
    operator), and a blob mesh (RW: L = G (D - W); SYM: S = G^1/2 (D - W) G^1/2 from the downloaded W and deg)."""
    from pyfocusr_amd.meshgen import blob_mesh

    out = []
    for n, sym in ((4097, False), (12289, True)):
        g = graphs(n, sym)
        out.append(("matrix%d%s" % (n, "s" if sym else ""), g, hip.PF_OP_SYM if sym else hip.PF_OP_RW, g.M, 0.0))
    key = ("blob", 5000)
    if key not in _MESHES:
        m = blob_mesh(5000, seed=9)
        _MESHES[key] = (hip.DeviceLaplacian(m.points, m.faces, ctx=graphs(1).ctx), m)
    g, _ = _MESHES[key]
    d = g.download()
    n = g.n
    W = sparse.csr_matrix((d["w"], d["colidx"], d["rowptr"]), shape=(n, n))
    L = (sparse.diags(d["l_diag"]) + sparse.csr_matrix((d["l_offdiag"], d["colidx"], d["rowptr"]), shape=(n, n))).tocsr()
    s = np.sqrt(1.0 / (d["deg"] + 1e-8))
    S = (sparse.diags(s) @ (sparse.diags(d["deg"]) - W) @ sparse.diags(s)).tocsr()
    S.sort_indices()
    L.sort_indices()
    assert g.symmetric
    out.append(("blob_rw", g, hip.PF_OP_RW, L, 0.0))
    out.append(("blob_sym", g, hip.PF_OP_SYM, S, 8.0))  # (S's entries: the device rounds them its own way, a few ulp)
    return out


_MESHES = {}


@pytest.fixture(scope="module")
def operators(hip, graphs):
    yield operator_cases(hip, graphs)
    for g, _ in _MESHES.values():
        g.close()
    _MESHES.clear()


def exact_apply(A, x):
    return ex.exact_matvec(A.indptr, A.indices, A.data, x)


def op_depth(A, extra):
    return int(np.max(np.diff(A.indptr))) + 4 + extra


def test_spmv_multi_exact(operators):
    """pf_spmv_multi (k_sell_op_slots: one block row per slot) for 1, 3 and 17 slots against the exact products of every
    row; bound (row width + 4) 2^-53 (|A| |x|) (the SELL loop contracts to FMAs), both operators of the mesh graph."""
    for label, g, op, A, extra in operators:
        rng = np.random.default_rng(11)
        n = g.n
        g.ws_ensure(40)
        saved = g.op
        g.op = op
        try:
            for count in (1, 3, 17):
                X = planted(rng, n, count)
                upload_cols(g, 0, X)
                g.spmv_multi(0, 20, count)
                got = g.download_slots(20, count)
                for c in range(count):
                    want = exact_apply(A, X[:, c])
                    bound = op_depth(A, extra) * ex.EPS * (abs(A) @ np.abs(X[:, c]))
                    assert np.all(np.abs(got[:, c] - want) <= bound), (label, count, c)
                assert_padding_zero(g, 20, 20 + count - 1)
        finally:
            g.op = saved


def test_op_step_formula(operators):
    """pf_op_step (k_sell_op, pf_launch_op): out = alpha (shift x - A x) - beta prev, the formula of pyfocusr_hip.h, for
    every combination of alpha (1, -1, 0.37), shift (0, 1.3) and beta (0, 1, 0.6), with prev, without (prev = -1), and
    with out aliasing prev."""
    for label, g, op, A, extra in operators:
        rng = np.random.default_rng(12)
        n = g.n
        g.ws_ensure(8)
        x, prev = planted(rng, n), planted(rng, n)
        ax = exact_apply(A, x)
        absax = abs(A) @ np.abs(x)
        depth = op_depth(A, extra) + 4
        for alpha in (1.0, -1.0, 0.37):
            for shift in (0.0, 1.3):
                for beta in (0.0, 1.0, 0.6):
                    for mode in ("prev", "none", "alias"):
                        g.upload(0, x)
                        g.upload(1, prev)
                        g.upload(2, np.full(n, 5.0))
                        out = 1 if mode == "alias" else 2
                        g.op_step(0, None if mode == "none" else 1, out, alpha, shift, beta, op=op)
                        got = g.download_slots(out, 1)[:, 0]
                        p = 0.0 if mode == "none" else prev
                        want = alpha * (shift * x - ax) - beta * p
                        bound = depth * ex.EPS * (abs(alpha) * (abs(shift) * np.abs(x) + absax) + abs(beta) * np.abs(p)) + 2 * ex.EPS * np.abs(want)
                        assert np.all(np.abs(got - want) <= bound), (label, alpha, shift, beta, mode)
                        assert np.array_equal(g.download_slots(0, 1)[:, 0], x)
                        assert_padding_zero(g, out)


def test_cheb_steps_split_and_one_step_path(hip, operators):
    """pf_cheb_steps: a degree-p recurrence split as (k_first = 1, n1) + (k_first = n1 + 1, p - n1) gives the bits of one
    call, for n1 = 0, 1, 3 and p - 1; and the bits of pf_cheb with one step per launch (persist off: ChebRun forms
    every step with pf_launch_op and the same alpha = 1/(e rho) or 2/(e rho), shift = c, beta = 0 or 1/rho^2, so the same
    bits are required, not a bound).  Both against the numpy recurrence (test_spmv_and_cheb's tolerance), rho = 1 and
    1.3, and the returned (prev, cur) slots: cur holds y_p, prev y_(p - 1)."""
    hip.persist_enable(False)
    try:
        for label, g, op, A, extra in operators:
            rng = np.random.default_rng(13)
            n = g.n
            g.ws_ensure(12)
            x = planted(rng, n)
            # the interval [c - e, c + e]: the mesh operator's [0, 2]; a matrix's Gershgorin interval [0, 2R]
            R = float(np.max(abs(A) @ np.ones(n)))
            c, e = (1.002, 0.998) if label.startswith("blob") else (R, R)
            for p in (7, 40):
                for rho in (1.0, 1.3):
                    ys = [x, (c * x - A @ x) / (e * rho)]
                    for _ in range(p - 1):
                        ys.append((2.0 / (e * rho)) * (c * ys[-1] - A @ ys[-1]) - ys[-2] / rho**2)
                    g.upload(0, x)
                    g.upload(1, np.full(n, 9.0))
                    pv, cu = g.cheb_steps(1, 0, 1, p, c, e, rho, op=op)
                    whole = g.download_slots(cu, 1)[:, 0]
                    before = g.download_slots(pv, 1)[:, 0]
                    assert {pv, cu} == {0, 1}
                    scale = np.max(np.abs(ys[p]))
                    assert np.max(np.abs(whole - ys[p])) <= 1e-12 * scale, (label, p, rho)
                    assert np.max(np.abs(before - ys[p - 1])) <= 1e-12 * np.max(np.abs(ys[p - 1])), (label, p, rho)
                    assert_padding_zero(g, 0, 1)
                    for n1 in (0, 1, 3, p - 1):
                        g.upload(0, x)
                        a_, b_ = g.cheb_steps(1, 0, 1, n1, c, e, rho, op=op)
                        if n1 == 0:
                            assert (a_, b_) == (1, 0)
                        a_, b_ = g.cheb_steps(a_, b_, n1 + 1, p - n1, c, e, rho, op=op)
                        assert (a_, b_) == (pv, cu), (label, p, n1)
                        assert np.array_equal(g.download_slots(b_, 1)[:, 0], whole), (label, p, rho, n1)
                        assert np.array_equal(g.download_slots(a_, 1)[:, 0], before), (label, p, rho, n1)
                    g.upload(0, x)
                    saved = g.op
                    g.op = op
                    try:
                        g.cheb(0, 2, p, c, e, rho)
                    finally:
                        g.op = saved
                    assert np.array_equal(g.download_slots(2, 1)[:, 0], whole), (label, p, rho)
    finally:
        hip.persist_enable(True)


# ------------------------------------------------------------------------------------------------------------ rows
def row_sets(rng, n):
    return {"empty": np.zeros(0, np.int64), "single": np.array([n - 1], np.int64),
            "unsorted": rng.permutation(n)[: max(1, n // 3)].astype(np.int64), "all": rng.permutation(n).astype(np.int64)}


@pytest.mark.parametrize("n", [1, 65, 4097, 12289])
def test_rows_host_forms(graphs, n):
    """pf_rows_gather / _scatter / _fill (k_rows_to_new, k_rows_gather, k_rows_scatter, k_rows_fill): bit for bit what
    numpy indexing in mesh order gives, on row sets that are empty, one row, unsorted, and the whole graph permuted."""
    g = graphs(n)
    rng = np.random.default_rng(n + 5)
    g.ws_ensure(2)
    x = planted(rng, n)
    for label, idx in row_sets(rng, n).items():
        rows = g.rows_create(idx)
        g.upload(0, x)
        assert np.array_equal(g.rows_gather(0, rows), x[idx]), label
        vals = rng.standard_normal(len(idx))
        g.rows_scatter(0, rows, vals)
        want = x.copy()
        want[idx] = vals
        assert np.array_equal(g.download_slots(0, 1)[:, 0], want), label
        g.rows_fill(0, rows, -2.5)
        want[idx] = -2.5
        assert np.array_equal(g.download_slots(0, 1)[:, 0], want), label
        assert_padding_zero(g, 0)


@pytest.mark.parametrize("n", [65, 12289])
def test_rows_device_forms(graphs, n):
    """pf_rows_gather_dev / _scatter_dev / _gather2_dev / _scatter2_dev with torch device buffers: slot_b = -1 (only the
    first half written), a stride larger than the row count (the gap untouched), and pf_rows_set_sources offsets that
    permute and shift the receive buffer."""
    import torch

    g = graphs(n)
    rng = np.random.default_rng(n + 6)
    g.ws_ensure(4)
    xa, xb = planted(rng, n), planted(rng, n)
    dev = torch.device("cuda", g.ctx.device)
    for label, idx in row_sets(rng, n).items():
        m = len(idx)
        rows = g.rows_create(idx)
        g.upload(0, xa)
        g.upload(1, xb)
        buf = torch.full((m,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        g.rows_gather_dev(0, rows, buf.data_ptr())
        g.sync()
        assert np.array_equal(buf.cpu().numpy(), xa[idx]), label
        src = rng.standard_normal(m)
        buf = torch.from_numpy(src).to(dev)
        torch.cuda.synchronize()
        g.rows_scatter_dev(1, rows, buf.data_ptr())
        g.sync()
        want_b = xb.copy()
        want_b[idx] = src
        assert np.array_equal(g.download_slots(1, 1)[:, 0], want_b), label
        stride = m + 5
        for slot_b in (1, None):
            buf = torch.full((2 * stride,), -1.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            g.rows_gather2_dev(0, slot_b, rows, buf.data_ptr(), stride)
            g.sync()
            got = buf.cpu().numpy()
            assert np.array_equal(got[:m], xa[idx]) and np.all(got[m:stride] == -1.0), label
            if slot_b is None:
                assert np.all(got[stride:] == -1.0), label
            else:
                assert np.array_equal(got[stride:stride + m], want_b[idx]) and np.all(got[stride + m:] == -1.0), label
        if m == 0:
            continue
        off = rng.permutation(m).astype(np.int64) + 3  # rows' values sit permuted, 3 places in
        g.rows_set_sources(rows, off)
        recv = rng.standard_normal(2 * stride + 3)
        for slot_b in (1, None):
            g.upload(0, xa)
            g.upload(1, xb)
            buf = torch.from_numpy(recv).to(dev)
            torch.cuda.synchronize()
            g.rows_scatter2_dev(0, slot_b, rows, buf.data_ptr(), stride)
            g.sync()
            wa, wb = xa.copy(), xb.copy()
            wa[idx] = recv[off]
            if slot_b is not None:
                wb[idx] = recv[off + stride]
            assert np.array_equal(g.download_slots(0, 1)[:, 0], wa), label
            assert np.array_equal(g.download_slots(1, 1)[:, 0], wb), label
            assert_padding_zero(g, 0, 1)


# ---------------------------------------------------------------------------------------------------- start vector
@pytest.mark.parametrize("n", [1, 65, 4097, 12289])
def test_start_vector(graphs, n):
    """pf_start_vector (k_start_vector over n_pad rows): zero on isolated rows (no off-diagonal entry), finite, the same
    bits for the same seed and other bits for another, zero padding rows."""
    g = graphs(n)
    g.ws_ensure(3)
    g.upload(0, np.full(n, 3.0))
    g.start_vector(0, 12345)
    g.start_vector(1, 12345)
    g.start_vector(2, 54321)
    v = g.download_slots(0, 3)
    M = g.M
    isolated = np.diff(M.indptr) - (M.diagonal() != 0) == 0
    assert np.all(np.isfinite(v))
    assert np.all(v[isolated] == 0.0)
    assert np.array_equal(v[:, 0], v[:, 1])
    if np.any(~isolated):
        assert np.any(v[~isolated, 0] != 0.0) and not np.array_equal(v[:, 0], v[:, 2])
    assert_padding_zero(g, 0, 1, 2)


# ----------------------------------------------------------------------------------------------- finalize / rows
@pytest.mark.parametrize("n", [65, 4097, 12289])
def test_finalize_and_resident_rows(graphs, n):
    """pf_finalize_vectors (k_vec_stats_partial / _finish over 1, 2 and 4 chunks, k_vec_params, k_vec_apply) against
    orc.canonicalize and orc.minmax_normalize; an exact tie of the largest |entry| (-a at an earlier caller index, +a at
    a later one: the earlier wins, the column flips); a constant column (ptp = 0: min-max leaves it as it is, bit for
    bit).  Then pf_final_rows and pf_final_remap_begin: bit-exact gathers of the resident block."""
    g = graphs(n)
    rng = np.random.default_rng(n + 8)
    k = 4
    X = planted(rng, n, k)
    X[:, 1] = 0.01 * rng.standard_normal(n)
    if n > 1:
        X[n // 3, 1], X[n - 1, 1] = -5.0, 5.0  # the tie: the earlier index (negative) decides the sign
    X[:, 3] = 0.5  # constant
    g.ws_ensure(k)
    upload_cols(g, 0, X)
    exp = X / np.linalg.norm(X, axis=0)
    _, exp = orc.canonicalize(np.arange(float(k)), exp)
    raw = g.finalize_vectors(0, k, minmax=False).copy()
    np.testing.assert_allclose(raw[:, :3], exp[:, :3], rtol=1e-13, atol=1e-16)
    if n > 1:
        assert raw[n // 3, 1] > 0 and raw[n - 1, 1] < 0
    const = 0.5 * (1.0 / np.sqrt(0.25 * n))
    assert np.all(raw[:, 3] == const)
    rows = rng.integers(0, n, 50)
    assert np.array_equal(g.final_rows(rows), raw[rows])
    assert np.array_equal(g.final_rows(np.zeros(0, np.int64)), np.zeros((0, k)))
    nrm = g.finalize_vectors(0, k, minmax=True)
    got = nrm.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = orc.minmax_normalize(exp)
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=0, atol=1e-14)
    assert np.all(got[:, :3].min(axis=0) == -0.5) and np.all(got[:, :3].max(axis=0) == 0.5)
    assert np.all(got[:, 3] == const)  # ptp = 0: left as it is
    assert np.array_equal(g.final_rows(rows), got[rows])
    cols = np.array([2, 0, 3, 1], np.int32)
    signs = np.array([-1.0, 1.0, -1.0, 1.0])
    g.final_remap(cols, signs, nrm)
    g.finalize_wait()
    assert np.array_equal(nrm, got[:, cols] * signs)
    assert np.array_equal(g.final_rows(rows), got[rows])  # the resident block itself is unchanged


def test_landings_grow_recycle_and_come_from_the_pool(hip):
    """The pinned landings of a graph (HostLanding, pf_scratch.h) through their sizes, on a context of the test's own
    and a 600-vertex mesh (n_pad 4096, the least there is): orth with counts 3, 63, 64, 70, 3 on one graph (64 is the first count to outgrow
    the floor of 64 doubles: the stream is drained and the block recycled; 70 grows again; 3 keeps the large block),
    gram 8 x 8 and 9 x 8, finalize with 2, 64, 65, 2 columns (65 outgrows the finaliser's floor of 384 doubles).  Then the
    graph is freed and a second one on the same context takes its landings from the context's pools: counts 70 and 3
    again.  Every result against the exact references and tolerances of test_orth_exact (one pass), test_gram_exact and
    test_finalize_and_resident_rows."""
    from pyfocusr_amd.meshgen import blob_mesh

    n = 600
    m = blob_mesh(n, seed=5)
    rng = np.random.default_rng(n)
    Q, ws = orth_inputs(rng, n, 70)
    w = ws["mild"]
    h1 = np.array([ex.exact_dot(Q[:, b], w) for b in range(70)])
    depth = ex.reduction_depth(n)
    own = hip.Context()

    def graph():
        g = hip.DeviceLaplacian(m.points, m.faces, ctx=own)
        assert g.info.n_pad == 4096  # (one reduction chunk, mostly padding)
        g.op = hip.PF_OP_RW  # (finalize_vectors: the slots as they are, no G^1/2)
        g.ws_ensure(72)
        upload_cols(g, 1, Q)
        return g

    def orth(g, count, label):
        g.upload(0, w)
        g.orth_begin(0, 1, count, True)
        h, nrm = g.orth_end()
        assert not g.orth_redone and not g.orth_twice, label
        check_orth_result(g, 0, h, nrm, w, pair_reference(Q, w, h1, count), True, False, label)

    try:
        g = graph()
        try:
            for count in (3, 63, 64, 70, 3):
                orth(g, count, "first graph, count %d" % count)
            for (fa, ca, fb, cb) in ((1, 8, 9, 8), (1, 9, 10, 8)):
                G = g.gram(fa, ca, fb, cb)
                A, B = Q[:, fa - 1:fa - 1 + ca], Q[:, fb - 1:fb - 1 + cb]
                bound = depth * ex.EPS * (np.abs(A).T @ np.abs(B)) * (1 + 1e-6)
                want = np.stack([ex.exact_rowdots(A.T, B[:, j]) for j in range(cb)], axis=1)
                assert np.all(np.abs(G - want) <= bound), (ca, cb, np.max(np.abs(G - want) - bound))
            for k in (2, 64, 65, 2):
                _, exp = orc.canonicalize(np.arange(float(k)), Q[:, :k] / np.linalg.norm(Q[:, :k], axis=0))
                raw = g.finalize_vectors(1, k, minmax=False)
                np.testing.assert_allclose(raw, exp, rtol=1e-13, atol=1e-16, err_msg="finalize, %d columns" % k)
        finally:
            g.close()
        g = graph()
        try:
            for count in (70, 3):
                orth(g, count, "second graph, count %d" % count)
        finally:
            g.close()
    finally:
        own.close()


def test_point_rows(hip, ctx):
    """pf_point_rows (k_final_rows over the resident points): bit-exact mesh-order rows, empty, single, unsorted, all."""
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(3000, seed=2)
    g = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx)
    try:
        rng = np.random.default_rng(3)
        for label, idx in row_sets(rng, g.n).items():
            assert np.array_equal(g.point_rows(idx), np.asarray(m.points, dtype=np.float64)[idx].reshape(-1, 3)), label
    finally:
        g.close()
