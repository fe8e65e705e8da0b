"""Optimal one-to-one assignment on Euclidean costs (`euclidean_assignment`, `pf_assign`): the "hungarian"
correspondences of focusr.py:340-349 without an n x n matrix."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

from pyfocusr_amd import euclidean_assignment


def _lsa(A, B):
    return linear_sum_assignment(cdist(A, B))


def _cost(A, B, rows, cols):
    return float(np.sqrt(((A[rows] - B[cols]) ** 2).sum(1)).sum())


def _planted(n, d, seed):
    """A on a jittered lattice (spacing ~1 per axis), B = A[perm] + noise two orders of magnitude below the spacing."""
    rng = np.random.default_rng(seed)
    side = max(1, int(np.ceil(n ** (1.0 / d))))
    cells = rng.choice(side ** d, size=n, replace=False)
    A = np.stack(np.unravel_index(cells, (side,) * d), axis=1).astype(np.float64) + rng.uniform(-0.2, 0.2, (n, d))
    perm = rng.permutation(n)
    B = np.empty_like(A)
    B[perm] = A + rng.normal(scale=0.01, size=(n, d))  # row i of A belongs to row perm[i] of B
    return A, B, perm


def _check_certificate(A, B, col, u, v, gap, rows=None, chunk=1024):
    """Dual feasibility u_i + v_j <= C_ij (+1e-12 max C) over all columns for `rows`, and tightness of the assigned
    pairs: their slacks sum to at most gap (plus rounding)."""
    rows = np.arange(A.shape[0]) if rows is None else rows
    c_assigned = np.sqrt(((A - B[col]) ** 2).sum(1))
    max_c = 0.0
    worst = -np.inf
    for k in range(0, len(rows), chunk):
        r = rows[k:k + chunk]
        C = cdist(A[r], B)
        max_c = max(max_c, C.max())
        worst = max(worst, float((u[r, None] + v[None, :] - C).max()))
    assert worst <= 1e-12 * max(max_c, c_assigned.max())
    slack = c_assigned - u - v[col]
    assert slack.min() >= -1e-12 * c_assigned.max()
    assert slack.sum() <= gap + 1e-12 * c_assigned.sum() + 1e-14 * len(col) * c_assigned.max()


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("shape", [(300, 300), (200, 300), (300, 200)])
def test_host_switch_is_scipy(shape, monkeypatch):
    monkeypatch.setenv("PF_ASSIGN", "host")
    rng = np.random.default_rng(1)
    A, B = rng.normal(size=(shape[0], 3)), rng.normal(size=(shape[1], 3))
    r, c = euclidean_assignment(A, B)
    rs, cs = _lsa(A, B)
    assert np.array_equal(r, rs) and np.array_equal(c, cs)


def test_host_path_rejects_non_finite(monkeypatch):
    monkeypatch.setenv("PF_ASSIGN", "host")
    A = np.zeros((4, 2))
    A[2, 1] = np.nan
    with pytest.raises(ValueError):
        euclidean_assignment(A, np.ones((4, 2)))


# ------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000, 4097])
def test_planted_permutation(ctx, n, d):
    A, B, perm = _planted(n, d, seed=n * 31 + d)
    r, c = euclidean_assignment(A, B, ctx=ctx)
    assert np.array_equal(r, np.arange(n))
    assert np.array_equal(c, perm)
    assert np.array_equal(c, _lsa(A, B)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 5])
@pytest.mark.parametrize("shape", [(2000, 2000), (1500, 2000), (2000, 1500)])
def test_random_clouds_match_scipy(ctx, shape, d):
    rng = np.random.default_rng(shape[0] + 7 * shape[1] + d)
    A, B = rng.uniform(size=(shape[0], d)), rng.uniform(size=(shape[1], d))
    r, c, u, v, stats = euclidean_assignment(A, B, return_duals=True, ctx=ctx)
    rs, cs = _lsa(A, B)
    assert np.array_equal(r, rs) and np.array_equal(c, cs)
    ref = _cost(A, B, rs, cs)
    assert abs(stats.total_cost - ref) <= 1e-12 * ref
    assert stats.gap_bound <= 1e-10 * stats.total_cost


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pair_5k", "pair_15k"])
def test_fixture_pairs(ctx, golden, name):
    A, B = golden(name)["coords_s_w"], golden(name)["coords_t_w"]
    want = golden("assign_pairs")
    col, stats = ctx.assign(A, B)
    assert np.array_equal(col, want[name + "_col_ind"])
    assert stats.gap_bound <= 1e-10 * stats.total_cost
    assert abs(stats.total_cost - float(want[name + "_total_cost"])) <= 1e-12 * stats.total_cost
    assert stats.dense_passes >= 1 and stats.phases >= 1


@pytest.mark.gpu
def test_certificate_on_host_20k(ctx):
    rng = np.random.default_rng(20)
    n = 20000
    A = rng.normal(size=(n, 4))
    B = A[rng.permutation(n)] + rng.normal(scale=0.05, size=(n, 4))
    col, stats, u, v = ctx.assign(A, B, return_duals=True)
    assert np.array_equal(np.sort(col), np.arange(n))
    assert stats.gap_bound <= 1e-10 * stats.total_cost
    assert np.all(v <= 0.0)
    _check_certificate(A, B, col, u, v, stats.gap_bound)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["duplicates", "lattice"])
def test_ties_are_optimal_and_deterministic(ctx, case):
    rng = np.random.default_rng(5)
    if case == "duplicates":
        base = rng.uniform(size=(400, 3))
        A = np.concatenate([base, base[:200], base[:100]])  # 700 rows, many exact copies
        B = rng.uniform(size=(700, 3))
    else:
        g = np.stack(np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij"), -1).reshape(-1, 2)
        A, B = g, g + np.array([0.5, 0.0])  # every row ties between two columns
    r1, c1, u, v, stats = euclidean_assignment(A, B, return_duals=True, ctx=ctx)
    r2, c2 = euclidean_assignment(A, B, ctx=ctx)
    assert np.array_equal(r1, r2) and np.array_equal(c1, c2)
    assert np.array_equal(np.sort(c1), np.arange(B.shape[0]))
    rs, cs = _lsa(A, B)
    assert abs(_cost(A, B, r1, c1) - _cost(A, B, rs, cs)) <= stats.gap_bound + 1e-12 * _cost(A, B, rs, cs)


@pytest.mark.gpu
def test_scale_250k(ctx):
    """250k x 250k in d = 5: a synthetic embedding (a smooth 5-D image of a 3-D cloud, the target its shuffled copy
    displaced by a quarter of the point spacing).  Certificate on the host for 2000 sampled rows and every assigned
    pair; device memory O(n (d + K)) from the call's own allocation count."""
    import time

    rng = np.random.default_rng(250)
    n, d = 250000, 5
    x = rng.uniform(-1, 1, size=(n, 3))
    A = np.stack([x[:, 0], x[:, 1], x[:, 2], 0.5 * x[:, 0] * x[:, 1], 0.5 * np.sin(2 * x[:, 2])], axis=1)
    spacing = n ** (-1.0 / 3.0)
    B = A[rng.permutation(n)] + rng.normal(scale=0.25 * spacing, size=(n, d))
    t0 = time.perf_counter()
    col, stats, u, v = ctx.assign(A, B, return_duals=True)
    elapsed = time.perf_counter() - t0
    assert elapsed < 300.0
    assert np.array_equal(np.sort(col), np.arange(n))
    assert stats.gap_bound <= 1e-10 * stats.total_cost
    assert stats.device_bytes <= 8 * n * (2 * d + 3 * stats.k + 16)
    sample = np.sort(rng.choice(n, size=2000, replace=False))
    _check_certificate(A, B, col, u, v, stats.gap_bound, rows=sample)
    print("250k assignment: %.2f s, stats %s" % (elapsed, stats.as_dict()))


@pytest.mark.gpu
def test_focusr_hungarian_matches_host(ctx, monkeypatch):
    from pyfocusr_amd import Focusr
    from pyfocusr_amd.meshgen import blob_mesh

    a, b = blob_mesh(3000, seed=3), blob_mesh(3000, seed=4)

    def run():
        reg = Focusr(a, b, icp_register_first=False, n_spectral_features=3, n_extra_spectral=0, list_features_to_calc=[],
                     initial_correspondence_type="hungarian", final_correspondence_type="hungarian", ctx=ctx,
                     registration=lambda src, tgt, kind: tgt)
        reg.align_maps()
        return reg.corresponding_target_idx_for_each_source_pt.copy()

    dev = run()
    monkeypatch.setenv("PF_ASSIGN", "host")
    host = run()
    assert np.array_equal(dev, host)


@pytest.mark.gpu
def test_errors_and_wide_coordinates(ctx):
    A = np.random.default_rng(0).normal(size=(50, 3))
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[7, 1] = bad
        with pytest.raises(ValueError):
            euclidean_assignment(A, B, ctx=ctx)
        with pytest.raises(ValueError):
            ctx.assign(B, A)
    # d = 17 goes to scipy
    rng = np.random.default_rng(17)
    A, B = rng.normal(size=(120, 17)), rng.normal(size=(120, 17))
    assert np.array_equal(euclidean_assignment(A, B, ctx=ctx)[1], _lsa(A, B)[1])


@pytest.mark.gpu
def test_focusr_wide_spectral_coordinates_use_scipy(ctx):
    """d = 17 through Focusr.get_hungarian_correspondence: scipy's answer."""
    from pyfocusr_amd import Focusr

    rng = np.random.default_rng(3)
    src, tgt = rng.normal(size=(200, 17)), rng.normal(size=(200, 17))
    reg = Focusr.__new__(Focusr)
    reg._ctx = ctx
    reg.get_hungarian_correspondence(tgt, src)
    assert np.array_equal(reg.corresponding_target_idx_for_each_source_pt, _lsa(src, tgt)[1])
