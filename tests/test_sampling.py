"""Farthest-point sampling (`pyfocusr_amd.sampling`, `pf_fps.hip`) against tests/_fps_ref.py.

CPU: the numpy reference on a hand-made case (ties, owners, distances) and on equal points.  GPU: samples, owners and
squared distances bit for bit at every depth the kernel is instantiated for and at sizes of one block plus one point and
of many blocks with a ragged last one; exact ties and duplicates; m beyond the distinct points; the refusals.
"""
import functools

import numpy as np
import pytest

import _fps_ref as pr

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------ CPU
def test_reference_hand_made_case():
    P = np.array([[0.0], [10.0], [4.0], [10.0], [5.0]])
    sel, owner, dmin = pr.fps(P, 3, start=0)
    # round 0 from index 0: dmin = [0, 100, 16, 100, 25], the tie of 1 and 3 goes to 1; round 1: dmin = [0, 0, 16, 0, 25]
    # gives index 4, not 2 (25 > 16); round 2: dmin = [0, 0, 1, 0, 0]
    assert sel.tolist() == [0, 1, 4]
    assert owner.tolist() == [0, 1, 2, 1, 2] and owner.dtype == np.int32
    assert dmin.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    sel2, owner2, dmin2 = pr.fps(P, 2, start=0)
    assert sel2.tolist() == [0, 1] and owner2.tolist() == [0, 1, 0, 1, 0] and dmin2.tolist() == [0.0, 0.0, 16.0, 0.0, 25.0]


def test_reference_start_at_the_point_farthest_from_the_centroid():
    P = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 4.0], [2.0, 2.0]])  # four corners tie: the lowest index
    sel, owner, dmin = pr.fps(P, 2, start=-1)
    assert sel.tolist() == [0, 3] and owner.tolist() == [0, 0, 0, 1, 0] and dmin.tolist() == [0.0, 16.0, 16.0, 0.0, 8.0]


def test_reference_equal_points_repeat_index_zero():
    sel, owner, dmin = pr.fps(np.full((6, 3), 2.5), 4, start=-1)
    assert sel.tolist() == [0, 0, 0, 0] and owner.tolist() == [0] * 6 and np.all(dmin == 0.0)
    assert pr.fps(np.full((6, 3), 2.5), 3, start=4)[0].tolist() == [4, 0, 0]


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@functools.lru_cache(maxsize=None)
def cloud(n, d):
    return np.random.default_rng(1000 * d + n).standard_normal((n, d))


def check(ctx, P, m, start):
    from pyfocusr_amd import farthest_point_sampling

    sel, owner, d2 = farthest_point_sampling(P, m, start=None if start < 0 else start, return_owner=True, return_d2=True, ctx=ctx)
    rsel, rowner, rd2 = pr.fps(P, m, start=start)
    assert sel.dtype == np.int64 and owner.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(sel, rsel)
    assert np.array_equal(owner, rowner)
    assert np.array_equal(d2, rd2)  # the same bits
    return sel, owner, d2


def assert_clear_first_sample(P):
    """The farthest point from the centroid leads the runner-up by far more than any summation order of the centroid
    could move either: the device's choice cannot depend on that order."""
    v = np.sort(pr.centroid_distances(P))
    assert v[-1] - v[-2] > 1e-9 * v[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 3, 5, 16])
def test_fps_is_bit_identical_to_the_reference(ctx, d):
    P = cloud(2500, d)
    assert_clear_first_sample(P)
    check(ctx, P, 300, -1)
    check(ctx, P, 300, 1234)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(257, 100), (70001, 100), (257, 1), (257, 257)])
def test_fps_block_boundaries_and_extreme_m(ctx, n, m):
    """257: one block plus one point; 70001: many blocks, the last one ragged; m = 1 and m = n."""
    P = cloud(n, 3)
    assert_clear_first_sample(P)
    check(ctx, P, m, -1)
    check(ctx, P, m, n - 1)


@pytest.mark.gpu
def test_fps_exact_ties_on_a_lattice_give_the_lowest_index(ctx):
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), np.arange(3.0), indexing="ij"), axis=-1).reshape(-1, 3)
    sel, _, _ = check(ctx, g, 200, -1)  # integer sums: the centroid is exact in any order, the eight corners tie
    assert sel[0] == 0
    check(ctx, g, 200, 611)


@pytest.mark.gpu
def test_fps_duplicate_rows(ctx):
    P = cloud(2500, 3).copy()
    P[400] = P[10]
    P[2000] = P[10]
    sel, owner, d2 = check(ctx, P, 300, -1)
    assert owner[10] == owner[400] == owner[2000] and d2[10] == d2[400] == d2[2000]
    assert not ({400, 2000} & set(sel.tolist()))  # a tie with row 10 goes to row 10
    check(ctx, P, 300, 2000)


@pytest.mark.gpu
def test_fps_more_samples_than_distinct_points_repeats_index_zero(ctx):
    rng = np.random.default_rng(5)
    P = rng.standard_normal((5, 3))[rng.integers(0, 5, 50)]
    assert len(np.unique(P, axis=0)) == 5
    sel, _, d2 = check(ctx, P, 20, -1)
    assert len(set(sel[:5].tolist())) == 5 and sel[5:].tolist() == [0] * 15 and np.all(d2 == 0.0)


@pytest.mark.gpu
def test_fps_two_calls_give_the_same_bits(ctx):
    from pyfocusr_amd import farthest_point_sampling

    P = cloud(70001, 3)
    a = farthest_point_sampling(P, 64, return_owner=True, return_d2=True, ctx=ctx)
    b = farthest_point_sampling(P, 64, return_owner=True, return_d2=True, ctx=ctx)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
def test_fps_accepts_a_mesh(ctx):
    from pyfocusr_amd import farthest_point_sampling
    from pyfocusr_amd.meshgen import blob_mesh

    mesh = blob_mesh(700, seed=0)
    sel = farthest_point_sampling(mesh, 50, ctx=ctx)
    assert np.array_equal(sel, pr.fps(np.asarray(mesh.points, dtype=np.float64), 50)[0])


@pytest.mark.gpu
def test_fps_refusals(hip, ctx):
    P = cloud(257, 3)
    for pts, m, start in [(np.zeros((10, 0)), 1, -1), (np.zeros((10, 17)), 1, -1), (P, 0, -1), (P, 258, -1), (P, 5, 257)]:
        with pytest.raises(hip.PfError):
            ctx.farthest_point_sampling(pts, m, start=start)
    bad = P.copy()
    bad[100, 1] = np.nan
    with pytest.raises(hip.PfError):
        ctx.farthest_point_sampling(bad, 5)
    ctx.farthest_point_sampling(P, 5)  # and the context works on


@pytest.mark.gpu
def test_voronoi_masses(ctx):
    from pyfocusr_amd import farthest_point_sampling, voronoi_masses

    P = cloud(2500, 3)
    mass = np.random.default_rng(3).uniform(0.5, 1.5, len(P))
    _, owner = farthest_point_sampling(P, 300, return_owner=True, ctx=ctx)
    w = voronoi_masses(owner, mass, 300)
    assert w.shape == (300,) and np.array_equal(w, np.bincount(owner, weights=mass, minlength=300))
    assert abs(w.sum() - mass.sum()) <= len(P) * EPS * mass.sum()
    assert np.all(w > 0.0)  # distinct points: every sample owns itself
