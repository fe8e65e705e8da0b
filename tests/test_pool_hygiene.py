"""No device unit depends on what its pool memory held before (run with `-m gpu` on an MI355X).

Every device buffer of the library comes from the per-ctx caching allocator (`pf_malloc`): the `Scratch` blocks of a call,
the `DevBuf`s that grow and stay, the `keep` blocks a handle owns.  A block of that cache holds whatever its last user
left, and a `DevBuf` that an earlier, larger call grew keeps that call's data beyond the current problem's extent.  Each
case below is one entry-point family on the paths `profiles/pool_hygiene.md` lists for it, run four times:

* plain: `pf_pool_poison(0)`;
* 0xFF and 0x00: every block the pool hands out filled with all-ones (NaN, -1) or with zero bytes first - a reader that
  needs zeros breaks under the first, one that needs all-ones (the blocks some units set to 0xFF / 0x7F on purpose) under
  the second;
* after a larger neighbour: poison off, the same unit first run on the same ctx or handle on a problem at least twice as
  large in every size (and a larger k, K or d where it has one), so that the grown buffers hold foreign data.

All four give the same bytes (`tobytes()`: NaNs compare as bits) in every output array and every count the entry point
reports (timings are left out), and the plain result passes the criterion of the unit's own test file against that file's
reference - equal must not mean equally wrong.  Where a path has a statistic the case asserts that the path was taken."""
import contextlib
import os

import numpy as np
import pytest

import _knn_ref as kr
from oracle import reference_port as orc


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


# ------------------------------------------------------------------------------------------------ the four runs
CASES = {}


def case(make):
    """Registers `make(hip, ctx) -> (run, check)`: `run(neighbour)` returns every output of the case (arrays, counts; nested
    tuples, lists and dicts are walked), after the larger neighbour's work when `neighbour` is set; `check(out)` holds a
    plain run's outputs against the unit's reference and asserts the path statistics."""
    CASES[make.__name__] = make
    return make


def _flat(out, path="out"):
    """[(where, bytes)] of every leaf of `out`; python numbers as int64 / float64."""
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in _flat(out[k], "%s[%r]" % (path, k))]
    if isinstance(out, (tuple, list)):
        return [x for i, v in enumerate(out) for x in _flat(v, "%s[%d]" % (path, i))]
    if isinstance(out, (bool, int, np.integer)):
        return [(path, np.int64(out).tobytes())]
    if isinstance(out, (float, np.floating)):
        return [(path, np.float64(out).tobytes())]
    assert isinstance(out, np.ndarray), (path, type(out))
    return [(path, np.ascontiguousarray(out).tobytes())]


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _drop(d):
    """A dict of a call's outputs without its timings."""
    return {k: v for k, v in d.items() if k != "device_ms" and not k.startswith("ms_")}


def test_flattening_compares_bits():
    a = _flat({"x": np.array([np.nan, 1.0]), "n": 3, "t": (np.int32(4), 2.5)})
    assert [w for w, _ in a] == ["out['n']", "out['t'][0]", "out['t'][1]", "out['x']"]
    assert a == _flat({"x": np.array([np.nan, 1.0]), "n": 3, "t": (np.int32(4), 2.5)})  # a NaN equals itself as bits
    assert a != _flat({"x": np.array([np.nan, -1.0]), "n": 3, "t": (np.int32(4), 2.5)})
    assert _drop({"a": 1, "device_ms": 2.0, "ms_sort": 1.0}) == {"a": 1}


def _four_runs(hip, ctx, name):
    """(the test itself, parametrised over CASES, is at the end of the file)"""
    run, check = CASES[name](hip, ctx)
    lib = hip.load_library()
    runs = {}
    try:
        for mode, label in ((0, "plain"), (1, "0xFF"), (2, "0x00")):
            assert lib.pf_pool_poison(mode) == 0
            out = run(False)
            if mode == 0:
                check(out)
            runs[label] = _flat(out)
    finally:
        lib.pf_pool_poison(0)
    runs["after a larger neighbour"] = _flat(run(True))
    plain = runs.pop("plain")
    assert len(plain) > 0
    for label, got in runs.items():
        assert [w for w, _ in got] == [w for w, _ in plain], label
        differ = [w for (w, a), (_, b) in zip(plain, got) if a != b]
        assert not differ, "%s: %s differ from the plain run" % (label, ", ".join(differ))


# ------------------------------------------------------------------------------------------------ 1-NN and top-k searches
def _cloud(n, d, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=(n, d))


def _with_nan(qry, row):
    qry = qry.copy()
    qry[row, row % qry.shape[1]] = np.nan
    return qry


def _check_1nn(ref, qry, *results):
    """`test_gpu_parity.test_knn_bit_exact`'s criterion for every (idx, d2) of `results` on the clean queries (one brute
    force serves them all); a NaN query has no neighbour."""
    ok = ~np.isnan(qry).any(axis=1)
    bidx, bd2 = orc.knn1_bruteforce(ref, qry[ok])
    for idx, d2 in results:
        assert idx.dtype == np.int64
        assert np.array_equal(idx[ok], bidx) and np.array_equal(d2[ok], bd2)
        assert np.all(idx[~ok] == kr.NO_NEIGHBOUR) and np.all(np.isposinf(d2[~ok]))


@case
def knn1_one_launch(hip, ctx):
    """d <= 8 and both sets <= PF_KNN_SMALL: `k_knn_small`; 203 queries are no multiple of the group of 8 (d = 3) or 4 (d = 7)."""
    sets = [(_cloud(1000, d, 10 + d), _with_nan(_cloud(203, d, 20 + d), 77)) for d in (3, 7)]
    big = (_cloud(2100, 8, 1), _cloud(500, 8, 2))

    def run(neighbour):
        if neighbour:
            ctx.knn1(*big)
        return [ctx.knn1(ref, qry, return_d2=True) for ref, qry in sets]

    def check(out):
        for (ref, qry), (idx, d2) in zip(sets, out):
            _check_1nn(ref, qry, (idx, d2))

    return run, check


def _grid_case(ctx, bucket_max):
    """The grid search above PF_KNN_SMALL at d = 5, counted and plain; 3001 queries: a ragged last group of 4.  The
    counter of candidate-query pairs is compared with the other outputs where the points are sorted by the (stable)
    radix sort.  Behind the counting sort it is not a function of the input: the order inside a cell is the order in
    which the atomics of `k_bucket_scatter` land, the queries of a wave's group are neighbours in that order, and the
    group's rectangle - what the counter counts - follows its members (six plain runs of this case gave six counts
    within 0.3 % of each other; indices and distances do not depend on it).  There every run asserts its range instead."""
    ref, qry = _cloud(16500, 5, 31), _with_nan(_cloud(3001, 5, 32), 1234)
    big = (_cloud(40000, 6, 33), _cloud(7000, 6, 34))

    def search(r, q):
        if bucket_max is None:
            return ctx.knn1(r, q, return_d2=True)
        ctx.knn_mode(1)  # (as test_knn_radix_sorted_cells forces it)
        try:
            with _env("PF_KNN_BUCKET_MAX", str(bucket_max)):
                return ctx.knn1(r, q, return_d2=True)
        finally:
            ctx.knn_mode(0)

    def run(neighbour):
        if neighbour:
            ctx.knn_count(True)
            search(*big)
            ctx.knn_count(False)
            search(*big)
        ctx.knn_count(True)
        try:
            counted = search(ref, qry)
        finally:
            pairs = ctx.knn_count(False)
        assert 0 < pairs < len(ref) * len(qry)  # the counting grid kernel ran, and pruned
        return counted, pairs if bucket_max is not None else (), search(ref, qry)

    def check(out):
        counted, _, plain = out
        _check_1nn(ref, qry, counted, plain)

    return run, check


@case
def knn1_grid_counting_sort(hip, ctx):
    return _grid_case(ctx, None)


@case
def knn1_grid_radix_sort(hip, ctx):
    return _grid_case(ctx, 1)


@case
def knn1_box_hierarchy(hip, ctx):
    """d = 10 by the default mode: `pf_knn_tree.hip`; 4200 references are 66 leaves in two supers, the last leaf ragged."""
    ref, qry = _cloud(4200, 10, 41), _with_nan(_cloud(1003, 10, 42), 500)
    big = (_cloud(9000, 12, 43), _cloud(2100, 12, 44))

    def run(neighbour):
        if neighbour:
            ctx.knn1(*big)
        ctx.knn_tree_stats(True)
        try:
            counted = ctx.knn1(ref, qry, return_d2=True)
        finally:
            stats = ctx.knn_tree_stats(False)
        return counted, stats, ctx.knn1(ref, qry, return_d2=True)

    def check(out):
        counted, (leaves, supers), plain = out
        _check_1nn(ref, qry, counted, plain)
        assert leaves > 0 and supers > 0  # the hierarchy ran

    return run, check


@case
def knn1_modes_forced(hip, ctx):
    """`knn_mode` 1 (the grid on sets the one-launch kernel would take) and 2 (the hierarchy at d = 5)."""
    ref, qry = _cloud(3000, 5, 51), _with_nan(_cloud(777, 5, 52), 3)
    big = (_cloud(6100, 6, 53), _cloud(1600, 6, 54))

    def run(neighbour):
        out = []
        try:
            for mode in (1, 2):
                ctx.knn_mode(mode)
                if neighbour:
                    ctx.knn1(*big)
                ctx.knn_count(True)
                ctx.knn_tree_stats(True)
                try:
                    res = ctx.knn1(ref, qry, return_d2=True)
                finally:
                    stats = (ctx.knn_count(False),) + ctx.knn_tree_stats(False)
                if mode == 1:  # (behind the counting sort the pair counter is no function of the input: _grid_case)
                    assert 0 < stats[0] < len(ref) * len(qry)
                out.append((res, () if mode == 1 else stats[1:]))
        finally:
            ctx.knn_mode(0)
        return out

    def check(out):
        (grid, _), (tree, (leaves, supers)) = out
        _check_1nn(ref, qry, grid, tree)
        assert leaves > 0 and supers > 0

    return run, check


@case
def knn_k2_k4(hip, ctx):
    """`pf_knn` (`k_knn_grid<D, K>`) at d = 3 for k = 2 and 4."""
    ref, qry = _cloud(2500, 3, 61), _with_nan(_cloud(301, 3, 62), 100)
    big = (_cloud(6000, 4, 63), _cloud(700, 4, 64))
    ok = ~np.isnan(qry).any(axis=1)

    def run(neighbour):
        if neighbour:
            ctx.knn(big[0], big[1], 4)
        return [ctx.knn(ref, qry, k) for k in (2, 4)]

    def check(out):
        widx, wd2 = kr.brute_argmin(ref, qry[ok], 4)
        for k, (idx, d2) in zip((2, 4), out):  # (test_tail_kernels.check_topk and test_topk_nan_queries)
            assert idx.dtype == np.int64 and idx.shape == (len(qry), k)
            assert np.array_equal(idx[ok], widx[:, :k]) and np.array_equal(d2[ok], wd2[:, :k])
            assert np.all(idx[~ok] == kr.NO_NEIGHBOUR) and np.all(np.isposinf(d2[~ok]))

    return run, check


@case
def knn_topk_lists(hip, ctx):
    """`pf_knn_topk`: the exhaustive scan at d = 20 and k = 64, the hierarchy's lists at d = 16 and k = 64 over two supers."""
    sets = [(_cloud(700, 20, 71), _with_nan(_cloud(91, 20, 72), 45), 64), (_cloud(4200, 16, 73), _with_nan(_cloud(131, 16, 74), 9), 64),
            (_cloud(900, 3, 75), _cloud(257, 3, 76), 9)]
    big = [(_cloud(1500, 40, 77), _cloud(200, 40, 78), 64), (_cloud(8500, 16, 79), _cloud(300, 16, 80), 64)]

    def run(neighbour):
        if neighbour:
            for ref, qry, k in big:
                ctx.knn_topk(ref, qry, k)
        return [ctx.knn_topk(ref, qry, k) for ref, qry, k in sets]

    def check(out):
        for (ref, qry, k), (idx, d2) in zip(sets, out):  # (test_knn_topk.check and test_nan_queries_have_no_neighbour)
            ok = ~np.isnan(qry).any(axis=1)
            ridx, rd2 = kr.brute(ref, qry[ok], k)
            assert idx.dtype == np.int64 and d2.dtype == np.float64 and idx.shape == d2.shape == (len(qry), k)
            assert np.array_equal(idx[ok], ridx) and np.array_equal(d2[ok], rd2)
            assert np.all(idx[~ok] == kr.NO_NEIGHBOUR) and np.all(d2[~ok] == np.inf)

    return run, check


# ------------------------------------------------------------------------------------------------ assignment
def _assign_out(ctx, A, B):
    col, stats, u, v = ctx.assign(A, B, return_duals=True)
    s = stats.as_dict()
    ints = {k: int(x) for k, x in s.items() if isinstance(x, (int, np.integer)) and not isinstance(x, bool)}
    return col, u, v, ints, float(stats.total_cost), float(stats.gap_bound)


def _check_assignment(A, B, out):
    """`test_assignment.test_random_clouds_match_scipy`'s criterion."""
    import test_assignment as ta

    col, u, v, ints, total, gap = out
    rs, cs = ta._lsa(A, B)
    assert np.array_equal(rs, np.arange(len(A))) and np.array_equal(col, cs)
    want = ta._cost(A, B, rs, cs)
    assert abs(total - want) <= 1e-12 * want
    assert gap <= 1e-10 * total
    assert np.all(v <= 0.0)
    ta._check_certificate(A, B, col, u, v, gap)


def _assign_case(ctx, A, B, bigA, bigB, dense):
    def run(neighbour):
        if neighbour:
            ctx.assign(bigA, bigB)
        return _assign_out(ctx, A, B)

    def check(out):
        _check_assignment(A, B, out)
        assert (out[3]["dense_bids"] > 0) == dense  # the queued dense path ran (or never had to)
        assert out[3]["phases"] >= 1 and out[3]["dense_passes"] >= 1

    return run, check


@case
def assign_full_lists(hip, ctx):
    """n_cols <= 16: every list is complete (`rad` infinite), the short lists' tail entries are never read."""
    rng = np.random.default_rng(81)
    A, B, bigA, bigB = (rng.uniform(size=shape) for shape in ((11, 3), (14, 3), (30, 4), (33, 4)))
    return _assign_case(ctx, A, B, bigA, bigB, False)


@case
def assign_rectangular(hip, ctx):
    """300 x 450: virtual rows, more than one block of 256 columns, two partial results of the price reduction."""
    rng = np.random.default_rng(82)
    A, B = rng.uniform(size=(300, 3)), rng.uniform(size=(450, 3))
    run, check = _assign_case(ctx, A, B, rng.uniform(size=(900, 5)), rng.uniform(size=(900, 5)), False)  # (a square one: 0.1 s)

    def check_any_path(out):  # (which way the bids went is not this case's point)
        _check_assignment(A, B, out)

    return run, check_any_path


@case
def assign_clustered_dense_bids(hip, ctx):
    """Rows in one tight cluster, columns mostly far away: the 16 nearest columns are soon priced out and rows queue for
    the dense bid (`queue`, `k_as_dense`)."""
    rng = np.random.default_rng(83)
    A = 0.01 * rng.standard_normal((200, 3))
    B = np.concatenate([0.01 * rng.standard_normal((20, 3)), rng.uniform(2.0, 3.0, size=(230, 3))])
    return _assign_case(ctx, A, B, rng.uniform(size=(500, 4)), rng.uniform(size=(500, 4)), True)


# ------------------------------------------------------------------------------------------------ mesh units
@case
def curvatures_every_output(hip, ctx):
    """`pf_curvatures` with every output on a closed blob and on the messy one (non-manifold, one-way, unreferenced)."""
    import _curvature_ref as cref
    import test_curvature as tc
    from pyfocusr_amd import discrete_curvatures
    from pyfocusr_amd.meshgen import blob_mesh

    names = ["blob700", "messy700"]
    big = blob_mesh(3000, seed=2)

    def run(neighbour):
        if neighbour:
            ctx.curvatures(big.points, big.faces)
        return [_drop(dict(discrete_curvatures(*tc.case(name)[:2], ctx=ctx))) for name in names]

    def check(out):
        for name, dev in zip(names, out):  # (test_device_counts_and_masks_... and test_device_fields_against_the_reference)
            r = tc.case(name)[2]
            assert np.array_equal(dev["topology"], r["topology"]) and np.array_equal(dev["boundary"], r["boundary"])
            got = cref.ratios(dev, r)
            for field in sorted(got):
                assert tc.BOUND[field] <= 1e-10 and got[field] <= tc.BOUND[field], (name, field, got[field])
            zero = r["area"] == 0.0
            for field in ("gaussian", "mean", "k_min", "k_max", "tensor", "tensor_k_min", "tensor_k_max", "d_min", "d_max", "normals"):
                assert np.all(dev[field][zero] == 0.0) and np.all(np.isfinite(dev[field])), (name, field)

    return run, check


@case
def curvatures_one_output(hip, ctx):
    """`pf_curvatures` asked for the mean curvature alone: the other output blocks are not taken, the kernel skips them."""
    import ctypes as C

    import test_curvature as tc
    from pyfocusr_amd.meshgen import blob_mesh

    pts, faces, r = tc.case("blob700")
    big = blob_mesh(3000, seed=2)
    lib = hip.load_library()
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def run(neighbour):
        if neighbour:
            ctx.curvatures(big.points, big.faces)
        mean = np.empty(len(pts))
        topology = np.zeros(5, dtype=np.int64)
        rc = lib.pf_curvatures(ctx._h, pts.ctypes.data_as(f64p), len(pts), faces.ctypes.data_as(i32p), len(faces), None, None,
                               mean.ctypes.data_as(f64p), None, None, None, None, None, topology.ctypes.data_as(C.POINTER(C.c_int64)), None)
        assert rc == 0
        return mean, topology

    def check(out):
        mean, topology = out
        every = ctx.curvatures(pts, faces)
        assert mean.tobytes() == every["mean"].tobytes() and np.array_equal(topology, r["topology"])
        assert np.all(np.abs(mean - r["mean"]) <= tc.BOUND["mean"] * r["mag_mean"])

    return run, check


@case
def mesh_cluster_seeds_and_dual(hip, ctx):
    """`pf_mesh_cluster` from seeds with the dual mesh (5000 vertices to 60 clusters: 26 iterations, more than one block of
    vertices and of faces), and from given centroids and labels without faces."""
    import _remesh_ref as rr
    import test_remesh as tr

    from pyfocusr_amd.meshgen import blob_mesh

    P, F, a, sel, r = tr.case(5000, 60, 40)
    P2, a2, labels2, C2 = tr._update_case()
    big = blob_mesh(10500, seed=3)
    big_seeds = np.arange(0, 10500, 70)

    def run(neighbour):
        if neighbour:
            ctx.cluster_mesh(big.points, big.faces, np.ones(len(big.points)), seeds=big_seeds, n_iter=3)
        return (_drop(ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=40)),
                _drop(ctx.cluster_mesh(P2, None, a2, centroids=C2, labels=labels2, n_iter=1, update_only=True)),
                _drop(ctx.cluster_mesh(P, None, a, centroids=r["centroids"], n_iter=0)))

    def check(out):
        whole, update, assigned = out
        assert whole["n_iter_run"] == tr.BLOBS["5000to60"][2]
        tr._assert_equals_reference(whole, r, "5000to60")  # (test_whole_call_equals_the_reference)
        want = rr.update(P2, a2, labels2, C2)  # (test_one_update_step_gives_the_centroids_bit_for_bit)
        assert update["centroids"].tobytes() == want.tobytes() and np.array_equal(update["labels"], labels2)
        assert np.array_equal(update["rep"], rr.representatives(P2, want, labels2)[0])
        assert np.array_equal(assigned["labels"], r["labels"])  # the converged centroids assign what they were made from
        assert np.array_equal(assigned["rep"], r["rep"]) and np.array_equal(assigned["count"], r["count"])

    return run, check


# ------------------------------------------------------------------------------------------------ sampling, descriptors
@case
def fps_with_voronoi_masses(hip, ctx):
    """`pf_fps`: 2500 points are ten blocks of partial bests, m = 300 rounds; from the centroid and from a given start; the
    Voronoi masses of the owners."""
    import test_sampling as ts
    from pyfocusr_amd import farthest_point_sampling, voronoi_masses

    sets = [(ts.cloud(2500, 3), 300, -1), (ts.cloud(2500, 5), 300, 1234)]
    mass = np.random.default_rng(3).uniform(0.5, 1.5, 2500)
    big = ts.cloud(5200, 16)

    def run(neighbour):
        if neighbour:
            ctx.farthest_point_sampling(big, 610, return_owner=True, return_d2=True)
        out = []
        for P, m, start in sets:
            sel, owner, d2 = farthest_point_sampling(P, m, start=None if start < 0 else start, return_owner=True, return_d2=True, ctx=ctx)
            out.append((sel, owner, d2, voronoi_masses(owner, mass, m)))
        return out

    def check(out):
        for (P, m, start), (sel, owner, d2, w) in zip(sets, out):  # (test_sampling.check, test_voronoi_masses)
            ts.assert_clear_first_sample(P)
            rsel, rowner, rd2 = ts.pr.fps(P, m, start=start)
            assert sel.dtype == np.int64 and owner.dtype == np.int32 and d2.dtype == np.float64
            assert np.array_equal(sel, rsel) and np.array_equal(owner, rowner) and np.array_equal(d2, rd2)
            assert np.array_equal(w, np.bincount(owner, weights=mass, minlength=m)) and np.all(w > 0.0)

    return run, check


@case
def descriptors_and_coefficients(hip, ctx):
    """`pf_spectral_descriptors` and `pf_descriptor_coefficients` at 1500 rows: three blocks of DESC_ROWS = 512, the last one
    ragged, so that the coefficients go through the per-block partial sums and `k_desc_combine`."""
    import _descriptor_ref as dr
    import test_spectral_descriptors as tsd

    n, K, k_out, T = 1500, 20, 8, 200
    phi, G, mass = tsd.random_tables(n, K, T, seed=2)
    bphi, bG, bmass = tsd.random_tables(3100, 41, 410, seed=3)

    def run(neighbour):
        if neighbour:
            ctx.spectral_descriptors(bphi, bG)
            ctx.descriptor_coefficients(bphi, bmass, bG, 17)
        return ctx.spectral_descriptors(phi, G), ctx.descriptor_coefficients(phi, mass, G, k_out)

    def check(out):
        F, A = out
        assert F.shape == (n, T) and F.tobytes() == dr.descriptors(phi, G).tobytes()
        ref, ref_abs = dr.coefficients_long(phi, mass, G, k_out)  # (test_coefficients_within_the_summation_bound)
        assert A.shape == (k_out, T)
        assert np.all(np.abs(A.astype(np.longdouble) - ref) <= (n + K + 4) * tsd.EPS * ref_abs)

    return run, check


@case
def mesh_topology_every_output(hip, ctx):
    """`pf_mesh_topology` with every output and the outward rule, on a closed blob with 40 reversed faces (a flipped patch:
    the orientation rounds, the volume's sorted sums) beside an open cylinder (a second component with two boundary
    loops: the loop pass allocates), and once more without points."""
    import _topology_ref as tref
    import test_topology as tt
    from pyfocusr_amd import mesh_topology

    bp, bf = tt._reversed_blob(700, 1, 40, 7)[:2]
    cp, cf = tref.open_cylinder(40, 6)
    cf = tref.reverse(cf, [3, 4, 77])
    pts = np.ascontiguousarray(np.concatenate([bp, np.asarray(cp) + [0.0, 0.0, 50.0]]), dtype=np.float64)
    faces = np.ascontiguousarray(np.concatenate([bf, np.asarray(cf) + len(bp)]), dtype=np.int32)
    refs = {outward: tref.topology(len(pts), faces, pts, outward=outward) for outward in (True, False)}
    big_p, big_f, _ = tt.case("blob5000_reversed")

    def fields(dev):  # (rounds and loop rounds depend on the order the hooks land in: test_two_calls_give_the_same_bits)
        return {k: dev[k] for k in sorted(dev) if k not in ("device_ms", "rounds", "loop_rounds")}, (dev["rounds"], dev["loop_rounds"])

    def run(neighbour):
        if neighbour:
            mesh_topology((big_p, big_f), ctx=ctx)
        both = [fields(mesh_topology((pts, faces), outward=outward, ctx=ctx)) for outward in (True, False)]
        run.rounds = [r for _, r in both]
        return [f for f, _ in both]

    def check(out):
        for outward, dev, (rounds, loop_rounds) in zip((True, False), out, run.rounds):
            r = refs[outward]
            tt._assert_equal_integers(dev, r, "blob and cylinder")  # (test_device_integers_equal_the_reference)
            assert dev["n_patches"] == 2 and dev["n_boundary_loops"] == 2 and dev["flip"].any()
            assert rounds >= 1 and loop_rounds >= 1  # the labelling ran, and the loop pass took its blocks
        want, got, mag = refs[True]["patches"]["signed_volume"], out[0]["patches"]["signed_volume"], refs[True]["volume_terms"]
        assert want[0] > 1e-3 * mag[0] and abs(got[0] - want[0]) <= 1e-12 * mag[0]  # (test_device_signed_volume; the blob)
        assert got[1] == 0.0 and np.all(out[1]["patches"]["signed_volume"] == 0.0)  # the open patch, and no outward rule

    return run, check


@case
def map_distortion_with_and_without_normals(hip, ctx):
    """`pf_map_distortion`: a vertex map with target normals, a 3-corner map with weights and unmapped rows, a map without
    normals (`imgn` is not taken); 1396 faces are six groups of the totals' first level."""
    import _map_quality_ref as mref
    import test_map_quality as tm

    names = ["nearest", "surface", "cone"]
    bp, bf = tm._blob(1900, 6)
    bn = np.random.default_rng(6).standard_normal(bp.shape)

    def run(neighbour):
        if neighbour:
            ctx.map_distortion(bp, bf, bp, tm._identity(len(bp)), None, bn)
        return [_drop(ctx.map_distortion(*tm.case(name)[0])) for name in names]

    def check(out):
        for name, dev in zip(names, out):  # (test_device_equals_the_reference)
            r = tm.case(name)[1]
            for field in mref.INT_FIELDS:
                assert dev[field].dtype == r[field].dtype and np.array_equal(dev[field], r[field]), (name, field)
            for field in mref.FLOAT_FIELDS:
                assert np.all(np.isfinite(dev[field])) and np.array_equal(dev[field], r[field]), (name, field)
        assert np.any(out[1]["vertex_flags"] & 8) and out[2]["report"][2] == -1  # unmapped corners; nothing can be flagged flipped

    return run, check


# ------------------------------------------------------------------------------------------------ CPD
@case
def cpd_handle_and_gram(hip, ctx):
    """`pf_cpd_*` on one handle at d = 3 (E-step, basis, weighted Gram, affine and deformable sums and transforms,
    download) and the E-step at d = 16; N = 259 and M = 131 are no multiples of MOM_ROWS = 64, CPD_CHUNK = 128 or the
    block.  `pf_cpd_gram` with B aliased to A and with a B of its own.  The larger neighbour: a larger handle on the ctx,
    and a basis of K = 40 on the case's handle before its K = 7 (`mpart`, `msum`, `hpart` then hold the larger one's sums)."""
    import test_cpd_kernels as tk

    ref = tk.ref
    N, M, K = 259, 131, 7
    X, Y = tk.clouds(2103, N, M, 3)
    X16, Y16 = tk.clouds(2116, N, M, 16)
    rng = np.random.default_rng(2100)
    Q, Cm = rng.normal(size=(M, K)), 0.05 * rng.normal(size=(K, 3))
    Qbig = rng.normal(size=(M, 40))
    B, t = np.eye(3) + 0.05 * rng.normal(size=(3, 3)), 0.05 * rng.normal(size=3)  # (the clouds stay on top of each other)
    V = rng.normal(size=(M, 9))
    A2 = 0.5 * rng.normal(size=(200, 3))
    bigX, bigY = tk.clouds(2200, 600, 300, 3)
    s2, s16, w = 0.2, tk.sigma2_for(16), 0.1

    def copies(arrays):
        return tuple(np.array(a) for a in arrays)

    def run(neighbour):
        if neighbour:
            big = hip.DeviceCpd(bigX, bigY, ctx=ctx)
            big.set_basis(rng.normal(size=(300, 20)))
            big.estep_resident(s2, w)
            big.deform_sums()
            big.affine_sums()
            big.close()
            hip.gaussian_gram_product(bigX, bigX, 0.7, rng.normal(size=(600, 20)), ctx=ctx)
        out = {}
        dev = hip.DeviceCpd(X, Y, ctx=ctx)
        try:
            if neighbour:
                dev.set_basis(Qbig)
                dev.estep_resident(s2, w)
                dev.deform_sums()
                dev.apply_deform(np.zeros((40, 3)))
            dev.set_basis(Q)
            out["estep"] = copies(dev.estep(Y, s2, w))
            out["H_alone"] = np.array(dev.weighted_gram())
            out["deform_sums"] = copies(dev.deform_sums())
            out["affine_sums"] = {k: np.array(v) for k, v in dev.affine_sums().items()}
            dev.apply_affine(B, t)
            out["TY_affine"] = np.array(dev.download()[0])
            dev.estep_resident(s2, w)
            out["variance_sums"] = np.array(dev.apply_deform(Cm))
            out["resident"] = copies(dev.download())
        finally:
            dev.close()
        dev = hip.DeviceCpd(X16, Y16, ctx=ctx)
        try:
            out["estep16"] = copies(dev.estep(Y16, s16, w))
        finally:
            dev.close()
        out["gram_aliased"] = hip.gaussian_gram_product(Y, Y, 0.7, V, ctx=ctx)
        out["gram_own"] = hip.gaussian_gram_product(A2, Y, 0.7, V, ctx=ctx)
        return out

    def check(out):
        tk.check_estep("pool", "d=3", out["estep"], X, Y, s2, w)
        tk.check_estep("pool", "d=16", out["estep16"], X16, Y16, s16, w)
        P1, Pt1, PX = out["estep"]
        (wH, wR), (H_abs, R_abs) = ref.deform_sums_ld(Q, P1, PX, Y)  # (test_weighted_gram_and_deform_sums)
        H, R = out["deform_sums"]
        assert np.array_equal(out["H_alone"], H)
        tk.within("pool", "H", H, wH, tk.sum_bound(M, H_abs))
        tk.within("pool", "R", R, wR, tk.sum_bound(M, R_abs))
        got = out["affine_sums"]  # (test_affine_moments)
        for name, cloud, n in (("cx", X, N), ("cy", Y, M)):
            mean, mean_abs = ref.mean_ld(cloud)
            tk.within("pool", name, got[name], mean, tk.sum_bound(n, mean_abs))
        want, s_abs = ref.affine_moments_ld(P1, Pt1, PX, X, Y, got["cx"], got["cy"])
        assert set(want) | {"cx", "cy"} == set(got)
        for name in want:
            tk.within("pool", name, got[name], want[name], tk.sum_bound(N if name.startswith("sPt1") else M, s_abs[name]))
        want, s_abs = ref.affine_ld(Y, B, t)  # (test_apply_affine)
        tk.within("pool", "TY = Y B + t", out["TY_affine"], want, 4.0 * (3 + 2) * tk.EPS * s_abs)
        TY, rP1, rPt1, rPX = out["resident"]  # (check_apply_deform)
        want_TY, TY_abs = ref.deform_ld(Y, Q, Cm)
        tk.within("pool", "TY = Y + Q C", TY, want_TY, 4.0 * (K + 2) * tk.EPS * TY_abs)
        want, s_abs = ref.variance_sums_ld(rP1, rPt1, rPX, X, TY)
        tk.within("pool", "variance sums", out["variance_sums"], want, [tk.sum_bound(n, s) for n, s in zip((M, M, M, N, N), s_abs)])
        tk.check_estep("pool", "resident", (rP1, rPt1, rPX), X, out["TY_affine"], s2, w)
        tk.check_gram("pool", "Y, Y", out["gram_aliased"], Y, Y, 0.7, V)  # (test_gram_aliased_operands, test_gram_edges)
        tk.check_gram("pool", "A, Y", out["gram_own"], A2, Y, 0.7, V)

    return run, check


# ------------------------------------------------------------------------------------------------ functional maps
@case
def knn1_wide_scan(hip, ctx):
    """`pf_knn1_wide` at d = 17 (padded to 24 coordinates) and d = 128, counted and plain; 203 queries leave the second
    query of most lanes and the tail of `ld` unused, 700 references are split into ranges that `k_wide_merge` joins."""
    import _fmap_ref as fr
    import test_functional_maps as tf

    sets = [tf.cloud(d, 700, 203) for d in (17, 128)]
    sets = [(ref, _with_nan(qry, 101)) for ref, qry in sets]
    big = tf.cloud(128, 1500, 600)

    def run(neighbour):
        if neighbour:
            ctx.knn1_wide(*big)
        out = []
        for ref, qry in sets:
            ctx.knn1_wide_count(True)
            try:
                counted = ctx.knn1_wide(ref, qry, return_d2=True)
            finally:
                pairs = ctx.knn1_wide_count(False)
            out.append((counted, pairs, ctx.knn1_wide(ref, qry, return_d2=True)))
        return out

    def check(out):
        for (ref, qry), (counted, pairs, plain) in zip(sets, out):  # (test_functional_maps.check_wide)
            ok = ~np.isnan(qry).any(axis=1)
            ridx, rd2 = fr.brute_force_nn(ref, qry[ok])
            for idx, d2 in (counted, plain):
                assert idx.dtype == np.int64 and np.array_equal(idx[ok], ridx) and np.array_equal(d2[ok], rd2)
                assert np.all(np.isposinf(d2[~ok]))  # a NaN query is nearer to nothing
            assert pairs > 0  # the counting kernel ran

    return run, check


@case
def functional_map_handle(hip, ctx):
    """`pf_fmap_*` on one handle of 700 x 700 vertices and K = 40: project (700 rows are two PROJ_ROWS blocks: `part` and
    `k_fmap_combine`), convert through the narrow (k_t = 12) and the wide search (k_t = 24), zoomout, set_samples and
    zoomout_sampled.  The larger neighbour, on the same handle: a zoomout over a larger k range and a larger sample set."""
    import _fast_zoomout_ref as zr
    import _fmap_ref as fr
    import test_fast_zoomout as tz
    import test_functional_maps as tf

    p = tf.blob_pair(700, 0, 40)
    phi_t, phi_s, mass = p["phi_t"], p["phi_s"], p["mass_s"]
    T0 = fr.corrupt(p["T_true"], 0.3)
    T6 = fr.corrupt(p["T_true"], 0.6)
    S_t, S_s = tz.reference_samples(100)
    S_t200, S_s200 = tz.reference_samples(200)
    rng = np.random.default_rng(9)
    C12, C24 = rng.standard_normal((24, 12)), rng.standard_normal((24, 24))
    EPS = tf.EPS

    def run(neighbour):
        out = {}
        with hip.DeviceFunctionalMap(phi_t, phi_s, mass, ctx=ctx) as h:
            if neighbour:
                h.set_p2p(T6)
                h.zoomout(4, 40, 1, 1)
                h.set_samples(S_t200, S_s200)
                h.zoomout_sampled(4, 30, 1, 1)
            h.set_p2p(T0)
            out["project"] = h.project(17, 33)
            for name, Cm in (("narrow", C12), ("wide", C24)):
                h.convert(24, Cm.shape[1], Cm)
                out["convert_" + name] = h.get_p2p(return_d2=True)
            h.set_p2p(T0)
            out["zoomout_C"] = h.zoomout(5, 18, 3, 1)
            out["zoomout_T"] = h.get_p2p(return_d2=True)
            h.set_p2p(T6)
            h.set_samples(S_t, S_s)
            out["sampled_C"] = h.zoomout_sampled(4, 20, 1, 0)
            out["sampled_T"] = h.get_p2p(return_d2=True)
        return out

    def check(out):
        C = out["project"]  # (test_projection_within_the_summation_bound)
        bound = 2.0 * (700 + 2) * EPS * fr.project_abs(phi_t, phi_s, mass, T0, 17, 33)
        assert C.shape == (17, 33) and np.all(np.abs(C - fr.project(phi_t, phi_s, mass, T0, 17, 33)) <= bound)
        for name, Cm in (("narrow", C12), ("wide", C24)):  # (test_converted_indices_are_optimal_up_to_the_rounding_of_q)
            T, d2 = out["convert_" + name]
            k_s, k_t = Cm.shape
            assert T.shape == (700,) and T.min() >= 0 and T.max() < 700
            Q = phi_s[:, :k_s] @ Cm
            ref_t = phi_t[:, :k_t]
            _, best = fr.brute_force_nn(ref_t, Q)
            got = fr.row_d2(ref_t[T], Q)
            delta = 2.0 * (k_s + 2) * EPS * np.linalg.norm(np.abs(phi_s[:, :k_s]) @ np.abs(Cm), axis=1)
            assert np.all(np.sqrt(best) * (1.0 + (k_t + 2) * EPS) + 2.0 * delta - np.sqrt(got) >= 0.0)
            assert np.all(np.abs(np.sqrt(d2) - np.sqrt(got)) <= 2.0 * delta + (k_t + 2) * EPS * np.sqrt(got))
        rT, rC = fr.zoomout(phi_t, phi_s, mass, T0, 5, 18, step=3, n_iter_at_end=1)  # (test_zoomout_follows_the_reference_loop)
        assert np.array_equal(out["zoomout_T"][0], rT)
        assert np.all(np.abs(out["zoomout_C"] - rC) <= 2.0 * 702 * EPS * np.abs(phi_s[:, :18] * mass[:, None]).sum(0)[:, None]
                      * np.abs(phi_t[:, :18]).max(0)[None, :])
        rT, rC = zr.zoomout_sampled(phi_t, phi_s, mass, T6, S_t, S_s, 4, 20, step=1, n_iter_at_end=0)  # (test_sampled_zoomout_end_to_end)
        assert np.array_equal(rT, p["T_true"]) and np.array_equal(out["sampled_T"][0], p["T_true"])
        assert out["sampled_C"].shape == (20, 20) and np.max(np.abs(out["sampled_C"] - rC)) <= 1e-9

    return run, check


# ------------------------------------------------------------------------------------------------ surfaces
def _torus_quads(nu=72, nv=30):
    """2160 quads = 4320 fan triangles: 68 chunks of 64 (the last one half full) in two super-chunks; the last vertex, in
    the middle of the hole, is one no face references (its pseudonormal is 0)."""
    uu, vv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    au, av = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
    pts = np.stack([(3 + np.cos(av)) * np.cos(au), (3 + np.cos(av)) * np.sin(au), np.sin(av)], axis=-1).reshape(-1, 3)
    pts = np.concatenate([pts, [[0.0, 0.0, 0.0]]])
    quads = np.stack([uu * nv + vv, ((uu + 1) % nu) * nv + vv, ((uu + 1) % nu) * nv + (vv + 1) % nv, uu * nv + (vv + 1) % nv], axis=-1)
    return np.ascontiguousarray(pts), np.ascontiguousarray(quads.reshape(-1, 4), dtype=np.int32)


def _surface_queries(pts, n, seed, bad_row):
    """Points of the bounding box scaled by 1.2 and points near the vertices; one row is not finite."""
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(0), pts.max(0)
    mid, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    q = np.concatenate([rng.uniform(mid - half, mid + half, size=(n - n // 2, 3)),
                        pts[rng.integers(0, len(pts), n // 2)] + 0.05 * rng.standard_normal((n // 2, 3))])
    q[bad_row, 1] = np.nan
    return np.ascontiguousarray(q)


def _larger_surface_neighbour(hip, ctx, n_qry):
    """Every query kind on a surface of 9996 triangles with `n_qry` queries, then closed: its blocks go back to the pool."""
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(5000, seed=4)
    q = _surface_queries(m.points, n_qry, 5, 0)
    d = np.tile([0.3, 0.5, 0.8], (len(q), 1))
    big = hip.DeviceSurface(m.points, m.faces, ctx=ctx)
    try:
        big.distance(q)
        big.raycast(q, d)
        big.raycast(q, d, count=True)
        if n_qry < 16 * 4096:
            big.closest(q)
            big.signed_distance(q)
            big.winding_number(q)
            big.winding_number(q, beta=2.0)
    finally:
        big.close()


@case
def surface_queries_small_packets(hip, ctx):
    """One `DeviceSurface` of quads, built and prepared (signed structure, dipoles) inside every run: closest, distance with
    its statistics, signed distance with the topology counts, winding numbers exact and at beta = 2 with the bound, ray
    casts for the first hit and with counts, vertex normals; 1203 queries are packets of 4, the last one ragged."""
    import _ray_ref as rr
    import _signed_ref as sref
    import test_signed_distance as tsd
    import test_winding_number as tw
    from oracle import icp_port

    pts, quads = _torus_quads()
    q = _surface_queries(pts, 1203, 91, 600)
    ok = np.isfinite(q).all(axis=1)
    d = np.tile([0.3, 0.5, 0.8] / np.linalg.norm([0.3, 0.5, 0.8]), (len(q), 1))

    def run(neighbour):
        if neighbour:
            _larger_surface_neighbour(hip, ctx, 2500)
        out = {}
        surf = hip.DeviceSurface(pts, quads, ctx=ctx)
        try:
            out["closest"] = surf.closest(q)
            out["distance"] = surf.distance(q)
            out["topology"] = {k: v for k, v in surf.topology().items() if k != "volume"}  # (the volume is host numpy)
            out["signed"] = surf.signed_distance(q)
            out["normals"] = surf.vertex_normals()
            out["winding"] = surf.winding_number(q)
            out["winding_beta"] = surf.winding_number(q, beta=2.0)
            out["ray"] = surf.raycast(q, d)
            out["ray_count"] = surf.raycast(q, d, count=True)
            run.volume = surf.topology()["volume"]
        finally:
            surf.close()
        return out

    def check(out):
        want_pt, want_face, want_d2 = icp_port.closest_points_on_surface(pts, quads, q[ok])  # (test_surface_distance._check_brute)
        cpt, cface, cd2 = out["closest"]
        d2, face, stats = out["distance"]
        assert np.array_equal(d2[ok], want_d2) and np.array_equal(face[ok], want_face)
        assert np.array_equal(cd2[ok], want_d2) and np.array_equal(cface[ok], want_face) and np.array_equal(cpt[ok], want_pt)
        assert np.all(np.isnan(d2[~ok])) and np.all(face[~ok] == -1)
        dist = np.sqrt(d2[ok])  # (test_distance_nan_queries_are_counted_and_excluded, ..._stats_agree_with_numpy...)
        assert stats["n_nan"] == 1 and stats["n_finite"] == ok.sum() and stats["argmax"] == np.flatnonzero(ok)[np.argmax(dist)]
        np.testing.assert_allclose(stats["sum_d"], dist.sum(), rtol=1e-12)
        np.testing.assert_allclose(stats["sum_d2"], np.sum(dist * dist), rtol=1e-12)
        assert abs(stats["max_d"] - dist.max()) <= np.spacing(dist.max())
        counts = sref.topology_counts(quads)
        topo = out["topology"]
        assert (topo["n_edges"], topo["n_boundary_edges"], topo["n_nonmanifold_edges"], topo["n_inconsistent_edges"]) == tuple(counts)
        assert topo["closed"] and run.volume != 0.0
        sd, sface, feature, amb = out["signed"]
        tsd._assert_magnitude_exact(sd, sface, d2, face)  # (test_magnitude_and_face_bitwise_...)
        w_ref = sref.winding_number(pts, quads, q[ok])  # (test_sign_against_star_shape_and_winding_number)
        assert np.all(np.abs(w_ref - np.round(w_ref)) < 1e-6) and amb == 0
        inside = np.round(np.abs(w_ref)) == 1.0
        assert inside.any() and not inside.all()
        assert np.array_equal((sd[ok] < 0) if run.volume > 0 else (sd[ok] > 0), inside)
        assert set(np.unique(feature[ok])) <= {0, 1, 2} and feature[~ok].tolist() == [-1]
        w, bound = out["winding"]  # (test_exact_mode_against_reference, test_hierarchical_mode_within_its_own_bound)
        tol = 1e-9 * tw.wr.diagonal(pts)
        keep = dist >= tol
        assert np.all(bound[ok] == 0.0) and np.max(np.abs(w[ok] - w_ref)[keep]) <= tw.TOL and np.isnan(w[~ok]).all()
        wb, bb = out["winding_beta"]
        assert np.all(np.abs(wb[ok] - w[ok]) <= bb[ok] + tw.TOL) and np.any(bb[ok] > 0.0)  # (some cluster went in as a dipole)
        want = rr.cast(pts, quads, q[ok], d[ok])  # (test_ray_casting._same)
        for got in (out["ray_count"], out["ray"]):
            for g, x in zip(got, want):
                assert g.dtype == x.dtype and np.array_equal(g[ok], x, equal_nan=True)
            assert np.isnan(got[0][~ok]).all() and got[1][~ok].tolist() == [-1]
        assert np.isfinite(want[0]).any() and np.isinf(want[0]).any() and out["ray_count"][3][~ok].tolist() == [0]
        tri = sref.fan_triangles(quads)  # (test_mesh_units_small: sum of angle x unit normal over the corners of a vertex)
        X = pts[tri]
        cr = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        tn = cr / np.linalg.norm(cr, axis=1)[:, None]
        ref_vn, angsum = np.zeros_like(pts), np.zeros(len(pts))
        for j in range(3):
            e1, e2 = X[:, (j + 1) % 3] - X[:, j], X[:, (j + 2) % 3] - X[:, j]
            ang = np.arctan2(np.linalg.norm(np.cross(e1, e2), axis=1), np.einsum("ij,ij->i", e1, e2))
            np.add.at(ref_vn, tri[:, j], ang[:, None] * tn)
            np.add.at(angsum, tri[:, j], ang)
        assert np.all(np.abs(out["normals"] - ref_vn) <= 16 * np.finfo(np.float64).eps * angsum[:, None])

    return run, check


@case
def surface_queries_large_packets(hip, ctx):
    """`distance` with its statistics and `raycast` (first hit, and with counts) at 16 x 4096 = 65 536 queries: packets of
    16.  The reference is taken on 200 sampled rows; the statistics against numpy over the device's own distances."""
    import _ray_ref as rr
    from oracle import icp_port

    pts, quads = _torus_quads()
    n = 16 * 4096
    q = _surface_queries(pts, n, 92, 40000)
    ok = np.isfinite(q).all(axis=1)
    d = np.tile([0.3, 0.5, 0.8] / np.linalg.norm([0.3, 0.5, 0.8]), (n, 1))
    rows = np.sort(np.random.default_rng(93).choice(np.flatnonzero(ok), 200, replace=False))

    def run(neighbour):
        if neighbour:
            _larger_surface_neighbour(hip, ctx, 2 * n)
        surf = hip.DeviceSurface(pts, quads, ctx=ctx)
        try:
            return {"distance": surf.distance(q), "stats_only": surf.distance(q, per_point=False)[2], "ray": surf.raycast(q, d),
                    "ray_count": surf.raycast(q, d, count=True)}
        finally:
            surf.close()

    def check(out):
        d2, face, stats = out["distance"]
        _, want_face, want_d2 = icp_port.closest_points_on_surface(pts, quads, q[rows])
        assert np.array_equal(d2[rows], want_d2) and np.array_equal(face[rows], want_face)
        assert np.all(np.isnan(d2[~ok])) and np.all(face[~ok] == -1)
        dist = np.sqrt(d2[ok])  # (test_distance_stats_agree_with_numpy_and_repeat_bit_for_bit)
        assert stats == out["stats_only"] and stats["n_nan"] == 1 and stats["n_finite"] == n - 1
        np.testing.assert_allclose(stats["sum_d"], dist.sum(), rtol=1e-12)
        np.testing.assert_allclose(stats["sum_d2"], np.sum(dist * dist), rtol=1e-12)
        assert abs(stats["max_d"] - dist.max()) <= np.spacing(dist.max()) and stats["argmax"] == np.flatnonzero(ok)[np.argmax(dist)]
        want = rr.cast(pts, quads, q[rows], d[rows])
        for got in (out["ray_count"], out["ray"]):
            for g, x in zip(got, want):
                assert g.dtype == x.dtype and np.array_equal(g[rows], x, equal_nan=True)
            assert np.isnan(got[0][~ok]).all() and got[1][~ok].tolist() == [-1]
        assert np.array_equal(out["ray"][0], out["ray_count"][0], equal_nan=True) and np.array_equal(out["ray"][1], out["ray_count"][1])

    return run, check


@case
def surface_nd_closest(hip, ctx):
    """`DeviceSurfaceND.closest` at d = 3, 5 (the generic depth) and 16, pruned and exhaustive, with `last_search`; 4400
    triangles are 69 chunks in two super-chunks, 299 queries fill no packet of 8."""
    import test_surface_nd as tn

    sphere = tn._sphere_mesh(2200)
    depths = (3, 5, 16)
    big_pts, big_faces = tn._sphere_mesh(4600)
    big_q = tn._embed(np.random.default_rng(94).uniform(-1.0, 1.0, size=(640, 3)), 16)

    def run(neighbour):
        if neighbour:
            with hip.DeviceSurfaceND(tn._embed(big_pts, 16), big_faces, ctx=ctx) as big:
                big.closest(big_q)
                big.closest(big_q, exhaustive=True)
        out = []
        for dd in depths:
            coords, faces, q, _ = tn._sphere_case(sphere, dd)
            with hip.DeviceSurfaceND(coords, faces, ctx=ctx) as surface:
                pruned = surface.closest(q)
                stats = surface.last_search()
                exhaustive = surface.closest(q, exhaustive=True)
                out.append((pruned, stats, exhaustive, surface.last_search()))
        return out

    def check(out):
        for dd, (pruned, stats, exhaustive, stats_ex) in zip(depths, out):  # (test_equals_numpy_brute_force_pruned_and_exhaustive)
            _, faces, q, want = tn._sphere_case(sphere, dd)
            for got in (pruned, exhaustive):
                tn._same(dict(zip(("face", "vertices", "bary", "d2"), got)), want)
            assert stats["packets"] == (len(q) + 7) // 8 and stats["n_chunks"] == (len(faces) + 63) // 64
            assert 0 < stats["chunks_opened"] < stats["packets"] * stats["n_chunks"]  # the pruned search pruned
            assert stats_ex["chunks_opened"] == stats["packets"] * stats["n_chunks"]   # and the exhaustive one did not

    return run, check


# ------------------------------------------------------------------------------------------------ graphs
@case
def cotangent_build_and_apply(hip, ctx):
    """`pf_graph_build_cotan` on the messy blob (fins, flipped faces, stranded vertices; 1773 faces are seven blocks of the
    area's partial sums), `pf_graph_cotan_download`, and `pf_cotan_apply` with three columns and with one."""
    import _cotan_ref as cr
    import test_cotangent as tc

    name = "messy900"
    pts, faces = tc.mesh(name)
    big_pts, big_faces = tc.mesh("blob5000")
    x1 = np.random.default_rng(95).standard_normal((len(pts), 1))

    def run(neighbour):
        if neighbour:
            big = hip.DeviceLaplacian(big_pts, big_faces, ctx=ctx, cotangent=True)
            try:
                big.cotan_apply(np.ascontiguousarray(big_pts))
            finally:
                big.close()
        dev = hip.DeviceLaplacian(pts, faces, ctx=ctx, cotangent=True)
        try:
            return {"graph": dev.download(labels=True), "cotan": dev.cotan_download(), "hi": float(dev.hi), "area": float(dev.total_area),
                    "counts": (dev.n_isolated, dev.n_oneway, dev.n_components, dev.max_degree),
                    "apply3": dev.cotan_apply(np.ascontiguousarray(pts)), "apply1": dev.cotan_apply(x1)}
        finally:
            dev.close()

    def check(out):
        ref = tc.reference(name)  # (test_assembly_against_reference)
        h, c = out["graph"], out["cotan"]
        assert np.array_equal(h["rowptr"], ref["rowptr"]) and np.array_equal(h["colidx"], ref["colidx"])
        bound_w = 16 * tc.EPS * ref["w_bound"]
        row_bound = np.zeros(len(pts))
        np.add.at(row_bound, ref["rows"], bound_w)
        assert np.all(np.abs(c["w"] - ref["w"]) <= bound_w) and np.all(np.abs(c["diag"] - ref["diag"]) <= row_bound)
        assert np.all(np.abs(c["mass"] - ref["mass"]) <= 8 * tc.EPS * ref["mass"])
        off, sdiag, hi = cr.symmetric_operator(ref)
        np.testing.assert_allclose(out["hi"], hi, rtol=1e-13)
        np.testing.assert_allclose(out["area"], ref["total_area"], rtol=1e-13)
        np.testing.assert_allclose(-h["w"], off, rtol=1e-12, atol=1e-12 * hi)
        np.testing.assert_allclose(h["deg"], sdiag, rtol=1e-12, atol=1e-12 * hi)
        assert out["counts"][0] == ref["n_unreferenced"] > 0
        for x, got in ((pts, out["apply3"]), (x1, out["apply1"])):  # (test_mean_curvature_normals)
            want, bound = cr.apply(ref, x)
            assert got.shape == x.shape and np.all(np.abs(got - want) <= 16 * tc.EPS * bound)
            assert np.all(got[ref["mass"] == 0] == 0.0)

    return run, check


class _Resident(object):
    """What `test_tail_kernels._es_reference` reads of a graph, from host copies: the finalised block and the points."""

    def __init__(self, final, points):
        self._final, self._points = final, np.ascontiguousarray(points, dtype=np.float64)

    def final_rows(self, rows):
        return self._final[rows]

    def point_rows(self, rows):
        return self._points[rows]


@case
def graph_side_tails(hip, ctx):
    """On two small mesh graphs with eight finalised vectors: `pf_mean_filter` (4500 rows: a ragged second 4096-row pad
    block; three columns and two, the compile-time and the run-time kernel; two iterations), `pf_eigsort_costs` with 255
    and 257 samples, `pf_final_rows`, `pf_point_rows`, `pf_knn1_graphs`, `pf_rows_gather` / `scatter` / `fill`."""
    import test_tail_kernels as tt
    from pyfocusr_amd.meshgen import blob_mesh

    meshes = [blob_mesh(4500, seed=1), blob_mesh(1500, seed=0)]
    big_mesh = blob_mesh(9500, seed=2)
    W = tt._oracle_w(meshes[0].points, meshes[0].faces)
    rng = np.random.default_rng(96)
    vectors = [rng.standard_normal((m.points.shape[0], 8)) for m in meshes]
    v3, v2 = rng.standard_normal((4500, 3)), rng.standard_normal((4500, 2))
    k = 3
    col_t, sign_t, col_s, sign_s = tt._es_maps(k, rng)
    col_t, col_s = col_t % 8, col_s % 8
    rows_t, rows_s = rng.integers(0, 4500, 255).astype(np.int64), rng.integers(0, 1500, 257).astype(np.int64)
    sub = np.sort(rng.choice(4500, 700, replace=False)).astype(np.int64)
    x, vals = rng.standard_normal(4500), rng.standard_normal(700)

    def graph(mesh, vecs):
        g = hip.DeviceLaplacian(mesh.points, mesh.faces, ctx=ctx)
        g.ws_ensure(8)
        for slot in range(8):
            g.upload(slot, vecs[:, slot])
        return g, np.array(g.finalize_vectors(0, 8, minmax=True))

    def run(neighbour):
        if neighbour:
            big, _ = graph(big_mesh, rng.standard_normal((9500, 8)))
            try:
                big.mean_filter(rng.standard_normal((9500, 7)), 2)
                ctx.eigsort_costs(big, big, np.arange(600), np.arange(700), 8, np.arange(8), np.ones(8), np.arange(8), np.ones(8))
                ctx.knn1_graphs(big, big, np.arange(6), np.ones(6), np.arange(6), np.ones(6))
            finally:
                big.close()
        (gt, fin_t), (gs, fin_s) = graph(meshes[0], vectors[0]), graph(meshes[1], vectors[1])
        try:
            out = {"final": (fin_t, fin_s), "mean3": gt.mean_filter(v3, 2), "mean2": gt.mean_filter(v2, 2),
                   "costs": ctx.eigsort_costs(gt, gs, rows_t, rows_s, k, col_t, sign_t, col_s, sign_s),
                   "final_rows": gt.final_rows(rows_t), "point_rows": gs.point_rows(rows_s),
                   "knn1_graphs": ctx.knn1_graphs(gs, gt, col_s, sign_s, col_t, sign_t, return_d2=True)}
            rows = gt.rows_create(sub)
            gt.upload(0, x)
            out["gather"] = gt.rows_gather(0, rows)
            gt.rows_scatter(0, rows, vals)
            out["scattered"] = gt.download_slots(0, 1)[:, 0].copy()
            gt.rows_fill(0, rows, -2.5)
            out["filled"] = gt.download_slots(0, 1)[:, 0].copy()
        finally:
            gt.close()
            gs.close()
        return out

    def check(out):
        fin_t, fin_s = out["final"]
        for it_in, got in ((v3, out["mean3"]), (v2, out["mean2"])):  # (test_tail_kernels.check_mean_filter)
            assert np.array_equal(got, tt.orc.mean_filter_graph(W, it_in, iterations=2))
        costs, idx = out["costs"]  # (test_tail_kernels.check_es: the reference is fed what is resident on the device)
        resident = [_Resident(fin, mesh.points) for fin, mesh in zip(out["final"], meshes)]
        val, bound, widx = tt._es_reference(resident[0], resident[1], rows_t, rows_s, k, col_t, sign_t, col_s, sign_s)
        assert np.array_equal(idx, widx) and np.all(np.isfinite(costs)) and np.all(val > 0)
        assert np.all(np.abs(costs - val) <= bound)
        assert np.array_equal(out["final_rows"], fin_t[rows_t]) and np.array_equal(out["point_rows"], meshes[1].points[rows_s])
        nidx, nd2 = out["knn1_graphs"]  # (test_spectral_knn_on_device_resident_eigenvectors: the coordinates are products)
        bidx, bd2 = tt.orc.knn1_bruteforce(fin_s[:, col_s] * sign_s, fin_t[:, col_t] * sign_t)
        assert np.array_equal(nidx, bidx) and np.array_equal(nd2, bd2)
        want = x.copy()
        assert np.array_equal(out["gather"], want[sub])
        want[sub] = vals
        assert np.array_equal(out["scattered"], want)
        want[sub] = -2.5
        assert np.array_equal(out["filled"], want)

    return run, check


# ------------------------------------------------------------------------------------------------ the test
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pool_contents_change_nothing(hip, ctx, name):
    _four_runs(hip, ctx, name)
