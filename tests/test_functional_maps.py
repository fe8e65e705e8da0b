"""Functional maps and ZoomOut (`pyfocusr_amd.functional_maps`, `pf_fmap.hip`) against tests/_fmap_ref.py.

CPU: the numpy reference against closed forms, and its ZoomOut loop on the renumbered and moved 700-vertex blob with 60 %
of the initial map wrong (bases from `_cotan_ref.assemble` and scipy's shift-invert `eigsh`): it must return the
permutation at every vertex.  That pins the yardstick and the inputs of the device tests.

GPU: the wide search bit for bit against the brute force; the projection within the gamma_n bound of any summation
order; every converted index optimal up to the rounding of Q; ZoomOut end to end with exact recovery; the public path on
the device's own spectrum; `Focusr.refine_correspondences_zoomout`.
"""
import functools

import numpy as np
import pytest

import _cotan_ref as cr
import _fmap_ref as fr

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def blob_pair(n, seed, K):
    """Target: blob_mesh(n, seed); source: the same surface renumbered (default_rng(1)) and moved; bases from scipy."""
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    pt, ft = np.asarray(m.points, dtype=np.float64), np.asarray(m.faces, dtype=np.int32)
    ps, fs, T_true = fr.renumbered_pair(pt, ft, seed=1)
    out = dict(pt=pt, ft=ft, ps=ps, fs=fs, T_true=T_true)
    for side, (p, f) in (("t", (pt, ft)), ("s", (ps, fs))):
        ref = cr.assemble(p, f)
        _, vecs, _ = cr.generalized_eigs(ref, K)
        out["phi_" + side], out["mass_" + side] = np.ascontiguousarray(vecs), ref["mass"]
    return out


# ------------------------------------------------------------------------------------------------------ CPU
def test_reference_identity_map_gives_identity():
    p = blob_pair(700, 0, 40)
    C = fr.project(p["phi_t"], p["phi_t"], p["mass_t"], np.arange(700), 20, 20)
    assert np.max(np.abs(C - np.eye(20))) <= 1e-12


def test_reference_identity_functional_map_returns_the_permutation():
    p = blob_pair(700, 0, 40)
    phi_s = p["phi_t"][p["T_true"]]  # a permuted copy: source vertex i is target vertex T_true[i]
    T, d2 = fr.convert(p["phi_t"], phi_s, np.eye(20), return_d2=True)
    assert np.array_equal(T, p["T_true"]) and np.all(d2 == 0.0)


def test_reference_brute_force_takes_the_lowest_index_on_ties():
    ref = np.array([[1.0, 2.0], [0.0, 0.0], [1.0, 2.0], [0.0, 0.0]])
    idx, d2 = fr.brute_force_nn(ref, np.array([[0.0, 0.0], [1.0, 2.0], [0.5, 1.0]]))
    assert idx.tolist() == [1, 0, 0] and d2.tolist() == [0.0, 0.0, 1.25]


def test_reference_zoomout_recovers_the_permutation():
    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.6)
    assert np.mean(T0 == p["T_true"]) < 0.45
    T, C = fr.zoomout(p["phi_t"], p["phi_s"], p["mass_s"], T0, 4, 20)
    assert np.array_equal(T, p["T_true"])
    assert C.shape == (20, 20) and np.max(np.abs(np.abs(C) - np.eye(20))) <= 1e-9


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


# ---- 1. the wide search
N_REF, N_QRY = 2500, 777


def cloud(d, n_ref=N_REF, n_qry=N_QRY):
    rng = np.random.default_rng(100 + d)
    return rng.standard_normal((n_ref, d)), rng.standard_normal((n_qry, d))


def check_wide(ctx, ref, qry):
    idx, d2 = ctx.knn1_wide(ref, qry, return_d2=True)
    ridx, rd2 = fr.brute_force_nn(ref, qry)
    assert idx.dtype == np.int64 and np.array_equal(idx, ridx)
    assert np.array_equal(d2, rd2)  # the same bits
    return idx, d2


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3, 16, 17, 33, 64, 127, 128])
def test_wide_search_is_bit_identical_to_brute_force(ctx, d):
    ref, qry = cloud(d)
    idx, d2 = check_wide(ctx, ref, qry)
    if d in (3, 16):
        kidx, kd2 = ctx.knn1(ref, qry, return_d2=True)
        assert np.array_equal(idx, kidx) and np.array_equal(d2, kd2)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [20, 128])
def test_wide_search_single_reference_and_single_query(ctx, d):
    ref, qry = cloud(d)
    check_wide(ctx, ref[:1], qry)
    check_wide(ctx, ref, qry[:1])
    check_wide(ctx, ref[:1], qry[:1])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [5, 33])
def test_wide_search_duplicates_give_the_lowest_index(ctx, d):
    ref, qry = cloud(d)
    ref[400] = ref[10]
    ref[2000] = ref[10]
    qry[[0, 300, 776]] = ref[10]
    qry[5] = ref[2499]
    idx, d2 = check_wide(ctx, ref, qry)
    assert idx[[0, 300, 776]].tolist() == [10, 10, 10] and np.all(d2[[0, 300, 776, 5]] == 0.0) and idx[5] == 2499


@pytest.mark.gpu
def test_wide_search_refuses_d_out_of_range(hip, ctx):
    for d in (0, 129):
        with pytest.raises(hip.PfError):
            ctx.knn1_wide(np.zeros((4, d)), np.zeros((3, d)))


# ---- 2. the projection
N_S, N_T, K_MAX = 5000, 3100, 128


@functools.lru_cache(maxsize=None)
def random_problem():
    rng = np.random.default_rng(7)
    return dict(phi_t=rng.standard_normal((N_T, K_MAX)), phi_s=rng.standard_normal((N_S, K_MAX)),
                mass=rng.uniform(0.5, 1.5, N_S), T=rng.integers(0, N_T, N_S))


@pytest.fixture(scope="module")
def random_handle(hip, ctx):
    r = random_problem()
    h = hip.DeviceFunctionalMap(r["phi_t"], r["phi_s"], r["mass"], ctx=ctx)
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k_s,k_t", [(1, 1), (4, 4), (20, 20), (17, 33), (128, 128)])
def test_projection_within_the_summation_bound(random_handle, k_s, k_t):
    r, h = random_problem(), random_handle
    h.set_p2p(r["T"])
    C = h.project(k_s, k_t)
    again = h.project(k_s, k_t)
    assert C.shape == (k_s, k_t) and C.tobytes() == again.tobytes()  # no atomics: the same bits
    ref = fr.project(r["phi_t"], r["phi_s"], r["mass"], r["T"], k_s, k_t)
    # gamma_n for the n_s products (two roundings each) and n_s - 1 additions in ANY order, doubled for the two sides
    bound = 2.0 * (N_S + 2) * EPS * fr.project_abs(r["phi_t"], r["phi_s"], r["mass"], r["T"], k_s, k_t)
    err = np.abs(C - ref)
    print("projection %d x %d: max error / bound = %.3g" % (k_s, k_t, np.max(err / bound)))
    assert np.all(err <= bound)


@pytest.mark.gpu
def test_public_projection_matches_the_handle(ctx, random_handle):
    from pyfocusr_amd import functional_map_from_p2p

    r = random_problem()
    random_handle.set_p2p(r["T"])
    C = functional_map_from_p2p(r["phi_t"], r["phi_s"], r["mass"], r["T"], k_s=17, k_t=33, ctx=ctx)
    assert C.tobytes() == random_handle.project(17, 33).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [N_T, -1])
def test_point_map_out_of_range_is_refused(hip, random_handle, bad):
    T = random_problem()["T"].copy()
    T[1234] = bad
    with pytest.raises(hip.PfError):
        random_handle.set_p2p(T)
    with pytest.raises(hip.PfError):  # and no map is left behind
        random_handle.project(4, 4)


# ---- 3. the conversion
@pytest.mark.gpu
@pytest.mark.parametrize("k_t", [24, 12])
def test_converted_indices_are_optimal_up_to_the_rounding_of_q(random_handle, k_t):
    r, h, k_s = random_problem(), random_handle, 24
    C = np.random.default_rng(9).standard_normal((k_s, k_t))
    h.convert(k_s, k_t, C)
    T, d2 = h.get_p2p(return_d2=True)
    assert T.shape == (N_S,) and T.min() >= 0 and T.max() < N_T
    Q = r["phi_s"][:, :k_s] @ C
    ref_t = r["phi_t"][:, :k_t]
    _, best = fr.brute_force_nn(ref_t, Q)
    got = fr.row_d2(ref_t[T], Q)
    delta = 2.0 * (k_s + 2) * EPS * np.linalg.norm(np.abs(r["phi_s"][:, :k_s]) @ np.abs(C), axis=1)
    slack = np.sqrt(best) * (1.0 + (k_t + 2) * EPS) + 2.0 * delta - np.sqrt(got)
    print("conversion k_t = %d: %d of %d indices differ from numpy's, least slack %.3g" % (k_t, np.sum(got != best), N_S, slack.min()))
    assert np.all(slack >= 0.0)  # every row
    # the distance the device reports is to ITS Q: the two Q differ by at most delta in norm, the sums by their rounding
    assert np.all(np.abs(np.sqrt(d2) - np.sqrt(got)) <= 2.0 * delta + (k_t + 2) * EPS * np.sqrt(got))


@pytest.mark.gpu
def test_resident_and_explicit_functional_map_convert_alike(random_handle):
    r, h = random_problem(), random_handle
    for k in (24, 12):
        h.set_p2p(r["T"])
        C = h.project(24, k)
        h.convert(24, k)
        T_resident = h.get_p2p()
        h.set_p2p(r["T"])
        h.convert(24, k, C)
        assert np.array_equal(T_resident, h.get_p2p())


@pytest.mark.gpu
def test_public_conversion_matches_the_reference_on_a_permuted_copy(ctx):
    from pyfocusr_amd import p2p_from_functional_map

    p = blob_pair(700, 0, 40)
    phi_s = np.ascontiguousarray(p["phi_t"][p["T_true"]])
    for k in (12, 40):
        T, d2 = p2p_from_functional_map(p["phi_t"], phi_s, np.eye(k), return_d2=True, ctx=ctx)
        assert np.array_equal(T, p["T_true"]) and np.all(d2 == 0.0)


# ---- 4. ZoomOut end to end
@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,fraction,k_start,k_end", [(700, 0, 0.6, 4, 20), (700, 0, 0.6, 6, 40), (1500, 3, 0.3, 6, 40)])
def test_zoomout_recovers_the_permutation(ctx, n, seed, fraction, k_start, k_end):
    from pyfocusr_amd import zoomout_refine

    p = blob_pair(n, seed, 40)
    T0 = fr.corrupt(p["T_true"], fraction)
    T, C = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, k_start, k_end, ctx=ctx)
    dev = np.max(np.abs(np.abs(C) - np.eye(k_end)))
    print("zoomout %d, %d %% wrong, %d -> %d: %d vertices wrong, max ||C| - I| = %.3g" % (n, 100 * fraction, k_start, k_end,
                                                                                    np.sum(T != p["T_true"]), dev))
    assert T.dtype == np.int64 and np.array_equal(T, p["T_true"])
    assert C.shape == (k_end, k_end) and dev <= 1e-9


@pytest.mark.gpu
def test_zoomout_follows_the_reference_loop(ctx):
    """Step 3, one repeat at the end, and k_start == k_end (one ICP-style round): the same maps as the numpy loop."""
    from pyfocusr_amd import zoomout_refine

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.3)
    for k_start, k_end, step, extra in [(5, 18, 3, 1), (20, 20, 1, 0)]:
        T, C = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, k_start, k_end, step=step, n_iter_at_end=extra, ctx=ctx)
        rT, rC = fr.zoomout(p["phi_t"], p["phi_s"], p["mass_s"], T0, k_start, k_end, step=step, n_iter_at_end=extra)
        assert np.array_equal(T, rT)
        # the last projection is of the map BEFORE the last conversion; with equal maps all along it obeys test 2's bound
        assert np.all(np.abs(C - rC) <= 2.0 * 702 * EPS * np.abs(p["phi_s"][:, :k_end] * p["mass_s"][:, None]).sum(0)[:, None]
                      * np.abs(p["phi_t"][:, :k_end]).max(0)[None, :])


# ---- 5. the public path on the device's own spectrum
K_PUBLIC = 20  # the k_end asked of laplace_beltrami_spectrum


@pytest.mark.gpu
def test_zoomout_correspondences_on_the_device_spectrum(ctx):
    from pyfocusr_amd import PolyMesh, zoomout_correspondences

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.3)
    T, C = zoomout_correspondences(PolyMesh(p["pt"], p["ft"]), PolyMesh(p["ps"], p["fs"]), T0, k_start=4, k_end=K_PUBLIC, ctx=ctx)
    print("public path: %d vertices wrong" % np.sum(T != p["T_true"]))
    assert np.array_equal(T, p["T_true"]) and C.shape == (K_PUBLIC, K_PUBLIC)


# ---- 6. Focusr
def snapshot(obj):
    out = {}
    for name, value in list(vars(obj).items()):
        if isinstance(value, np.ndarray):
            out[name] = (value.dtype, value.shape, value.tobytes())
        elif isinstance(value, dict):
            out[name] = {k: (v.dtype, v.shape, v.tobytes()) if isinstance(v, np.ndarray) else repr(v) for k, v in value.items()}
        elif isinstance(value, (int, float, str, bool, tuple, type(None))):
            out[name] = value
    return out


@pytest.mark.gpu
def test_focusr_refine_correspondences_zoomout(ctx):
    from pyfocusr_amd import Focusr, PolyMesh

    p = blob_pair(700, 0, 40)
    np.random.seed(0)
    reg = Focusr(PolyMesh(p["pt"], p["ft"]), PolyMesh(p["ps"], p["fs"]), icp_register_first=False, list_features_to_calc=[],
                 n_spectral_features=3, n_extra_spectral=0, ctx=ctx)
    assert not hasattr(reg, "functional_map")
    reg.align_maps()
    before = [snapshot(reg), snapshot(reg.graph_target), snapshot(reg.graph_source)]
    assert before[0]["corresponding_target_idx_for_each_source_pt"][1] == (700,)
    reg.refine_correspondences_zoomout(4, 16)
    T = reg.zoomout_target_idx_for_each_source_pt
    assert T.shape == (700,) and T.dtype == np.int64 and T.min() >= 0 and T.max() < 700
    assert reg.functional_map.shape == (16, 16) and np.all(np.isfinite(reg.functional_map))
    after = [snapshot(reg), snapshot(reg.graph_target), snapshot(reg.graph_source)]
    for name in ("zoomout_target_idx_for_each_source_pt", "functional_map"):
        after[0].pop(name)
    assert after == before  # every attribute align_maps() had set keeps its bits
