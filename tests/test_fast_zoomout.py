"""ZoomOut on sub-samples (`zoomout_refine(samples=...)`, `fast_zoomout_correspondences`, `pf_fmap_zoomout_sampled`)
against tests/_fast_zoomout_ref.py.

CPU: the numpy loop on farthest-point samples of the renumbered and moved 700-vertex blob, 60 % of the initial map wrong,
returns the permutation at every vertex.  GPU: the refusals, the two Gram products within the summation bound, the loop
end to end against the reference, `samples=None` bit for bit as before, the public path on the device's own spectrum,
`Focusr.refine_correspondences_zoomout(n_samples=...)`.
"""
import functools

import numpy as np
import pytest

import _fast_zoomout_ref as zr
import _fmap_ref as fr
import _fps_ref as pr
from test_functional_maps import blob_pair, snapshot

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def reference_samples(q):
    p = blob_pair(700, 0, 40)
    return pr.fps(p["pt"], q)[0], pr.fps(p["ps"], q)[0]


@functools.lru_cache(maxsize=None)
def reference_run(q, k_start, k_end, step, extra):
    p = blob_pair(700, 0, 40)
    S_t, S_s = reference_samples(q)
    return zr.zoomout_sampled(p["phi_t"], p["phi_s"], p["mass_s"], fr.corrupt(p["T_true"], 0.6), S_t, S_s, k_start, k_end, step=step,
                              n_iter_at_end=extra)


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("q,step", [(100, 1), (200, 3)])
def test_reference_sampled_zoomout_recovers_the_permutation(q, step):
    p = blob_pair(700, 0, 40)
    T, C = reference_run(q, 4, 20, step, 0)
    dev = np.max(np.abs(np.abs(C) - np.eye(20)))
    print("reference, q = %d, step %d: %d vertices wrong, max ||C| - I| = %.3g" % (q, step, np.sum(T != p["T_true"]), dev))
    assert np.array_equal(T, p["T_true"])
    assert C.shape == (20, 20) and dev <= 1e-9


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
def device_samples(q):
    from pyfocusr_amd import _hip, farthest_point_sampling

    p = blob_pair(700, 0, 40)
    c = _hip.default_context()
    return farthest_point_sampling(p["pt"], q, ctx=c), farthest_point_sampling(p["ps"], q, ctx=c)


@pytest.fixture()
def handle(hip, ctx):
    p = blob_pair(700, 0, 40)
    h = hip.DeviceFunctionalMap(p["phi_t"][:, :20], p["phi_s"][:, :20], p["mass_s"], ctx=ctx)
    yield h
    h.close()


@pytest.mark.gpu
def test_device_samples_are_the_reference_samples():
    assert all(np.array_equal(a, b) for a, b in zip(device_samples(100), reference_samples(100)))


@pytest.mark.gpu
@pytest.mark.parametrize("side,bad", [("t", 700), ("t", -1), ("s", 700), ("s", -1)])
def test_set_samples_rejects_an_index_out_of_range(hip, handle, side, bad):
    p = blob_pair(700, 0, 40)
    S_t, S_s = (np.array(s) for s in reference_samples(100))
    (S_t if side == "t" else S_s)[37] = bad
    handle.set_p2p(p["T_true"])
    with pytest.raises(hip.PfError):
        handle.set_samples(S_t, S_s)
    with pytest.raises(hip.PfError):  # and no samples are left behind
        handle.zoomout_sampled(4, 20)


@pytest.mark.gpu
def test_zoomout_sampled_rejects_fewer_source_samples_than_k_end(hip, handle):
    p = blob_pair(700, 0, 40)
    S_t, S_s = reference_samples(100)
    handle.set_p2p(p["T_true"])
    handle.set_samples(S_t, S_s[:19])
    with pytest.raises(hip.PfError):
        handle.zoomout_sampled(4, 20)
    handle.set_samples(S_t, S_s[:20])  # as many samples as functions: a square fit, accepted (and of little use)
    C = handle.zoomout_sampled(4, 20)
    assert C.shape == (20, 20) and np.all(np.isfinite(C))


@pytest.mark.gpu
def test_zoomout_sampled_needs_samples_and_a_map(hip, handle):
    with pytest.raises(hip.PfError):
        handle.zoomout_sampled(4, 20)
    handle.set_samples(*reference_samples(100))
    with pytest.raises(hip.PfError):
        handle.zoomout_sampled(4, 20)


@pytest.mark.gpu
def test_degenerate_samples_are_refused(hip, handle):
    """Twenty-five copies of four vertices: A^T A has rank 4, the fifth pivot of the fit at k = 5 is zero up to rounding."""
    p = blob_pair(700, 0, 40)
    S_t, S_s = reference_samples(100)
    handle.set_p2p(p["T_true"])
    handle.set_samples(S_t, np.tile(S_s[:4], 25))
    with pytest.raises(hip.PfError, match="too few or degenerate"):
        handle.zoomout_sampled(4, 20)


@pytest.mark.gpu
@pytest.mark.parametrize("q,k", [(100, 20), (600, 40), (600, 7)])
def test_gram_products_within_the_summation_bound(hip, ctx, q, k):
    """G = A^T A and R = A^T B[Tsub] as the implementation forms them: `project` on the compact blocks with unit weights,
    G through the identity map into A itself.  q = 600 takes two blocks of rows, so the partial sums are combined."""
    p = blob_pair(700, 0, 40)
    S_t, S_s = (s[:q] for s in reference_samples(600))
    A, B = np.ascontiguousarray(p["phi_s"][S_s]), np.ascontiguousarray(p["phi_t"][S_t])
    Tsub = np.random.default_rng(q + k).integers(0, q, q)
    ones = np.ones(q)
    for ref_block, T, want in [(A, np.arange(q), zr.gram(A, k)), (B, Tsub, zr.rhs(A, B, Tsub, k))]:
        with hip.DeviceFunctionalMap(ref_block, A, ones, ctx=ctx) as h:
            h.set_p2p(T)
            got = h.project(k, k)
            assert got.tobytes() == h.project(k, k).tobytes()
            wide = h.project(40, 40)[:k, :k]
            assert got.tobytes() == wide.tobytes()  # an entry is the same sum whatever k: one product at k_end serves every round
        bound = 2.0 * (q + 2) * EPS * fr.project_abs(ref_block, A, ones, T, k, k)
        err = np.abs(got - want)
        print("gram q = %d, k = %d: max error / bound = %.3g" % (q, k, np.max(err / bound)))
        assert np.all(err <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("step,extra", [(1, 0), (1, 2), (3, 0)])
def test_sampled_zoomout_end_to_end(ctx, step, extra):
    from pyfocusr_amd import zoomout_refine

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.6)
    S_t, S_s = device_samples(100)
    T, C = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, 4, 20, step=step, n_iter_at_end=extra, samples=(S_t, S_s), ctx=ctx)
    rT, rC = zr.zoomout_sampled(p["phi_t"], p["phi_s"], p["mass_s"], T0, S_t, S_s, 4, 20, step=step, n_iter_at_end=extra)
    print("sampled zoomout, step %d, %d extra: %d vertices wrong, max |C - reference| = %.3g, reference ||C| - I| = %.3g"
          % (step, extra, np.sum(T != p["T_true"]), np.max(np.abs(C - rC)), np.max(np.abs(np.abs(rC) - np.eye(20)))))
    assert np.array_equal(rT, p["T_true"])
    assert T.dtype == np.int64 and np.array_equal(T, p["T_true"])
    assert C.shape == (20, 20) and np.max(np.abs(C - rC)) <= 1e-9


@pytest.mark.gpu
def test_sampled_zoomout_two_calls_give_the_same_bits(ctx):
    from pyfocusr_amd import zoomout_refine

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.6)
    a = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, 4, 20, samples=device_samples(100), ctx=ctx)
    b = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, 4, 20, samples=device_samples(100), ctx=ctx)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.gpu
def test_samples_none_is_the_existing_call(hip, ctx):
    from pyfocusr_amd import zoomout_refine

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.6)
    T, C = zoomout_refine(p["phi_t"], p["phi_s"], p["mass_s"], T0, 4, 20, samples=None, ctx=ctx)
    with hip.DeviceFunctionalMap(p["phi_t"][:, :20], p["phi_s"][:, :20], p["mass_s"], ctx=ctx) as h:
        h.set_p2p(T0)
        C_old = h.zoomout(4, 20, 1, 0)
        T_old = h.get_p2p()
    assert T.tobytes() == T_old.tobytes() and C.tobytes() == C_old.tobytes()


@pytest.mark.gpu
def test_fast_zoomout_correspondences_on_the_device_spectrum(ctx):
    from pyfocusr_amd import PolyMesh, fast_zoomout_correspondences

    p = blob_pair(700, 0, 40)
    T0 = fr.corrupt(p["T_true"], 0.3)
    T, C = fast_zoomout_correspondences(PolyMesh(p["pt"], p["ft"]), PolyMesh(p["ps"], p["fs"]), T0, k_start=4, k_end=20, n_samples=150,
                                        ctx=ctx)
    print("fast public path: %d vertices wrong" % np.sum(T != p["T_true"]))
    assert np.array_equal(T, p["T_true"]) and C.shape == (20, 20)


@pytest.mark.gpu
def test_focusr_refine_correspondences_zoomout_on_samples(ctx):
    from pyfocusr_amd import Focusr, PolyMesh

    p = blob_pair(700, 0, 40)
    np.random.seed(0)
    reg = Focusr(PolyMesh(p["pt"], p["ft"]), PolyMesh(p["ps"], p["fs"]), icp_register_first=False, list_features_to_calc=[],
                 n_spectral_features=3, n_extra_spectral=0, ctx=ctx)
    reg.align_maps()
    before = [snapshot(reg), snapshot(reg.graph_target), snapshot(reg.graph_source)]
    reg.refine_correspondences_zoomout(4, 16, n_samples=150)
    T = reg.zoomout_target_idx_for_each_source_pt
    assert T.shape == (700,) and T.dtype == np.int64 and T.min() >= 0 and T.max() < 700
    assert reg.functional_map.shape == (16, 16) and np.all(np.isfinite(reg.functional_map))
    after = [snapshot(reg), snapshot(reg.graph_target), snapshot(reg.graph_source)]
    for name in ("zoomout_target_idx_for_each_source_pt", "functional_map"):
        after[0].pop(name)
    assert after == before  # every attribute align_maps() had set keeps its bits
