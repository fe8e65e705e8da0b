"""Heat / wave kernel signatures and descriptor-fitted functional maps (`pyfocusr_amd.spectral_descriptors`,
`pf_descriptors.hip`) against tests/_descriptor_ref.py.

The pair: blob_mesh(700, seed) is the target, blob_mesh(900, seed) the source - one surface sampled twice, no vertex in
common, no initial map.  A source vertex's error is the distance from its own position to the target vertex it is mapped
to, in median target edge lengths; the condition is 2 edges at EVERY vertex (the numpy chain gives 0.90 after the fit and
0.74 after ZoomOut for seed 0, 1.08 and 1.13 for seed 3).

CPU: the numpy chain itself (bases from `_cotan_ref.generalized_eigs`), the regulariser's guard, the renumbered copy, the
host-made tables and the fit of the library against the reference's, the wrappers' argument checks.

GPU: `pf_spectral_descriptors` bit for bit against the numpy loop; `pf_descriptor_coefficients` within the bound of its
sums against extended precision - a term phi (m F) carries K + 2 roundings from F (p * p, times g, added), two from the
two products and one per addition over the n rows, in any order: gamma_(n + K + 4) times the sum of the terms' absolute
values, with eps (twice the unit roundoff) standing in for the unit roundoff; the public functions; the whole chain on
the device's own spectrum.
"""
import functools
import importlib

import numpy as np
import pytest

import _cotan_ref as cr
import _descriptor_ref as dr
import _fmap_ref as fr

EPS = np.finfo(np.float64).eps
K_BASIS, K_FIT, CAP = 20, 8, 2.0


@functools.lru_cache(maxsize=None)
def side(n, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    p, f = np.asarray(m.points, dtype=np.float64), np.asarray(m.faces, dtype=np.int32)
    ref = cr.assemble(p, f)
    vals, vecs, _ = cr.generalized_eigs(ref, K_BASIS)
    return dict(p=p, f=f, vals=vals, phi=np.ascontiguousarray(vecs), mass=ref["mass"])


@functools.lru_cache(maxsize=None)
def renumbered():
    """blob_mesh(700, 0) and its renumbered, moved copy (`_fmap_ref.renumbered_pair`), both with scipy bases."""
    t = side(700, 0)
    ps, fs, T_true = fr.renumbered_pair(t["p"], t["f"], seed=1)
    ref = cr.assemble(ps, fs)
    vals, vecs, _ = cr.generalized_eigs(ref, K_BASIS)
    return t, dict(p=ps, f=fs, vals=vals, phi=np.ascontiguousarray(vecs), mass=ref["mass"]), T_true


def spectra(t, s):
    return t["vals"], t["phi"], t["mass"], s["vals"], s["phi"], s["mass"]


@functools.lru_cache(maxsize=None)
def reference_chain(seed, mu=0.1):
    t, s = side(700, seed), side(900, seed)
    C = dr.functional_map(*spectra(t, s), K_FIT, mu=mu)
    T_fit = fr.convert(t["phi"], s["phi"], C)
    T_zo, _ = fr.zoomout(t["phi"], s["phi"], s["mass"], T_fit, K_FIT, K_BASIS)
    return C, T_fit, T_zo


def errors(t, s, T):
    return dr.map_errors(t["p"], t["f"], s["p"], T)


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("seed", [0, 3])
def test_reference_chain_lands_every_vertex_within_two_edges(seed):
    t, s = side(700, seed), side(900, seed)
    _, T_fit, T_zo = reference_chain(seed)
    e_fit, e_zo = errors(t, s, T_fit), errors(t, s, T_zo)
    print("seed %d: worst %.2f (median %.2f) after the fit, %.2f (%.2f) after ZoomOut" % (seed, e_fit.max(), np.median(e_fit),
                                                                                       e_zo.max(), np.median(e_zo)))
    assert e_fit.max() <= CAP and e_zo.max() <= CAP


def test_reference_fit_without_commutativity_is_useless():
    t, s = side(700, 0), side(900, 0)
    _, T_fit, _ = reference_chain(0, mu=0.0)
    assert np.mean(errors(t, s, T_fit) > CAP) > 0.5


def test_reference_fit_on_a_renumbered_copy_is_the_identity_up_to_signs():
    t, s, T_true = renumbered()
    C = dr.functional_map(*spectra(t, s), K_FIT)
    assert np.max(np.abs(np.abs(C) - np.eye(K_FIT))) <= 1e-9
    assert np.array_equal(fr.convert(t["phi"], s["phi"], C), T_true)


def test_tables_match_the_reference_and_their_definitions():
    sd = importlib.import_module("pyfocusr_amd.spectral_descriptors")  # the package's attribute of that name is the function

    vals = side(700, 0)["vals"]
    G, times = sd.hks_table(vals, n_times=37)
    rG, rtimes = dr.hks_table(vals, 37)
    assert np.array_equal(times, rtimes) and G.tobytes() == rG.tobytes()
    assert np.isclose(times[0], 4.0 * np.log(10.0) / vals[-1], rtol=1e-14) and np.isclose(times[-1], 4.0 * np.log(10.0) / vals[0], rtol=1e-14)
    assert np.all(np.diff(G, axis=1) < 0.0)  # the heat kernel decreases in t, and with it every signature
    F = dr.descriptors(side(700, 0)["phi"], G)
    assert np.all(np.diff(F[side(700, 0)["mass"] > 0], axis=1) < 0.0)
    G, en = sd.wks_table(vals, n_energies=41)
    rG, ren = dr.wks_table(vals, 41)
    assert np.array_equal(en, ren) and G.tobytes() == rG.tobytes()
    assert en[0] == np.log(vals[0]) and en[-1] == np.log(vals[-1])
    assert np.all(G >= 0.0) and np.max(np.abs(G.sum(axis=0) - 1.0)) <= K_BASIS * EPS  # K roundings of the quotients and of their sum
    # an explicit range moves the samples, not the eigenvalues
    rng = (1.5 * vals[0], 0.5 * vals[-1])
    G, times = sd.hks_table(vals, n_times=9, eig_range=rng)
    assert np.isclose(times[0], 4.0 * np.log(10.0) / rng[1], rtol=1e-14) and G.tobytes() == dr.hks_table(vals, 9, rng)[0].tobytes()
    G, en = sd.wks_table(vals, n_energies=9, eig_range=rng)
    assert en[0] == np.log(rng[0]) and en[-1] == np.log(rng[1]) and G.tobytes() == dr.wks_table(vals, 9, 7.0, rng)[0].tobytes()
    # explicit samples are taken as they are
    assert np.array_equal(sd.hks_table(vals, times=[0.5, 2.0])[0], np.exp(-vals[:, None] * np.array([0.5, 2.0])[None, :]))
    Gt, Gs = sd.descriptor_tables(vals, 1.1 * vals)
    rGt, rGs = dr.tables(vals, 1.1 * vals)
    assert Gt.shape == (K_BASIS, 200) and Gt.tobytes() == rGt.tobytes() and Gs.tobytes() == rGs.tobytes()


@pytest.mark.parametrize("bad", [0.0, -1e-3])
def test_a_non_positive_eigenvalue_raises(bad):
    from pyfocusr_amd import heat_kernel_signature, wave_kernel_signature

    t = side(700, 0)
    vals = t["vals"].copy()
    vals[0] = bad
    with pytest.raises(ValueError):
        heat_kernel_signature(vals, t["phi"])
    with pytest.raises(ValueError):
        wave_kernel_signature(vals, t["phi"])
    with pytest.raises(ValueError):
        dr.hks_table(vals)


def test_library_fit_matches_the_reference_fit():
    sd = importlib.import_module("pyfocusr_amd.spectral_descriptors")  # the package's attribute of that name is the function

    t, s = side(700, 0), side(900, 0)
    G_t, G_s = dr.tables(t["vals"], s["vals"])
    A_t, A_s = dr.coefficients(t["phi"], t["mass"], G_t, K_FIT), dr.coefficients(s["phi"], s["mass"], G_s, K_FIT)
    C = sd.fit_functional_map(A_t, A_s, t["vals"], s["vals"], 0.1)
    rC = reference_chain(0)[0]
    assert np.max(np.abs(C - rC)) <= 1e-9 * np.max(np.abs(rC))


def test_wrappers_refuse_bad_arguments():
    from pyfocusr_amd import (descriptor_coefficients, functional_map_from_descriptors, heat_kernel_signature,
                              signature_on_mesh, spectral_descriptors)

    phi, m = np.ones((10, 4)), np.ones(10)
    for args in [(None, np.ones((10, 129)), np.ones((129, 3))),  # K > 128
                 (None, phi, np.ones((4, 513))),                 # T > 512
                 (None, phi, np.ones((5, 3))),                   # G's rows are not phi's columns
                 (np.ones(3), phi, np.ones((4, 3))),             # one eigenvalue per column
                 (None, phi[:0], np.ones((4, 3))),               # no rows
                 (None, phi, np.ones((4, 0)))]:                  # no samples
        with pytest.raises(ValueError):
            spectral_descriptors(*args)
    for args in [(np.ones((10, 129)), m, np.ones((129, 3)), None), (phi, m, np.ones((4, 513)), None), (phi, m[:9], np.ones((4, 3)), None),
                 (phi, m, np.ones((4, 3)), 5), (phi, m, np.ones((4, 3)), 0), (phi, m, np.ones((3, 3)), None)]:
        with pytest.raises(ValueError):
            descriptor_coefficients(*args)
    with pytest.raises(ValueError):
        heat_kernel_signature(np.ones(3), phi)  # three eigenvalues, four columns
    t = side(700, 0)
    with pytest.raises(ValueError):
        functional_map_from_descriptors(*spectra(t, t), K_BASIS + 1)
    with pytest.raises(ValueError):
        functional_map_from_descriptors(*spectra(t, t), K_FIT, kinds=("nope",))
    with pytest.raises(ValueError):
        functional_map_from_descriptors(*spectra(t, t), K_FIT, n_samples=300)  # 600 samples in one table
    with pytest.raises(ValueError):
        signature_on_mesh(None, np.zeros((2, 2, 2)), "x")


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def random_tables(n, K, T, seed=0):
    rng = np.random.default_rng(1000 * seed + n + K + T)
    return rng.standard_normal((n, K)), rng.uniform(0.0, 1.0, (K, T)), rng.uniform(0.5, 1.5, n)


# ---- 1. the descriptors
@pytest.mark.gpu
@pytest.mark.parametrize("n,K,T", [(1, 1, 1), (513, 17, 33), (700, 128, 200), (300, 20, 512)])
def test_descriptors_are_bit_identical_to_the_numpy_loop(ctx, n, K, T):
    phi, G, _ = random_tables(n, K, T)
    F = ctx.spectral_descriptors(phi, G)
    assert F.shape == (n, T) and F.tobytes() == dr.descriptors(phi, G).tobytes()


@pytest.mark.gpu
def test_descriptors_with_zero_and_tiny_table_entries(ctx):
    phi, G, _ = random_tables(513, 17, 33, seed=1)
    G[::3] = 0.0
    G[1::3] *= np.exp(-700.0)   # just above the smallest normal number
    G[2, ::2] = 5e-324          # denormal
    phi[7] = 0.0
    F = ctx.spectral_descriptors(phi, G)
    assert F.tobytes() == dr.descriptors(phi, G).tobytes() and np.all(F[7] == 0.0)


# ---- 2. the coefficients
@pytest.mark.gpu
@pytest.mark.parametrize("K,k_out,T", [(1, 1, 1), (20, 8, 200), (128, 128, 33)])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1500])
def test_coefficients_within_the_summation_bound(ctx, n, K, k_out, T):
    phi, G, mass = random_tables(n, K, T, seed=2)
    A = ctx.descriptor_coefficients(phi, mass, G, k_out)
    again = ctx.descriptor_coefficients(phi, mass, G, k_out)
    assert A.shape == (k_out, T) and A.tobytes() == again.tobytes()  # no atomics: the same bits
    ref, ref_abs = dr.coefficients_long(phi, mass, G, k_out)
    err = np.abs(A.astype(np.longdouble) - ref)
    bound = (n + K + 4) * EPS * ref_abs
    print("coefficients n %d, K %d, k_out %d, T %d: max error / bound = %.3g" % (n, K, k_out, T, float(np.max(err / bound))))
    assert np.all(err <= bound)


@pytest.mark.gpu
def test_massless_and_empty_rows_contribute_exactly_nothing(ctx):
    n, K, k_out, T = 1500, 20, 8, 200
    phi, G, mass = random_tables(n, K, T, seed=3)
    massless, empty = np.array([0, 100, 511, 512, 1499]), np.array([5, 600, 1024, 1498])
    mass[massless] = 0.0
    phi[empty] = 0.0  # unreferenced vertices: 0 in every eigenvector
    A = ctx.descriptor_coefficients(phi, mass, G, k_out)
    phi2, mass2 = phi.copy(), mass.copy()
    phi2[massless] = 1e3 * np.random.default_rng(4).standard_normal((len(massless), K))
    mass2[empty] = 123.0
    assert ctx.descriptor_coefficients(phi2, mass2, G, k_out).tobytes() == A.tobytes()
    ref, ref_abs = dr.coefficients_long(phi, mass, G, k_out)
    assert np.all(np.abs(A.astype(np.longdouble) - ref) <= (n + K + 4) * EPS * ref_abs)


@pytest.mark.gpu
def test_library_refuses_sizes_out_of_range(hip, ctx):
    phi, G, mass = random_tables(8, 4, 3)
    bad = [lambda: ctx.spectral_descriptors(np.zeros((8, 129)), np.zeros((129, 3))),
           lambda: ctx.spectral_descriptors(phi, np.zeros((4, 513))),
           lambda: ctx.spectral_descriptors(phi[:0], G),
           lambda: ctx.descriptor_coefficients(np.zeros((8, 129)), mass, np.zeros((129, 3)), 4),
           lambda: ctx.descriptor_coefficients(phi, mass, np.zeros((4, 513)), 4),
           lambda: ctx.descriptor_coefficients(phi, mass, G, 5),
           lambda: ctx.descriptor_coefficients(phi, mass, G, 0),
           lambda: ctx.descriptor_coefficients(phi[:0], mass[:0], G, 4)]
    for call in bad:
        with pytest.raises(hip.PfError) as e:
            call()
        assert e.value.code == -1  # PF_E_ARG
    assert ctx.spectral_descriptors(phi, G).tobytes() == dr.descriptors(phi, G).tobytes()  # and the context is as it was


# ---- 3. the public functions on the scipy bases
@pytest.mark.gpu
def test_signatures_equal_the_reference_arrays(ctx):
    from pyfocusr_amd import heat_kernel_signature, spectral_descriptors, wave_kernel_signature

    t = side(700, 0)
    F, times = heat_kernel_signature(t["vals"], t["phi"], ctx=ctx)
    G, rtimes = dr.hks_table(t["vals"])
    assert F.shape == (700, 100) and np.array_equal(times, rtimes) and F.tobytes() == dr.descriptors(t["phi"], G).tobytes()
    F, en = wave_kernel_signature(t["vals"], t["phi"], ctx=ctx)
    G, ren = dr.wks_table(t["vals"])
    assert F.shape == (700, 100) and np.array_equal(en, ren) and F.tobytes() == dr.descriptors(t["phi"], G).tobytes()
    rng = (1.5 * t["vals"][0], 0.5 * t["vals"][-1])
    F, _ = heat_kernel_signature(t["vals"], t["phi"], n_times=7, eig_range=rng, ctx=ctx)
    assert F.tobytes() == dr.descriptors(t["phi"], dr.hks_table(t["vals"], 7, rng)[0]).tobytes()
    assert spectral_descriptors(t["vals"], t["phi"], G, ctx=ctx).tobytes() == dr.descriptors(t["phi"], G).tobytes()


@pytest.mark.gpu
def test_functional_map_from_descriptors_on_the_resampled_pair(ctx):
    from pyfocusr_amd import functional_map_from_descriptors, p2p_from_functional_map, zoomout_refine

    t, s = side(700, 0), side(900, 0)
    C = functional_map_from_descriptors(*spectra(t, s), K_FIT, ctx=ctx)
    rC = reference_chain(0)[0]
    print("fit: max |C - C_ref| / max |C_ref| = %.3g" % (np.max(np.abs(C - rC)) / np.max(np.abs(rC))))
    assert C.shape == (K_FIT, K_FIT) and np.max(np.abs(C - rC)) <= 1e-9 * np.max(np.abs(rC))
    T0 = p2p_from_functional_map(t["phi"], s["phi"], C, ctx=ctx)
    T, _ = zoomout_refine(t["phi"], s["phi"], s["mass"], T0, K_FIT, K_BASIS, ctx=ctx)
    e0, e1 = errors(t, s, T0), errors(t, s, T)
    print("device chain: worst %.2f after the fit, %.2f after ZoomOut" % (e0.max(), e1.max()))
    assert e0.max() <= CAP and e1.max() <= CAP


# ---- 4. the whole chain on the device's own spectrum
@pytest.mark.gpu
def test_descriptor_correspondences_on_the_resampled_pair(ctx):
    from pyfocusr_amd import PolyMesh, descriptor_correspondences

    t, s = side(700, 0), side(900, 0)
    T, C = descriptor_correspondences(PolyMesh(t["p"], t["f"]), PolyMesh(s["p"], s["f"]), k_init=K_FIT, k_end=K_BASIS, ctx=ctx)
    e = errors(t, s, T)
    print("public chain: worst %.2f, median %.2f" % (e.max(), np.median(e)))
    assert T.shape == (900,) and T.dtype == np.int64 and C.shape == (K_BASIS, K_BASIS)
    assert e.max() <= CAP


@pytest.mark.gpu
def test_descriptor_correspondences_on_a_renumbered_copy(ctx):
    from pyfocusr_amd import PolyMesh, descriptor_correspondences

    t, s, T_true = renumbered()
    T, _ = descriptor_correspondences(PolyMesh(t["p"], t["f"]), PolyMesh(s["p"], s["f"]), k_init=K_FIT, k_end=K_BASIS, ctx=ctx)
    print("renumbered copy: %d vertices wrong" % np.sum(T != T_true))
    assert np.array_equal(T, T_true)


@pytest.mark.gpu
def test_signature_on_mesh_round_trip(ctx, tmp_path):
    from pyfocusr_amd import PolyMesh, heat_kernel_signature, read_vtk_mesh, signature_on_mesh, write_vtk_mesh

    t = side(700, 0)
    mesh = PolyMesh(t["p"], t["f"])
    F, _ = heat_kernel_signature(t["vals"], t["phi"], n_times=5, ctx=ctx)
    assert signature_on_mesh(mesh, F[:, [0, 4]], "hks") == ["hks_0", "hks_1"]
    assert signature_on_mesh(mesh, F[:, 2], "hks_mid") == ["hks_mid"]
    stored = dict(mesh.point_data)
    assert np.array_equal(stored["hks_0"], F[:, 0]) and np.array_equal(stored["hks_1"], F[:, 4]) and np.array_equal(stored["hks_mid"], F[:, 2])
    path = str(tmp_path / "hks.vtk")
    write_vtk_mesh(mesh, path)
    back = dict(read_vtk_mesh(path).point_data)
    for name in ("hks_0", "hks_1", "hks_mid"):
        assert np.array_equal(back[name], stored[name])
