"""Heat and wave kernel signatures on a Laplace-Beltrami spectrum, and functional maps fitted to them, on the device.

Given the eigenpairs (lambda_a, phi_a) of `laplace_beltrami_spectrum`, every descriptor of the form

    F[i, t] = sum_a phi[i, a]^2 g_t(lambda_a)

is the product of the squared basis with a small table G[a, t] = g_t(lambda_a) made on the host:

    heat kernel signature (Sun et al. 2009)      g_t = exp(-lambda tau_t), tau_t geometric between 4 ln10 / lambda_hi
                                                 and 4 ln10 / lambda_lo
    wave kernel signature (Aubry et al. 2011)    g_t = exp(-(e_t - log lambda)^2 / (2 sigma^2)) / its sum over a, e_t
                                                 linear between log lambda_lo and log lambda_hi, sigma = 7 steps of e

`pf_spectral_descriptors` evaluates F (a ascending, separate multiply and add: the bits of the numpy loop), and
`pf_descriptor_coefficients` its mass-weighted coefficients A[a, t] = sum_i m_i phi[i, a] F[i, t] without storing F
(`pf_descriptors.hip`; fixed summation order, no atomics: two calls give the same bits).  At most 128 basis functions
and 512 samples per call.

The coefficients are what the first functional map of a pair is fitted to when no point map exists yet
(Ovsjanikov et al. 2012): C, k x k, in the convention of `functional_maps` (target coefficients -> those of the
pull-back on the source, A_s ~ C A_t), minimises

    ||C A_t - A_s||_F^2 + mu' sum_ab C_ab^2 ((lambda_s,a - lambda_t,b) / s)^2,

the second term being the commutativity with the two Laplacians; without it the fit is useless (the descriptors of a
smooth shape span few directions).  The objective decouples into k systems of size k x k, solved on the host.
`descriptor_correspondences` chains it all: spectra, descriptors, fit, point map, ZoomOut.

Nothing here has been timed on an MI355X yet (profiles/spectral_descriptors.md).
"""
import numpy as np

from . import _hip, vtk_functions

__all__ = ["heat_kernel_signature", "wave_kernel_signature", "spectral_descriptors", "descriptor_coefficients",
           "functional_map_from_descriptors", "descriptor_correspondences", "signature_on_mesh"]

MAX_K, MAX_T = 128, 512


def _values(eig_vals, eig_range):
    """(eigenvalues, lambda_lo, lambda_hi): all positive, the range from `eig_range` or the first and last value."""
    vals = np.asarray(eig_vals, dtype=np.float64)
    if vals.ndim != 1 or len(vals) < 1:
        raise ValueError("eig_vals must be a non-empty vector")
    if not np.all(vals > 0.0):
        raise ValueError("every eigenvalue must be positive (the null pairs are skipped by laplace_beltrami_spectrum)")
    lo, hi = (vals[0], vals[-1]) if eig_range is None else (float(eig_range[0]), float(eig_range[1]))
    if not 0.0 < lo <= hi:
        raise ValueError("need 0 < lambda_lo <= lambda_hi, got %r, %r" % (lo, hi))
    return vals, lo, hi


def hks_table(eig_vals, times=None, n_times=100, eig_range=None):
    """(G[K, T], times): G[a, t] = exp(-lambda_a tau_t)."""
    vals, lo, hi = _values(eig_vals, eig_range)
    if times is None:
        times = np.geomspace(4.0 * np.log(10.0) / hi, 4.0 * np.log(10.0) / lo, int(n_times))
    times = np.asarray(times, dtype=np.float64)
    if times.ndim != 1 or len(times) < 1:
        raise ValueError("times must be a non-empty vector")
    return np.exp(-vals[:, None] * times[None, :]), times


def wks_table(eig_vals, energies=None, n_energies=100, sigma_steps=7.0, eig_range=None):
    """(G[K, T], energies): G[a, t] = exp(-(e_t - log lambda_a)^2 / (2 sigma^2)) over its column sum,
    sigma = sigma_steps * (e_1 - e_0)."""
    vals, lo, hi = _values(eig_vals, eig_range)
    if energies is None:
        energies = np.linspace(np.log(lo), np.log(hi), int(n_energies))
    energies = np.asarray(energies, dtype=np.float64)
    if energies.ndim != 1 or len(energies) < 2:
        raise ValueError("at least two energies are needed (their spacing sets sigma)")
    sigma = float(sigma_steps) * (energies[1] - energies[0])
    if not sigma > 0.0:
        raise ValueError("sigma_steps * (e_1 - e_0) must be positive")
    G = np.exp(-(energies[None, :] - np.log(vals)[:, None]) ** 2 / (2.0 * sigma ** 2))
    return G / G.sum(axis=0)[None, :], energies


def _check_table(vecs, G):
    vecs, G = np.asarray(vecs, dtype=np.float64), np.asarray(G, dtype=np.float64)
    if vecs.ndim != 2 or G.ndim != 2 or G.shape[0] != vecs.shape[1]:
        raise ValueError("eig_vecs must be (n, K) and G (K, T)")
    n, K = vecs.shape
    if n < 1 or not 1 <= K <= MAX_K or not 1 <= G.shape[1] <= MAX_T:
        raise ValueError("n = %d, K = %d, T = %d: need n >= 1, 1 <= K <= %d, 1 <= T <= %d" % (n, K, G.shape[1], MAX_K, MAX_T))
    return vecs, G


def spectral_descriptors(eig_vals, eig_vecs, G, ctx=None):
    """F (n, T) = (eig_vecs ** 2) @ G for a caller's own table G (K, T), summed over a ascending with a separate
    multiply and add.  `eig_vals` (K,) or None: only its length is checked (G already holds what depends on it)."""
    vecs, G = _check_table(eig_vecs, G)
    if eig_vals is not None and np.shape(eig_vals) != (vecs.shape[1],):
        raise ValueError("eig_vals must have one entry per column of eig_vecs")
    return (ctx or _hip.default_context()).spectral_descriptors(vecs, G)


def descriptor_coefficients(eig_vecs, mass, G, k=None, ctx=None):
    """A (k, T): A[a, t] = sum_i mass[i] eig_vecs[i, a] F[i, t], a < k (default: every column), F as in
    `spectral_descriptors` over ALL columns of eig_vecs; F itself is never stored."""
    vecs, G = _check_table(eig_vecs, G)
    mass = np.asarray(mass, dtype=np.float64)
    if mass.shape != (vecs.shape[0],):
        raise ValueError("mass must have one entry per row of eig_vecs")
    k = vecs.shape[1] if k is None else int(k)
    if not 1 <= k <= vecs.shape[1]:
        raise ValueError("k = %d outside 1 .. %d" % (k, vecs.shape[1]))
    return (ctx or _hip.default_context()).descriptor_coefficients(vecs, mass, G, k)


def heat_kernel_signature(eig_vals, eig_vecs, times=None, n_times=100, ctx=None, eig_range=None):
    """(F[n, T], times): F[i, t] = sum_a exp(-lambda_a tau_t) phi[i, a]^2.  Default times:
    `np.geomspace(4 ln10 / lambda_hi, 4 ln10 / lambda_lo, n_times)` with lambda_lo, lambda_hi the first and last
    eigenvalue given, or `eig_range` (so that two meshes are sampled at the same scales).  A non-positive eigenvalue
    raises `ValueError`."""
    G, times = hks_table(eig_vals, times, n_times, eig_range)
    return spectral_descriptors(eig_vals, eig_vecs, G, ctx=ctx), times


def wave_kernel_signature(eig_vals, eig_vecs, energies=None, n_energies=100, sigma_steps=7.0, ctx=None, eig_range=None):
    """(F[n, T], energies): F[i, t] = sum_a g_t(lambda_a) phi[i, a]^2 with the log-normal band g_t around e_t,
    normalised over a.  Default energies: `np.linspace(log lambda_lo, log lambda_hi, n_energies)`; `eig_range` as in
    `heat_kernel_signature`."""
    G, energies = wks_table(eig_vals, energies, n_energies, sigma_steps, eig_range)
    return spectral_descriptors(eig_vals, eig_vecs, G, ctx=ctx), energies


_TABLES = {"hks": lambda vals, n, rng: hks_table(vals, None, n, rng)[0],
           "wks": lambda vals, n, rng: wks_table(vals, None, n, 7.0, rng)[0]}


def descriptor_tables(vals_t, vals_s, kinds=("hks", "wks"), n_samples=100):
    """(G_t, G_s): the tables of every kind over the two spectra's shared range, stacked along T."""
    vals_t, vals_s = np.asarray(vals_t, dtype=np.float64), np.asarray(vals_s, dtype=np.float64)
    kinds = tuple(kinds)
    if not kinds or any(kind not in _TABLES for kind in kinds):
        raise ValueError("kinds must be a non-empty selection of %r" % (sorted(_TABLES),))
    if vals_t.ndim != 1 or vals_s.ndim != 1 or len(vals_t) < 1 or len(vals_s) < 1:
        raise ValueError("vals_t and vals_s must be non-empty vectors")
    rng = (max(vals_t[0], vals_s[0]), min(vals_t[-1], vals_s[-1]))
    return tuple(np.concatenate([_TABLES[kind](vals, int(n_samples), rng) for kind in kinds], axis=1) for vals in (vals_t, vals_s))


def fit_functional_map(A_t, A_s, vals_t, vals_s, mu):
    """C (k x k) minimising ||C A_t - A_s||_F^2 + mu' sum_ab C_ab^2 ((vals_s[a] - vals_t[b]) / s)^2 with
    s = max(vals_s[k-1], vals_t[k-1]) and mu' = mu trace(A_t A_t^T) / k: one k x k system per row of C."""
    k = A_t.shape[0]
    gram = A_t @ A_t.T
    rhs = A_t @ A_s.T  # column a: the right-hand side of row a
    mu_p = float(mu) * np.trace(gram) / k
    s = max(vals_s[k - 1], vals_t[k - 1])
    C = np.empty((k, k))
    for a in range(k):
        C[a] = np.linalg.solve(gram + mu_p * np.diag(((vals_s[a] - vals_t[:k]) / s) ** 2), rhs[:, a])
    return C


def functional_map_from_descriptors(vals_t, phi_t, mass_t, vals_s, phi_s, mass_s, k, kinds=("hks", "wks"), n_samples=100,
                                    mu=0.1, ctx=None):
    """C (k x k), `functional_maps`' convention, fitted to the two surfaces' descriptors with the commutativity
    regulariser of weight `mu` (see the module's text).  The descriptors use ALL eigenpairs given, sampled over the
    range the two spectra share; the coefficients are taken on the first k basis functions of each side."""
    k = int(k)
    vals_t, vals_s = np.asarray(vals_t, dtype=np.float64), np.asarray(vals_s, dtype=np.float64)
    if not 1 <= k <= min(len(vals_t), len(vals_s)):
        raise ValueError("k = %d outside 1 .. %d" % (k, min(len(vals_t), len(vals_s))))
    if not mu >= 0.0:
        raise ValueError("mu must be >= 0")
    G_t, G_s = descriptor_tables(vals_t, vals_s, kinds, n_samples)
    A_t = descriptor_coefficients(phi_t, mass_t, G_t, k, ctx=ctx)
    A_s = descriptor_coefficients(phi_s, mass_s, G_s, k, ctx=ctx)
    return fit_functional_map(A_t, A_s, vals_t, vals_s, mu)


def descriptor_correspondences(target_mesh, source_mesh, k_init=8, k_end=20, kinds=("hks", "wks"), n_samples=100, mu=0.1,
                               step=1, n_zoomout_samples=None, ctx=None):
    """(T, C): dense correspondences of two meshes from their Laplace-Beltrami spectra alone - no initial map.  Both
    spectra (`laplace_beltrami_spectrum`, k_end pairs) and lumped masses (`cotangent_laplacian`), a functional map
    fitted to the descriptors at k_init, its point map, and `zoomout_refine` from k_init to k_end.  T[i] is the target
    vertex of source vertex i; C is the last functional map, k_end x k_end.  Raises `ValueError` if the eigensolver
    delivers fewer than k_end pairs for a mesh.  Intrinsic symmetries of the surface are not resolved: a symmetric
    shape can come back mirrored.  `n_zoomout_samples`: the refinement's rounds run on that many farthest-point
    samples of each mesh (`zoomout_refine(samples=...)`; `n_samples` is taken: it counts the descriptors' samples); None:
    on every vertex."""
    from .functional_maps import p2p_from_functional_map, zoomout_refine
    from .laplace_beltrami import cotangent_laplacian, laplace_beltrami_spectrum

    k_init, k_end = int(k_init), int(k_end)
    if not 1 <= k_init <= k_end:
        raise ValueError("need 1 <= k_init <= k_end")
    sides = []
    for name, mesh in (("target", target_mesh), ("source", source_mesh)):
        vals, vecs = laplace_beltrami_spectrum(mesh, k_end, ctx=ctx)
        if vecs.shape[1] < k_end:
            raise ValueError("the eigensolver delivered %d of the %d Laplace-Beltrami pairs of the %s mesh: lower k_end"
                             % (vecs.shape[1], k_end, name))
        _, mass = cotangent_laplacian(mesh, ctx=ctx)
        sides.append((vals, vecs, mass))
    (vals_t, phi_t, mass_t), (vals_s, phi_s, mass_s) = sides
    C0 = functional_map_from_descriptors(vals_t, phi_t, mass_t, vals_s, phi_s, mass_s, k_init, kinds=kinds, n_samples=n_samples,
                                         mu=mu, ctx=ctx)
    T0 = p2p_from_functional_map(phi_t, phi_s, C0, ctx=ctx)
    samples = None
    if n_zoomout_samples is not None:
        from .sampling import farthest_point_sampling

        samples = tuple(farthest_point_sampling(mesh, min(int(n_zoomout_samples), len(mesh.points)), ctx=ctx)
                        for mesh in (target_mesh, source_mesh))
    return zoomout_refine(phi_t, phi_s, mass_s, T0, k_init, k_end, step=step, samples=samples, ctx=ctx)


def signature_on_mesh(mesh, F, name):
    """Store descriptor columns on `mesh` as point data (`set_mesh_scalars`; written by `write_vtk_mesh` with 17 digits,
    so they read back exactly): a vector F (n,) becomes the array `name`, the columns of F (n, c) the arrays `name_0` ..
    `name_<c-1>` (select the columns worth keeping first).  Returns the names."""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim not in (1, 2):
        raise ValueError("F must be (n,) or (n, c)")
    cols = [(name, F)] if F.ndim == 1 else [("%s_%d" % (name, j), F[:, j]) for j in range(F.shape[1])]
    for col_name, values in cols:
        if vtk_functions._is_vtk_polydata(mesh):  # SetScalars would keep the last column only
            from vtk.util.numpy_support import numpy_to_vtk

            array = numpy_to_vtk(np.ascontiguousarray(values), deep=True)
            array.SetName(col_name)
            mesh.GetPointData().AddArray(array)
        else:
            vtk_functions.set_mesh_scalars(mesh, np.ascontiguousarray(values), name=col_name)
    return [col_name for col_name, _ in cols]
