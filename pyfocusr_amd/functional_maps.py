"""Functional maps between two surfaces and their spectral refinement, ZoomOut, on the device.

A point map T (for every SOURCE vertex i an index T[i] into the TARGET: the direction of
`Focusr.corresponding_target_idx_for_each_source_pt`) and the two surfaces' Laplace-Beltrami bases phi_t, phi_s
(M-orthonormal, ascending: `laplace_beltrami_spectrum`) define the functional map (Ovsjanikov et al. 2012)

    C[a, b] = sum_i m_s[i] phi_s[i, a] phi_t[T[i], b]                          (k_s x k_t),

which carries the coefficients of a function on the target to those of its pull-back on the source.  Back: the rows of
Q = phi_s[:, :k_s] C are the source vertices in the target's spectral coordinates, and T[i] is the row of
phi_t[:, :k_t] nearest to Q[i].  ZoomOut (Melzi et al. 2019) alternates the two while the basis grows:

    k = k_start;  loop:  C = project(T) at (k, k);  T = convert(C);  stop if k == k_end;  k = min(k + step, k_end)

A few dozen rounds turn a noisy or partly wrong map into a sharp one.  Everything runs in `pf_fmap.hip`: the bases are
uploaded once, the projection is a gathered weighted Gram matrix reduced in a fixed order (no floating-point atomics:
two calls give the same bits), the search is exact (the library's 1-NN search for k_t <= 16, a register- and LDS-tiled
exhaustive scan up to 128 dimensions), squared distances summed left to right, the lowest index on exact ties.
At most 128 basis functions.

Fast ZoomOut (Melzi et al. 2019, 4.2.3): the same loop on a few hundred or thousand farthest-point samples of each surface
(`sampling.farthest_point_sampling`), C fitted there by least squares - exact for an exact map whatever the sampling - and
one conversion to a full-resolution point map at the end: `zoomout_refine(..., samples=(S_t, S_s))`,
`fast_zoomout_correspondences`.
"""
import numpy as np

from . import _hip
from .neighbours import k_nearest_neighbours

__all__ = ["functional_map_from_p2p", "p2p_from_functional_map", "soft_p2p_from_functional_map", "zoomout_refine", "zoomout_correspondences",
           "fast_zoomout_correspondences"]


def _handle(phi_t, phi_s, mass_s, K, ctx):
    phi_t, phi_s = np.asarray(phi_t, dtype=np.float64), np.asarray(phi_s, dtype=np.float64)
    if phi_t.ndim != 2 or phi_s.ndim != 2:
        raise ValueError("phi_t and phi_s must be (n, K) arrays")
    if not 1 <= K <= min(phi_t.shape[1], phi_s.shape[1]):
        raise ValueError("%d basis functions asked for, the bases have %d and %d" % (K, phi_t.shape[1], phi_s.shape[1]))
    if mass_s is None:
        mass_s = np.ones(phi_s.shape[0])
    return _hip.DeviceFunctionalMap(phi_t[:, :K], phi_s[:, :K], mass_s, ctx=ctx)


def functional_map_from_p2p(phi_t, phi_s, mass_s, T, k_s=None, k_t=None, ctx=None):
    """C (k_s x k_t) of the point map T; k_s, k_t default to all columns of phi_s, phi_t.  An index outside
    0 .. n_t - 1 raises `PfError`."""
    k_s = np.shape(phi_s)[1] if k_s is None else int(k_s)
    k_t = np.shape(phi_t)[1] if k_t is None else int(k_t)
    if not (1 <= k_s <= np.shape(phi_s)[1] and 1 <= k_t <= np.shape(phi_t)[1]):
        raise ValueError("k_s, k_t must lie in 1 .. the number of basis functions")
    K = max(k_s, k_t)
    pt, ps = _pad(phi_t, K), _pad(phi_s, K)
    with _handle(pt, ps, mass_s, K, ctx) as h:
        h.set_p2p(T)
        return h.project(k_s, k_t)


def _pad(phi, K):
    """The first K columns; zero columns (never read) where the basis has fewer."""
    phi = np.asarray(phi, dtype=np.float64)
    if phi.shape[1] >= K:
        return phi[:, :K]
    out = np.zeros((phi.shape[0], K))
    out[:, :phi.shape[1]] = phi
    return out


def p2p_from_functional_map(phi_t, phi_s, C, return_d2=False, ctx=None):
    """T (int64, one target index per source vertex) of the k_s x k_t functional map C: the row of phi_t[:, :k_t]
    nearest to each row of phi_s[:, :k_s] C; with `return_d2` also the squared distances."""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim != 2:
        raise ValueError("C must be a k_s x k_t matrix")
    k_s, k_t = C.shape
    if k_s > np.shape(phi_s)[1] or k_t > np.shape(phi_t)[1]:
        raise ValueError("C is %d x %d, the bases have %d and %d functions" % (k_s, k_t, np.shape(phi_s)[1], np.shape(phi_t)[1]))
    K = max(k_s, k_t)
    with _handle(_pad(phi_t, K), _pad(phi_s, K), None, K, ctx) as h:
        h.convert(k_s, k_t, C)
        return h.get_p2p(return_d2=return_d2)


def soft_p2p_from_functional_map(phi_t, phi_s, C, k, ctx=None):
    """(idx (n_s, k) int64, d2 (n_s, k)) of the k_s x k_t functional map C: for every source vertex the k rows of
    phi_t[:, :k_t] nearest to its row of Q = phi_s[:, :k_s] C, ascending by (squared distance, index)
    (`neighbours.k_nearest_neighbours`; 1 <= k <= 64, k_t <= 128).  Q is formed on the host, one term per basis
    function in ascending order.  `neighbours.inverse_distance_average(values, idx, d2)` then carries per-vertex values
    of the target - its points, point data - to the source as a smooth average; idx[:, 0] is
    `p2p_from_functional_map`'s vertex."""
    C = np.asarray(C, dtype=np.float64)
    phi_t, phi_s = np.asarray(phi_t, dtype=np.float64), np.asarray(phi_s, dtype=np.float64)
    if C.ndim != 2 or phi_t.ndim != 2 or phi_s.ndim != 2:
        raise ValueError("C must be a k_s x k_t matrix, phi_t and phi_s (n, K) arrays")
    k_s, k_t = C.shape
    if k_s > phi_s.shape[1] or k_t > phi_t.shape[1] or k_s < 1:
        raise ValueError("C is %d x %d, the bases have %d and %d functions" % (k_s, k_t, phi_s.shape[1], phi_t.shape[1]))
    Q = phi_s[:, 0:1] * C[0:1, :]
    for a in range(1, k_s):
        Q = Q + phi_s[:, a:a + 1] * C[a:a + 1, :]
    return k_nearest_neighbours(np.ascontiguousarray(phi_t[:, :k_t]), Q, k, ctx=ctx)


def zoomout_refine(phi_t, phi_s, mass_s, T0, k_start, k_end, step=1, n_iter_at_end=0, samples=None, ctx=None):
    """(T, C): the point map T0 refined by ZoomOut from k_start to k_end basis functions (`n_iter_at_end` more rounds
    at k_end), and the last functional map, k_end x k_end.  k_start == k_end is one ICP-style round.  One upload, one
    download; the loop runs in `pf_fmap_zoomout`.

    `samples=(S_t, S_s)`, vertex indices into the target and into the source (at least k_end of the source), runs the
    rounds on those rows alone (`pf_fmap_zoomout_sampled`): the first C is the projection of T0 at full resolution, every
    later one the least-squares fit (A^T A) C = A^T B[Tsub] on the samples with A = phi_s[S_s], B = phi_t[S_t], and T is
    the conversion of the last C at full resolution.  `PfError` if the samples do not determine the fit.  With `None`
    nothing changes."""
    k_start, k_end, step = int(k_start), int(k_end), int(step)
    if not (1 <= k_start <= k_end and step >= 1 and n_iter_at_end >= 0):
        raise ValueError("need 1 <= k_start <= k_end, step >= 1, n_iter_at_end >= 0")
    with _handle(phi_t, phi_s, mass_s, k_end, ctx) as h:
        h.set_p2p(T0)
        if samples is None:
            C = h.zoomout(k_start, k_end, step, int(n_iter_at_end))
        else:
            S_t, S_s = samples
            h.set_samples(S_t, S_s)
            C = h.zoomout_sampled(k_start, k_end, step, int(n_iter_at_end))
        return h.get_p2p(), C


def zoomout_correspondences(target_mesh, source_mesh, T0, k_start=4, k_end=30, step=1, n_samples=None, ctx=None):
    """(T, C): `zoomout_refine` on the two meshes' own cotangent Laplace-Beltrami bases (`laplace_beltrami_spectrum`,
    k_end functions each) and the source's lumped vertex areas (`cotangent_laplacian`).  Raises `ValueError` if the
    eigensolver delivers fewer than k_end pairs for a mesh.  The largest k_end the tests ask for is 20 (a renumbered and
    moved 700-vertex blob, 30 % of T0 wrong, to be recovered at every vertex); that test has not run on an MI355X yet
    (DESIGN.md 10b), and the solver is not tuned for more pairs here.  `n_samples`: the rounds run on that many
    farthest-point samples of each mesh (`fast_zoomout_correspondences`); None: on every vertex."""
    from .laplace_beltrami import cotangent_laplacian, laplace_beltrami_spectrum
    from .sampling import farthest_point_sampling

    samples = None
    if n_samples is not None:
        samples = tuple(farthest_point_sampling(mesh, min(int(n_samples), len(mesh.points)), ctx=ctx)
                        for mesh in (target_mesh, source_mesh))

    bases = []
    for name, mesh in (("target", target_mesh), ("source", source_mesh)):
        _, vecs = laplace_beltrami_spectrum(mesh, int(k_end), ctx=ctx)
        if vecs.shape[1] < int(k_end):
            raise ValueError("the eigensolver delivered %d of the %d Laplace-Beltrami pairs of the %s mesh: lower k_end"
                             % (vecs.shape[1], int(k_end), name))
        bases.append(vecs)
    _, mass_s = cotangent_laplacian(source_mesh, ctx=ctx)
    return zoomout_refine(bases[0], bases[1], mass_s, T0, k_start, k_end, step=step, samples=samples, ctx=ctx)


def fast_zoomout_correspondences(target_mesh, source_mesh, T0, k_start=4, k_end=30, step=1, n_samples=1000, ctx=None):
    """(T, C): `zoomout_correspondences` with the rounds on min(n_samples, n) farthest-point samples of each mesh's 3-D
    points: the work of a round no longer grows with the product of the vertex counts, only the one conversion at the end
    does.  n_samples must be at least k_end (`PfError` otherwise)."""
    if n_samples is None or int(n_samples) < 1:
        raise ValueError("n_samples must be a positive number")
    return zoomout_correspondences(target_mesh, source_mesh, T0, k_start=k_start, k_end=k_end, step=step, n_samples=int(n_samples),
                                   ctx=ctx)
