"""Cotangent Laplace-Beltrami operator of a triangle mesh, assembled and solved on the device.

The reference's Laplacian weighs an edge by the inverse of its length: it measures the triangulation, not the surface
(its spectrum ignores scale and changes with the meshing density).  The cotangent operator with a lumped mass matrix is
the FEM discretisation of the surface's Laplace-Beltrami operator (Pinkall & Polthier 1993; Meyer et al. 2003):

    w_ij = 1/2 sum of cot(angle opposite (i, j)) over the faces that contain the edge,  d_i = sum_j w_ij,
    m_i  = 1/3 sum of the areas of the faces at i,                                       L = M^-1 (D - W).

Its eigenvalues scale with 1 / length^2 and converge under refinement; its eigenfunctions are what spectral
coordinates, shape-DNA and heat / wave kernel descriptors are defined on; applied to the vertex positions it gives the
mean-curvature normal.  `pf_graph_build_cotan` assembles it from a resident mesh without floating-point atomics (two
builds give the same bits); the spectrum is computed on the symmetric S = M^-1/2 (D - W) M^-1/2 by the filtered Krylov
solver behind `recursive_eig`, with sqrt(m) on every connected component locked as its null vector.

`Graph(mesh, laplacian="cotangent")` and `Focusr(..., laplacian="cotangent")` use the same operator.  Vertices that no
face references have mass 0, an empty row, and 0 in every eigenvector and normal.  Triangle meshes only; a face of zero
area raises `PfError` (PF_E_DEGENERATE).
"""
import numpy as np
from scipy import sparse

from . import _hip
from .vtk_functions import mesh_arrays

__all__ = ["cotangent_laplacian", "laplace_beltrami_spectrum", "mean_curvature_normals", "mean_curvature"]


def _device(mesh, ctx):
    points, faces = mesh_arrays(mesh)
    return _hip.DeviceLaplacian(points, faces, ctx=ctx, cotangent=True)


def cotangent_laplacian(mesh, ctx=None):
    """(L_c, mass): L_c = D - W as a scipy CSR matrix (symmetric, rows summing to 0, off-diagonals -w_ij - positive at
    obtuse angles) and the lumped barycentric vertex areas m; the generalised problem is L_c phi = lambda diag(m) phi."""
    with _device(mesh, ctx) as dev:
        h, c = dev.download(), dev.cotan_download()
        n = dev.n
    W = sparse.csr_matrix((c["w"], h["colidx"], h["rowptr"]), shape=(n, n))
    L = sparse.csr_matrix(sparse.diags(c["diag"]) - W)
    L.sort_indices()
    return L, c["mass"]


def laplace_beltrami_spectrum(mesh, k, ctx=None):
    """The k smallest non-null eigenpairs of L_c phi = lambda M phi, ascending: (eig_vals[k], eig_vecs[n, k]) with
    eig_vecs^T M eig_vecs = I and `Graph`'s sign convention (the largest-|entry| of a column, lowest index on ties, is
    positive).  One null pair per connected component and per unreferenced vertex is skipped; fewer than k columns come
    back only when the mesh has fewer non-null pairs."""
    from .graph import _cotan_solver_kw, _cotan_vectors, _device_eigs

    with _device(mesh, ctx) as dev:
        k = int(k)
        n_null = dev.n_components + dev.n_isolated
        vals, vecs, _ = _device_eigs(dev, k=k + n_null, n_k_needed=k, k_buffer=1, minmax=False, verbose=False,
                                     **_cotan_solver_kw(dev, k))
        vecs = _cotan_vectors(dev.mass, vecs, unit=False)
    return vals[:k], np.ascontiguousarray(vecs[:, :k])


def mean_curvature_normals(mesh, ctx=None):
    """(n, 3): M^-1 (D - W) applied to the vertex positions (`pf_cotan_apply`) - the discrete mean-curvature normal
    of length 2 H; with this sign (D - W, positive semi-definite) it points outward where the surface is convex; 0 on
    unreferenced vertices."""
    with _device(mesh, ctx) as dev:
        points, _ = mesh_arrays(mesh)
        return dev.cotan_apply(np.asarray(points, dtype=np.float64))


def mean_curvature(mesh, ctx=None):
    """(n,): the unsigned mean curvature H = 1/2 |mean_curvature_normals|."""
    return 0.5 * np.linalg.norm(mean_curvature_normals(mesh, ctx=ctx), axis=1)
