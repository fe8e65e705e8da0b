"""Statistical shape models on the MI355X: generalized Procrustes alignment and the principal modes of a population.

Once every subject's surface is expressed on one template's vertices (`population_from_template`: one `Focusr` run per
subject, the template as the source), the population `shapes (S, n, 3)` has a mean shape and modes of variation:

* `generalized_procrustes` removes position, orientation and (optionally) size: the aligned shapes, their mean, the
  similarity transform of every shape and the history of the mean's change;
* `build_shape_model` chains the alignment and a `ShapeModel`: `mean`, `modes (K, n, 3)` orthonormal in the weighted inner
  product `<a, b> = sum_i w_i a_i . b_i`, `eigenvalues`, the training `scores (S, K)`; `project`, `reconstruct`, `sample`,
  `compactness`, `mode_on_mesh`.

The population stays on the device (`_hip.DeviceShapes`, `pf_shapes_*`): the device does the passes over the S x n points
(centroids, cross-covariances, transforms, the mean, the S x S Gram matrix, the modes as combinations of the shapes, the
scores), every sum in a fixed order, so two calls give the same bits.  Every small dense step is numpy on the host: one
3 x 3 SVD per shape and iteration (Kabsch), one S x S `eigh`.  `weights` are per-point weights, typically the vertex areas
of the template (`discrete_curvatures(template).area`).  The exact definitions are in include/pyfocusr_hip.h.

This is a capability of its own: nothing in `Focusr.align_maps()` calls it.
"""
import numpy as np

from . import _hip
from . import vtk_functions

__all__ = ["generalized_procrustes", "ShapeModel", "build_shape_model", "population_from_template", "ProcrustesResult"]

EIGENVALUE_FLOOR = 1e-10  # modes whose eigenvalue is below this fraction of the largest are dropped: rounding noise of the Gram matrix


class ProcrustesResult(object):
    """What `generalized_procrustes` returns: `aligned (S, n, 3)`, `mean (n, 3)`, `transforms (S, 4, 4)` (aligned point =
    A x + b with [[A, b], [0, 1]] composed over every step), `history` (the `change` of every iteration), `n_iter`,
    `converged`, `weights`, `weight_sum`."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __iter__(self):  # aligned, mean, transforms, history = generalized_procrustes(...)
        return iter((self.aligned, self.mean, self.transforms, self.history))


def kabsch_step(H, q, rho, scaling, reflection):
    """(R (3, 3), scale) of one shape from its alignment sums: y = scale (x R) with x a row vector brings the shape onto
    the reference.  H[a][b] = sum w x_a r_b, q = sum w |x|^2, rho the weighted RMS size of the reference."""
    U, sv, Vt = np.linalg.svd(H)
    d = np.ones(3)
    if not reflection and np.linalg.det(U @ Vt) < 0.0:
        d[2] = -1.0
    R = (U * d) @ Vt
    if not scaling:
        return R, 1.0
    trace = (sv[0] * d[0] + sv[1] * d[1]) + sv[2] * d[2]
    return R, trace / (rho * q)


def _step_matrices(R, scale):
    """(S, 4, 4) of y = scale (x R): A = scale R^T."""
    M = np.zeros((len(R), 4, 4))
    M[:, :3, :3] = scale[:, None, None] * np.transpose(R, (0, 2, 1))
    M[:, 3, 3] = 1.0
    return M


def _check_options(max_iter, tol):
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and not negative")


def procrustes_loop(dev, scaling, reflection, max_iter, tol):
    """The alignment itself on a `_hip.DeviceShapes`: (mean, transforms, history, converged)."""
    S, W = dev.S, dev.weight_sum
    eye = np.tile(np.eye(3), (S, 1, 1))
    c = dev.center()
    M = np.tile(np.eye(4), (S, 1, 1))
    M[:, :3, 3] = -c
    if scaling:
        _, q, _ = dev.align_sums()
        if np.any(q == 0.0):
            raise ValueError("shape %d has no extent: it cannot be brought to unit size" % int(np.argmax(q == 0.0)))
        k = 1.0 / np.sqrt(q / W)
        dev.transform(eye, k)
        M = _step_matrices(eye, k) @ M
    mean, _ = dev.mean(0, 1)
    history, converged = [], False
    for _ in range(int(max_iter)):
        H, q, rho2 = dev.align_sums()
        rho = np.sqrt(rho2 / W)
        R, scale = np.empty((S, 3, 3)), np.empty(S)
        for s in range(S):
            R[s], scale[s] = kabsch_step(H[s], q[s], rho, scaling, reflection)
        dev.transform(R, scale)
        M = _step_matrices(R, scale) @ M
        mean, change = dev.mean()
        history.append(change)
        if np.sqrt(change / W) < tol * rho:
            converged = True
            break
    return mean, M, np.array(history), converged


def _aligned_device(shapes, weights, scaling, reflection, max_iter, tol, ctx):
    """(ProcrustesResult, the open `DeviceShapes` that holds the aligned population with the mean as its reference)."""
    _check_options(max_iter, tol)
    X, w = _hip.check_population(shapes, weights)
    dev = _hip.DeviceShapes(X, w, ctx=ctx)
    try:
        mean, M, history, converged = procrustes_loop(dev, bool(scaling), bool(reflection), max_iter, tol)
        return ProcrustesResult(aligned=dev.download(), mean=mean, transforms=M, history=history, n_iter=len(history),
                                converged=converged, weights=w, weight_sum=dev.weight_sum, scaling=bool(scaling),
                                reflection=bool(reflection)), dev
    except Exception:
        dev.close()
        raise


def generalized_procrustes(shapes, weights=None, scaling=True, reflection=False, max_iter=100, tol=1e-10, ctx=None):
    """Generalized Procrustes alignment of `shapes (S, n, 3)` float64 (or a list of (n, 3) arrays) in correspondence.

    Every shape is centred on its weighted centroid and, with `scaling`, brought to unit weighted RMS size; shape 0 is
    the first reference.  Each iteration rotates (and scales) every shape onto the reference by Kabsch's SVD -
    reflections only with `reflection=True` - and makes the mean the new reference, until the weighted RMS change of the
    mean falls below `tol` times the reference's RMS size, or `max_iter` iterations.  Returns a `ProcrustesResult`, which
    unpacks as (aligned, mean, transforms, history)."""
    result, dev = _aligned_device(shapes, weights, scaling, reflection, max_iter, tol, ctx)
    dev.close()
    return result


def principal_modes(dev, n_modes=None):
    """The Gram PCA of a `_hip.DeviceShapes` whose reference is the population's mean:
    (eigenvalues (K,), all_eigenvalues (S,), coeff (K, S), modes (K, n, 3), scores (S, K))."""
    S = dev.S
    G = dev.gram()
    lam, U = np.linalg.eigh(G / (S - 1))
    lam, U = lam[::-1], U[:, ::-1]
    keep = int(np.count_nonzero(lam[:S - 1] > EIGENVALUE_FLOOR * lam[0])) if lam[0] > 0.0 else 0
    if n_modes is not None:
        keep = min(keep, int(n_modes))
    if keep < 1:
        raise ValueError("the aligned population has no variation: no mode to keep")
    coeff = np.empty((keep, S))
    for k in range(keep):
        u = U[:, k]
        if u[np.argmax(np.abs(u))] < 0.0:  # the component of largest magnitude (the lowest index on ties) is positive
            u = -u
        coeff[k] = u / np.sqrt((S - 1) * lam[k])
    modes = dev.combine(coeff)
    return lam[:keep].copy(), lam.copy(), coeff, modes, dev.scores(modes)


class ShapeModel(object):
    """A point distribution model: `mean (n, 3)`, `modes (K, n, 3)`, `eigenvalues (K,)` (descending variances),
    `scores (S, K)` of the training shapes, `explained_variance_ratio (K,)`, `weights` (n,) or None, `transforms
    (S, 4, 4)` of the alignment.  A shape is `mean + sum_k b_k modes[k]`; the modes are orthonormal in the weighted
    inner product, so `b_k = sum_i w_i (x_i - mean_i) . modes[k]_i`."""

    def __init__(self, mean, modes, eigenvalues, scores, explained_variance_ratio, weights=None, transforms=None,
                 scaling=True, reflection=False, history=None):
        self.mean, self.modes, self.eigenvalues, self.scores = mean, modes, eigenvalues, scores
        self.explained_variance_ratio, self.weights, self.transforms = explained_variance_ratio, weights, transforms
        self.scaling, self.reflection, self.history = scaling, reflection, history

    @property
    def n_modes(self):
        return len(self.eigenvalues)

    def project(self, points, align=True, ctx=None):
        """The scores (K,) of a new shape `points (n, 3)` in correspondence with the mean; with `align` it is first
        centred and brought onto the mean by the alignment's own Kabsch step."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.shape != self.mean.shape:
            raise ValueError("points must be (%d, 3): in correspondence with the mean" % len(self.mean))
        with _hip.DeviceShapes(pts[None], self.weights, ctx=ctx) as dev:
            dev.set_reference(self.mean)
            if align:
                dev.center()
                H, q, rho2 = dev.align_sums()
                if self.scaling and q[0] == 0.0:
                    raise ValueError("the shape has no extent")
                R, scale = kabsch_step(H[0], q[0], np.sqrt(rho2 / dev.weight_sum), self.scaling, self.reflection)
                dev.transform(R[None], np.array([scale]))
            return dev.scores(self.modes)[0]

    def reconstruct(self, b):
        """mean + sum_k b_k modes[k] for scores b (K,) or (m, K) (fewer than K scores use the leading modes)."""
        b = np.asarray(b, dtype=np.float64)
        if b.ndim not in (1, 2) or b.shape[-1] > self.n_modes:
            raise ValueError("scores must be (k,) or (m, k) with k <= %d modes" % self.n_modes)
        return self.mean + np.tensordot(b, self.modes[:b.shape[-1]], axes=([-1], [0]))

    def sample(self, rng=None, n=1):
        """(n, n_points, 3) shapes with scores b_k ~ N(0, eigenvalue_k)."""
        rng = np.random.default_rng(rng)
        return self.reconstruct(rng.standard_normal((int(n), self.n_modes)) * np.sqrt(self.eigenvalues))

    def compactness(self):
        """The cumulative explained variance ratio (K,)."""
        return np.cumsum(self.explained_variance_ratio)

    def mode_on_mesh(self, mesh, k=0, sigma=3.0):
        """A copy of `mesh` (the template: n points) with its points at mean + sigma sqrt(eigenvalue_k) modes[k]."""
        if not 0 <= int(k) < self.n_modes:
            raise ValueError("mode %d out of range (0 .. %d)" % (k, self.n_modes - 1))
        pts, _ = vtk_functions.mesh_arrays(mesh)
        if len(pts) != len(self.mean):
            raise ValueError("the mesh has %d points, the model %d" % (len(pts), len(self.mean)))
        new_points = self.mean + (float(sigma) * np.sqrt(self.eigenvalues[k])) * self.modes[k]
        if isinstance(mesh, vtk_functions.PolyMesh):
            return vtk_functions.PolyMesh(new_points, mesh.faces.copy(), list(mesh.point_data))
        out = vtk_functions.vtk_deep_copy(mesh)
        points = out.GetPoints()
        for i in range(len(new_points)):
            points.SetPoint(i, new_points[i])
        return out


def _check_n_modes(n_modes, S):
    if n_modes is not None and not 1 <= int(n_modes) <= S - 1:
        raise ValueError("n_modes = %s out of range: %d shapes have at most %d modes" % (n_modes, S, S - 1))


def model_from_parts(mean, parts, weights, transforms, scaling, reflection, history):
    lam, all_lam, _, modes, scores = parts
    total = float(np.sum(all_lam[all_lam > 0.0]))
    return ShapeModel(mean, modes, lam, scores, lam / total, weights=weights, transforms=transforms, scaling=scaling,
                      reflection=reflection, history=history)


def build_shape_model(shapes, weights=None, n_modes=None, scaling=True, reflection=False, max_iter=100, tol=1e-10, ctx=None):
    """`generalized_procrustes` with the same options, then the principal modes of the aligned population (at
    most `n_modes`, at most S - 1): a `ShapeModel`.  The population goes to the device once."""
    X, w = _hip.check_population(shapes, weights)
    if X.shape[0] < 2:
        raise ValueError("a shape model needs at least two shapes")
    _check_n_modes(n_modes, X.shape[0])
    gpa, dev = _aligned_device(X, w, scaling, reflection, max_iter, tol, ctx)
    with dev:
        parts = principal_modes(dev, n_modes)
    return model_from_parts(gpa.mean, parts, w, gpa.transforms, gpa.scaling, gpa.reflection, gpa.history)


_POSITIONS = {"weighted": ("weighted_avg_transformed_points",), "surface": ("surface_transformed_points",),
              "nearest": ("nearest_neighbour_transformed_points", "nearest_neighbor_transformed_points")}


def population_from_template(template, subjects, positions="weighted", **focusr_kwargs):
    """(S, n_template, 3): where every vertex of `template` lies on each of the `subjects`.  For each subject one
    `Focusr(vtk_mesh_target=subject, vtk_mesh_source=template, **focusr_kwargs).align_maps()` (the subject is the target, the template the source); the
    row is its `weighted_avg_transformed_points` ("weighted"), `surface_transformed_points` ("surface") or
    `nearest_neighbour_transformed_points` ("nearest")."""
    from . import focusr as focusr_module

    if positions not in _POSITIONS:
        raise ValueError("positions must be \"weighted\", \"surface\" or \"nearest\", not %r" % (positions,))
    subjects = list(subjects)
    if len(subjects) == 0:
        raise ValueError("a population needs at least one subject")
    kwargs = dict(focusr_kwargs)
    if positions == "surface":
        kwargs.setdefault("return_surface_final_points", True)
    rows = []
    for subject in subjects:
        reg = focusr_module.Focusr(vtk_mesh_target=subject, vtk_mesh_source=template, **kwargs)
        reg.align_maps()
        moved = next((getattr(reg, name) for name in _POSITIONS[positions] if getattr(reg, name, None) is not None), None)
        if moved is None:
            raise ValueError("the registration left no %s: check the Focusr options" % _POSITIONS[positions][0])
        rows.append(np.asarray(moved, dtype=np.float64))
    if any(r.shape != rows[0].shape for r in rows):
        raise ValueError("the registrations returned different numbers of points")
    return np.ascontiguousarray(np.stack(rows))
