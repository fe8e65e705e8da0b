"""Mesh smoothing on the MI355X: Taubin and Laplacian fairing of a triangle mesh, or of a field on its vertices.

What comes out of `mask_to_mesh` is a voxel staircase; this is the step between extraction and anything differential
(curvatures, cotangent weights, `resample_mesh`).  A `MeshSmoother` uploads the mesh once and builds a CSR adjacency on
the device (`pf_smoother_create`); a run is one launch per sweep over it (`pf_smoother_run`):

* a sweep with factor f moves every movable vertex to x + f (mean of its neighbours - x), all reads from the previous
  sweep (Jacobi).  `method="laplacian"` is `iterations` sweeps with `lam`; `method="taubin"` is `iterations` pairs of
  sweeps with `lam` and mu = 1 / (pass_band - 1 / lam) < -lam, which does not shrink the surface;
* `weights="uniform"`: the plain mean; `"cotangent"`: the mean weighted by the clipped cotangent weights of the INPUT
  (computed once, never updated);
* `boundary="fixed"`: vertices of edges with one triangle stay; `"free"`: they move like the others; `"curve"`: they
  average only their neighbours along the boundary, so an open rim is smoothed along itself;
* `pinned`: a mask of vertices that never move;
* `max_displacement`: after every iteration each coordinate is clamped into [x0 - c, x0 + c] around the input.
  `smooth_mask_mesh` sets c = spacing / 2, so no vertex leaves the half-voxel box around its lattice position.

float64 throughout, every sum in a fixed order: two calls give the same bits, and tests/_smoothing_ref.py gives them in
numpy.  The exact definitions are in include/pyfocusr_hip.h.  Explicit smoothing only: no implicit fairing, no feature
preservation, weights are not re-evaluated (DESIGN.md has the list).
"""
import numpy as np

from . import _hip, vtk_functions
from ._meshargs import AttrDict, checked_mesh

_METHODS = ("taubin", "laplacian")


class SmoothingInfo(AttrDict):
    """What a smoothing run reports: a dict whose keys are also attributes."""


def taubin_mu(lam, pass_band):
    """mu = 1 / (pass_band - 1 / lam) of Taubin's lambda | mu scheme; ValueError unless it is negative with |mu| > lam."""
    lam, pass_band = float(lam), float(pass_band)
    if not (np.isfinite(lam) and lam > 0.0):
        raise ValueError("lam must be a positive finite number, not %r" % (lam,))
    if not np.isfinite(pass_band):
        raise ValueError("pass_band must be finite, not %r" % (pass_band,))
    d = pass_band - 1.0 / lam
    mu = 1.0 / d if d != 0.0 else np.inf
    if not (np.isfinite(mu) and mu < 0.0 and -mu > lam):
        raise ValueError("pass_band = %r with lam = %r gives mu = %r: Taubin smoothing needs mu < 0 and |mu| > lam "
                         "(0 < pass_band < 1 / lam)" % (pass_band, lam, mu))
    return mu


def _factors(iterations, method, lam, pass_band):
    """(factors (s,) f64, sweeps per iteration, mu or None)."""
    if method not in _METHODS:
        raise ValueError("method must be one of %r, not %r" % (_METHODS, method))
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be a non-negative integer, not %r" % (iterations,))
    iterations = int(iterations)
    if method == "taubin":
        mu = taubin_mu(lam, pass_band)
        return np.tile(np.array([float(lam), mu]), iterations), 2, mu
    lam = float(lam)
    if not (np.isfinite(lam) and lam > 0.0):
        raise ValueError("lam must be a positive finite number, not %r" % (lam,))
    return np.full(iterations, lam), 1, None


def _bound(value, ncols, name):
    """None, or the clamp (ncols,) f64 of a scalar or a vector of ncols entries: not negative, not NaN."""
    if value is None:
        return None
    c = np.asarray(value, dtype=np.float64)
    if c.ndim == 0:
        c = np.full(ncols, float(c))
    if c.shape != (ncols,):
        raise ValueError("%s must be a scalar or have %d entries, not shape %r" % (name, ncols, c.shape))
    if not (c >= 0.0).all():
        raise ValueError("%s must not be negative" % name)
    return np.ascontiguousarray(c)


def _closed_and_oriented(faces):
    """Whether every edge of the triangles is traversed exactly once in each direction (host, integers only)."""
    f = faces.astype(np.int64)
    a, b = f.ravel(), f[:, [1, 2, 0]].ravel()
    if (a == b).any():
        return False
    n = int(f.max()) + 1
    fwd = np.sort(a * n + b)
    return bool((fwd[1:] != fwd[:-1]).all() and np.array_equal(fwd, np.sort(b * n + a)))


def _like(mesh, points, faces):
    """A new mesh of the kind of `mesh` with these points: a (points, faces) pair for a pair, a vtkPolyData for one, else a
    `PolyMesh` with the point data carried over."""
    if isinstance(mesh, (tuple, list)):
        return points, faces.copy()
    if vtk_functions._is_vtk_polydata(mesh):
        from vtk.util.numpy_support import numpy_to_vtk

        out = vtk_functions.vtk_deep_copy(mesh)
        out.GetPoints().SetData(numpy_to_vtk(points, deep=True))
        return out
    data = [(name, np.array(values)) for name, values in getattr(mesh, "point_data", [])]
    return vtk_functions.PolyMesh(points, faces.copy(), data)


class MeshSmoother(object):
    """The smoothing operator of one triangle mesh, resident on the device: build once, run often.

    `mesh`: a `PolyMesh`, a vtkPolyData, an object with `points` and `faces`, or a `(points, faces)` pair.  `weights`:
    "uniform" or "cotangent"; `boundary`: "fixed", "free" or "curve"; `pinned`: a mask (n,) of vertices that never move
    (the module's docstring has the meanings).  Every ValueError is raised before the library is loaded."""

    def __init__(self, mesh, weights="uniform", boundary="fixed", pinned=None, ctx=None):
        pts, faces = checked_mesh(mesh, triangles="smoothing needs", indices=True, finite=True)
        if weights not in _hip.SMOOTH_WEIGHTS:
            raise ValueError("weights must be one of %r, not %r" % (tuple(_hip.SMOOTH_WEIGHTS), weights))
        if boundary not in _hip.SMOOTH_BOUNDARY:
            raise ValueError("boundary must be one of %r, not %r" % (tuple(_hip.SMOOTH_BOUNDARY), boundary))
        if pinned is not None:
            pinned = np.asarray(pinned)
            if pinned.shape != (pts.shape[0],) or pinned.dtype.kind not in "biu":
                raise ValueError("pinned must be a mask with one entry per point (%d), not %s of shape %r"
                                 % (pts.shape[0], pinned.dtype, pinned.shape))
            pinned = np.ascontiguousarray(pinned != 0, dtype=np.uint8)
        self.points, self.faces = pts, faces
        self.weights, self.boundary = weights, boundary
        self._device = _hip.DeviceSmoother(pts, faces, _hip.SMOOTH_WEIGHTS[weights], _hip.SMOOTH_BOUNDARY[boundary], pinned,
                                           ctx=ctx or _hip.default_context())

    @property
    def info(self):
        """edges, boundary_edges, non_manifold_edges, entries, largest_row, movable_vertices of the adjacency."""
        return SmoothingInfo(zip(_hip.SMOOTH_COUNTS, (int(c) for c in self._device.counts)))

    def adjacency(self):
        """(rowptr (n + 1,) int32, col (entries,) int32 ascending per row, w (entries,) f64, kind (n,) uint8 with
        1 = boundary | 2 = pinned | 4 = movable)."""
        return self._device.adjacency()

    def close(self):
        self._device.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _run(self, values, iterations, method, lam, pass_band, bound, stats):
        factors, per_iteration, mu = _factors(iterations, method, lam, pass_band)
        out, st, ms = self._device.run(values, factors, per_iteration, bound, stats)
        info = SmoothingInfo(self.info, mu=mu, sweeps=len(factors), device_ms=ms)
        if st is not None:
            info.update(volume_in=float(st[0]), volume_out=float(st[1]), mean=st[2:5].copy(), max_displacement=float(st[5]))
        return out, info

    def smooth_points(self, iterations=20, method="taubin", lam=0.5, pass_band=0.1, max_displacement=None, return_info=False):
        """The smoothed points (n, 3) of the mesh; with `return_info` also the `SmoothingInfo`: the counts, mu, sweeps,
        device_ms, volume_in, volume_out, mean (of the result's vertices) and max_displacement (the largest component)."""
        out, info = self._run(None, iterations, method, lam, pass_band, _bound(max_displacement, 3, "max_displacement"), True)
        return (out, info) if return_info else out

    def smooth_values(self, values, iterations=10, method="laplacian", lam=0.5, pass_band=0.1, max_change=None, return_info=False):
        """`values` (n,) or (n, c <= 32) smoothed over the mesh as it is; the result has the shape of `values`."""
        values = np.asarray(values)
        if values.ndim not in (1, 2) or values.shape[0] != self.points.shape[0]:
            raise ValueError("values must be (n,) or (n, c) with n = %d points, not shape %r" % (self.points.shape[0], values.shape))
        v = np.ascontiguousarray(values.reshape(values.shape[0], -1), dtype=np.float64)
        if not 1 <= v.shape[1] <= _hip.SMOOTH_MAX_COLUMNS:
            raise ValueError("values have %d columns: 1 .. %d can be smoothed at once" % (v.shape[1], _hip.SMOOTH_MAX_COLUMNS))
        if not np.isfinite(v).all():
            raise ValueError("values must be finite")
        out, info = self._run(v, iterations, method, lam, pass_band, _bound(max_change, v.shape[1], "max_change"), False)
        out = out.reshape(values.shape)
        return (out, info) if return_info else out


def smooth_mesh(mesh, iterations=20, method="taubin", lam=0.5, pass_band=0.1, weights="uniform", boundary="fixed", pinned=None,
                max_displacement=None, preserve_volume=False, return_info=False, ctx=None):
    """A new mesh of the input's kind with smoothed points; faces and point data are carried over, the input is untouched.

    `preserve_volume` (closed, consistently oriented meshes only, else ValueError) rescales the result on the host about
    its vertex mean m by s = cbrt(V_in / V_out): x = m + s (x - m); `info.scale` is s.  With `return_info` the result is
    (mesh, `SmoothingInfo`)."""
    _factors(iterations, method, lam, pass_band)  # refused before the mesh goes to the device
    _bound(max_displacement, 3, "max_displacement")
    if preserve_volume:
        faces = checked_mesh(mesh, triangles="smoothing needs", indices=True, finite=True)[1]
        if not _closed_and_oriented(faces):
            raise ValueError("preserve_volume needs a closed, consistently oriented mesh: every edge in two triangles that "
                             "traverse it in opposite directions")
    with MeshSmoother(mesh, weights=weights, boundary=boundary, pinned=pinned, ctx=ctx) as smoother:
        pts, info = smoother.smooth_points(iterations, method, lam, pass_band, max_displacement, return_info=True)
        faces = smoother.faces
    if preserve_volume:
        ratio = info.volume_in / info.volume_out if info.volume_out != 0.0 else np.nan
        if not (np.isfinite(ratio) and ratio > 0.0):
            raise ValueError("preserve_volume: the signed volume went from %r to %r; the mesh encloses none to preserve"
                             % (info.volume_in, info.volume_out))
        info["scale"] = float(np.cbrt(ratio))
        pts = info.mean + info.scale * (pts - info.mean)
    out = _like(mesh, pts, faces)
    return (out, info) if return_info else out


def smooth_mask_mesh(mesh, spacing, iterations=20, **kw):
    """`smooth_mesh` of a mesh extracted from a mask with voxel size `spacing` (a scalar or three), with
    `max_displacement = spacing / 2`: no vertex leaves the half-voxel box around its lattice position, which is the
    constrained smoothing a segmentation wants."""
    if "max_displacement" in kw:
        raise ValueError("smooth_mask_mesh sets max_displacement = spacing / 2 itself")
    s = np.asarray(spacing, dtype=np.float64)
    if s.shape not in ((), (3,)) or not (np.isfinite(s).all() and (s > 0.0).all()):
        raise ValueError("spacing must be a positive scalar or three positive numbers")
    return smooth_mesh(mesh, iterations=iterations, max_displacement=s / 2.0, **kw)


def smooth_point_data(mesh, values, iterations=10, lam=0.5, method="laplacian", weights="uniform", boundary="free", pass_band=0.1,
                      pinned=None, max_change=None, return_info=False, ctx=None):
    """A scalar or vector field (n,) or (n, c <= 32) smoothed over a fixed mesh, for example a curvature before it is
    thresholded.  `boundary="free"`: rim values are averaged like all others; `pinned` values keep their bits."""
    _factors(iterations, method, lam, pass_band)
    if np.ndim(values) not in (1, 2):
        raise ValueError("values must be (n,) or (n, c), not of %d dimensions" % np.ndim(values))
    if np.ndim(values) == 2 and not 1 <= np.shape(values)[1] <= _hip.SMOOTH_MAX_COLUMNS:
        raise ValueError("values have %d columns: 1 .. %d can be smoothed at once" % (np.shape(values)[1], _hip.SMOOTH_MAX_COLUMNS))
    n = checked_mesh(mesh, triangles="smoothing needs", indices=True, finite=True)[0].shape[0]
    if np.shape(values)[0] != n:
        raise ValueError("values must be (n,) or (n, c) with n = %d points, not shape %r" % (n, np.shape(values)))
    if not np.isfinite(np.asarray(values, dtype=np.float64)).all():
        raise ValueError("values must be finite")
    _bound(max_change, 1 if np.ndim(values) == 1 else np.shape(values)[1], "max_change")
    with MeshSmoother(mesh, weights=weights, boundary=boundary, pinned=pinned, ctx=ctx) as smoother:
        return smoother.smooth_values(values, iterations, method, lam, pass_band, max_change, return_info)
