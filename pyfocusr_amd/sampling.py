"""Point sampling on the device: farthest-point sampling (`pf_fps.hip`).

m samples of a point set, each the point farthest from the samples before it: deterministic and well spread, with the
covering radius and the Voronoi cell of every sample as by-products.  Squared distances are summed coordinate by
coordinate, left to right, with separate multiply and add; ties go to the lowest index; `tests/_fps_ref.py` states the
definition in numpy and the device returns its bits.
"""
import numpy as np

from . import _hip

__all__ = ["farthest_point_sampling", "voronoi_masses"]


def farthest_point_sampling(points_or_mesh, m, start=None, return_owner=False, return_d2=False, ctx=None):
    """sel (int64, m): indices of m farthest-point samples of an (n, d) array, 1 <= d <= 16, or of a mesh's points.

    `start` is the first sample; None starts at the point farthest from the centroid (lowest index on ties).  Each
    further sample is the point with the largest squared distance to its nearest sample so far, the lowest index on ties.
    `return_owner` adds owner (int32, n): the position in sel of every point's nearest sample, the earliest on ties;
    `return_d2` adds the squared distance to it, whose maximum is the squared covering radius of the samples.

    Duplicate points: once every point coincides with a sample all distances are 0 and the arg-max is index 0 again and
    again, so the samples repeat when m exceeds the number of distinct points; nothing is raised.  `PfError` for d
    outside 1 .. 16, m outside 1 .. n, `start` outside 0 .. n - 1 and non-finite coordinates."""
    pts = getattr(points_or_mesh, "points", points_or_mesh)
    pts = np.asarray(pts, dtype=np.float64)
    if pts.ndim != 2:
        raise ValueError("points must be an (n, d) array or a mesh")
    if start is not None and int(start) < 0:
        raise ValueError("start must be a point index or None")
    ctx = ctx if ctx is not None else _hip.default_context()
    return ctx.farthest_point_sampling(pts, int(m), start=-1 if start is None else int(start), return_owner=return_owner,
                                       return_d2=return_d2)


def voronoi_masses(owner, mass, m):
    """(m,) the mass of every sample's Voronoi cell - with vertex areas as `mass`, the area each sample represents:
    `np.bincount(owner, weights=mass, minlength=m)` (one pass on the host).  A sample that repeats an earlier one owns
    nothing."""
    owner, mass = np.asarray(owner), np.asarray(mass, dtype=np.float64)
    if owner.ndim != 1 or owner.shape != mass.shape:
        raise ValueError("owner and mass must be vectors of equal length")
    if owner.size and (owner.min() < 0 or owner.max() >= int(m)):
        raise ValueError("owner must lie in 0 .. m - 1")
    return np.bincount(owner, weights=mass, minlength=int(m))
