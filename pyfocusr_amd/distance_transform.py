"""Exact Euclidean distance transforms of masks on the MI355X, and what a mask needs from them.

A mask is an (nx, ny, nz) boolean array or label map (non-zero is foreground; a 2-D image is (nx, ny, 1)) with voxel
`spacing` (one number or three, in the unit of the result).  `pf_edt_create` gives, for every voxel, the exact distance to
the nearest foreground voxel centre and which voxel that is (the feature transform); the definition, ties included, is in
include/pyfocusr_hip.h, tests/_edt_ref.py restates it in numpy and the device returns its bits.

* `distance_transform(mask, spacing)`: the distance of every voxel to the mask (0 inside); `signed=True`: the distance
  to the other class, negative inside; `squared=True`: the squared distances, which is what thresholds should be taken on.
* `signed_distance_of_mask`, `nearest_feature`, `propagate_labels`: the signed field, the index triplet of the nearest
  foreground voxel, and a label map grown into its background.
* `dilate_mask`, `erode_mask`, `open_mask`, `close_mask(mask, radius, spacing)`: morphology with exact Euclidean balls of
  a radius in the unit of the spacing, so on anisotropic voxels too: `dist2 <= radius * radius`.
* `mask_offset_surface(mask, distance, spacing, origin)`: the surface at a signed distance from a segmentation (margins,
  shells) as a closed `PolyMesh`, the distance field handed to the isosurface on the device (`pf_edt_isosurface`).
  `isosurface.mask_to_mesh(..., method="distance")` is its level 0.
"""
import numpy as np

from . import _hip
from .remesh import resample_mesh
from .vtk_functions import PolyMesh


def _context(ctx):
    return ctx if ctx is not None else _hip.default_context()


def _radius(radius):
    radius = float(radius)
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError("radius must be finite and not negative")
    return radius


def distance_transform(mask, spacing=1.0, signed=False, squared=False, return_nearest=False, ctx=None):
    """(nx, ny, nz) float64: the distance from every voxel to the nearest foreground voxel of `mask` (0 inside; +inf
    everywhere if there is none).

    signed          the distance to the nearest voxel of the other class, negative inside the mask (like
                    `signed_distance_volume`); +inf or -inf everywhere if a class is empty.
    squared         the squared distance instead (of the magnitude, with `signed`): exact, no square root taken.
    return_nearest  the result is `(distances, nearest)`; `nearest` (nx, ny, nz) int32 is the flat index of that nearest
                    voxel in `mask.ravel()`, -1 where there is none."""
    mask, spacing = _hip.check_mask(mask, spacing)
    out = _context(ctx).distance_transform(mask, spacing, signed=signed, dist=not squared, dist2=bool(squared),
                                           nearest=bool(return_nearest))
    d = out["dist2" if squared else "dist"]
    return (d, out["nearest"]) if return_nearest else d


def signed_distance_of_mask(mask, spacing=1.0, ctx=None):
    """`distance_transform(mask, spacing, signed=True)`: negative inside, positive outside, never 0."""
    return distance_transform(mask, spacing, signed=True, ctx=ctx)


def nearest_feature(mask, spacing=1.0, ctx=None):
    """(nx, ny, nz, 3) int32: the index triplet (i', j', k') of the foreground voxel nearest to every voxel (a foreground
    voxel's own); -1 everywhere if there is none."""
    mask, spacing = _hip.check_mask(mask, spacing)
    near = _context(ctx).distance_transform(mask, spacing, dist=False, dist2=False)["nearest"]
    out = np.stack(np.unravel_index(np.maximum(near, 0), mask.shape), axis=-1).astype(np.int32)
    out[near < 0] = -1
    return out


def propagate_labels(labels, spacing=1.0, ctx=None):
    """`labels` with every 0 voxel given the label of its nearest non-zero voxel (the feature transform applied to
    `labels.ravel()`); unchanged if every voxel is 0."""
    labels = np.asarray(labels)
    mask, spacing = _hip.check_mask(labels, spacing)
    near = _context(ctx).distance_transform(mask, spacing, dist=False, dist2=False)["nearest"]
    return np.where(near >= 0, labels.reshape(-1)[np.maximum(near, 0)], labels)


def _within(mask, spacing, radius, ctx):
    d2 = _context(ctx).distance_transform(mask, spacing, dist=False, nearest=False)["dist2"]
    return d2 <= radius * radius


def dilate_mask(mask, radius, spacing=1.0, ctx=None):
    """(nx, ny, nz) bool: the voxels within `radius` of a foreground voxel (an exact Euclidean ball; `dist2 <= radius^2`).
    What lies outside the volume contributes nothing."""
    radius = _radius(radius)
    mask, spacing = _hip.check_mask(mask, spacing)
    return _within(mask, spacing, radius, ctx)


def erode_mask(mask, radius, spacing=1.0, ctx=None):
    """(nx, ny, nz) bool: the foreground voxels farther than `radius` from every background voxel: the dilation of the
    complement, complemented.  What lies outside the volume counts as background."""
    radius = _radius(radius)
    mask, spacing = _hip.check_mask(mask, spacing)
    # the voxel outside the volume that is nearest to one inside lies in the first layer around it
    complement = np.pad(mask == 0, 1, mode="constant", constant_values=True)
    return ~_within(complement, spacing, radius, ctx)[1:-1, 1:-1, 1:-1]


def open_mask(mask, radius, spacing=1.0, ctx=None):
    """Erosion, then dilation: specks and bridges thinner than the ball go, the rest keeps its size."""
    return dilate_mask(erode_mask(mask, radius, spacing, ctx=ctx), radius, spacing, ctx=ctx)


def close_mask(mask, radius, spacing=1.0, ctx=None):
    """Dilation, then erosion: pinholes and gaps narrower than the ball are filled."""
    return erode_mask(dilate_mask(mask, radius, spacing, ctx=ctx), radius, spacing, ctx=ctx)


def _origin(origin):
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError("origin must be three finite numbers")
    return origin


def signed_field_surface(mask, level, spacing, origin, pad, ctx=None):
    """(`_hip.Context.isosurface`'s dict, shape, origin of the lattice): the level set of the signed distance field of
    `mask` inside `pad` layers of background, or None if a class of the padded mask is empty.  One `pf_edt_create`, one
    `pf_edt_isosurface`."""
    mask, spacing = _hip.check_mask(mask, spacing)
    origin = _origin(origin)
    if pad:
        mask, origin = np.pad(mask, pad, mode="constant"), origin - pad * spacing
        mask, spacing = _hip.check_mask(mask, spacing)
    if min(mask.shape) < 2:
        raise ValueError("every extent of a mask that becomes a surface must be at least 2, not %r" % (mask.shape,))
    if not mask.any() or mask.all():
        return None, mask.shape, origin
    with _hip.DeviceDistanceTransform(mask, spacing, signed=True, ctx=_context(ctx)) as edt:
        with edt.isosurface(level, origin) as iso:
            pts, faces, key, cell = iso.fetch()
            raw = {"points": pts, "faces": faces, "vertex_key": key, "face_cell": cell, "report": iso.report,
                   "device_ms": edt.device_ms + iso.device_ms}
    return raw, mask.shape, origin


def mask_offset_surface(mask, distance, spacing=1.0, origin=(0.0, 0.0, 0.0), n_vertices=None, ctx=None):
    """The surface at signed distance `distance` from the voxel centres of a segmentation as a closed `PolyMesh`:
    `distance > 0` is a margin around it, `distance < 0` a shell inside it.  The mask is padded with
    `ceil(max(distance, 0) / min(spacing)) + 2` layers of background, its signed distance field stays on the device and
    the isosurface is taken there.  Every vertex lies within one cell diagonal of the exact offset.  A mask with an empty
    class gives a mesh without points.  `n_vertices` passes the result through `resample_mesh`."""
    distance = float(distance)
    if not np.isfinite(distance):
        raise ValueError("distance must be finite")
    checked, spacing = _hip.check_mask(mask, spacing)
    origin = _origin(origin)
    if not checked.any() or checked.all():
        return PolyMesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
    pad = int(np.ceil(max(distance, 0.0) / spacing.min())) + 2
    raw, _, _ = signed_field_surface(checked, distance, spacing, origin, pad, ctx=ctx)
    out = PolyMesh(raw["points"], raw["faces"])
    if n_vertices is not None and len(out.faces):
        out = resample_mesh(out, n_vertices, ctx=ctx)
    return out
