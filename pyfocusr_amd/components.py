"""Connected components of masks and label maps on the MI355X, and what a segmentation needs from them.

A volume is an (nx, ny, nz) boolean array or label map of integers (0 is background).  `pf_ccl_create` labels its connected
components for 6-, 18- or 26-connectivity and gives exact integer statistics for each; the definition, numbering included,
is in include/pyfocusr_hip.h, tests/_ccl_ref.py restates it in numpy and the device returns its bytes.  In binary mode the
labels are `scipy.ndimage.label`'s.  The host chooses components from the small tables, the device applies the choice to
the volume (`pf_ccl_select`), so none of the functions below moves the surface of what it keeps.

* `connected_components(vol, connectivity, by_value, background, return_stats)`: `(labels, n)` and a `ComponentStats`.
* `keep_largest_components(mask, n)`, `remove_small_components(mask, min_voxels | min_volume)`: specks go.
* `largest_component_per_label(labels)`: the same for every value of a label map, values preserved.
* `fill_holes(mask)`: the background components that do not reach the border are filled.
* `component_boxes(stats, pad)`: crop slices.
"""
import numpy as np

from . import _hip


def _context(ctx):
    return ctx if ctx is not None else _hip.default_context()


def _spacing(spacing):
    spacing = np.asarray(spacing, dtype=np.float64)
    spacing = np.repeat(spacing, 3) if spacing.ndim == 0 else spacing.reshape(-1)
    if spacing.shape != (3,):
        raise ValueError("spacing must be one number or three")
    if not (np.isfinite(spacing).all() and (spacing > 0.0).all()):
        raise ValueError("spacing must be positive and finite")
    return spacing


class ComponentStats(object):
    """The tables of `pf_ccl_fetch` for the C components of a volume of `shape`, component c + 1 in row c: `count` (C,)
    int64 voxels, `value` (C,) int32 the input at the root (0 for background components), `root` (C,) int32 the lowest flat
    index, `lo` and `hi` (C, 3) int32 the inclusive bounding box, `border` (C,) bool whether the component touches the
    border of the volume, `sum` (C, 3) int64 the sums of the indices.  Everything else is arithmetic on these."""

    def __init__(self, shape, count, value, root, lo, hi, border, sum):  # noqa: A002
        self.shape = tuple(int(e) for e in shape)
        self.count, self.value, self.root, self.lo, self.hi, self.sum = count, value, root, lo, hi, sum
        self.border = np.asarray(border).astype(bool)

    def __len__(self):
        return len(self.count)

    def centroid(self, spacing=1.0, origin=(0.0, 0.0, 0.0)):
        """(C, 3) float64: origin + spacing * (mean index) of every component."""
        origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("origin must be three finite numbers")
        return origin + _spacing(spacing) * (self.sum / self.count[:, None].astype(np.float64))

    def volume(self, spacing=1.0):
        """(C,) float64: count times the volume of a voxel."""
        return self.count * float(np.prod(_spacing(spacing)))

    @property
    def bounding_box(self):
        """Per component the tuple of three slices that crops it."""
        return component_boxes(self, 0)


def component_boxes(stats, pad=0):
    """Per component of `stats` the tuple of three slices of its bounding box grown by `pad` voxels, clamped to the volume."""
    pad = int(pad)
    if pad < 0:
        raise ValueError("pad must not be negative")
    lo = np.maximum(stats.lo.astype(np.int64) - pad, 0)
    hi = np.minimum(stats.hi.astype(np.int64) + pad + 1, np.array(stats.shape, dtype=np.int64))
    return [tuple(slice(int(a), int(b)) for a, b in zip(l, h)) for l, h in zip(lo, hi)]


def _stats(shape, raw):
    return ComponentStats(shape, *[raw[k] for k in _hip.CCL_TABLES])


def connected_components(vol, connectivity=6, by_value=False, background=False, return_stats=False, ctx=None):
    """`(labels, n)`: labels (nx, ny, nz) int32, 0 on the background and 1..n on the components, numbered by their lowest
    voxel in C order (`scipy.ndimage.label`'s numbering).  connectivity 6, 18 or 26.

    by_value      neighbours are joined only if their values are equal: the components of every label of a label map.
    background    the zero voxels are labelled instead, the non-zero ones are the background.
    return_stats  the result is `(labels, n, ComponentStats)`."""
    vol, connectivity = _hip.check_label_volume(vol, connectivity)
    if by_value and background:
        raise ValueError("by_value and background exclude each other: the background has one value")
    mode = _hip.PF_CCL_BACKGROUND if background else (_hip.PF_CCL_BY_VALUE if by_value else _hip.PF_CCL_BINARY)
    raw = _context(ctx).connected_components(vol, connectivity, mode, stats=bool(return_stats))
    if return_stats:
        return raw["component"], raw["n"], _stats(vol.shape, raw)
    return raw["component"], raw["n"]


def _largest(count, n):
    """keep (C,) bool: the n largest counts; ties go to the lower component number."""
    keep = np.zeros(len(count), dtype=bool)
    keep[np.argsort(-count, kind="stable")[:n]] = True
    return keep


def keep_largest_components(mask, n=1, connectivity=6, ctx=None):
    """(nx, ny, nz) bool: the `n` largest components of the mask (by voxel count; ties go to the component that comes first
    in C order).  No voxel of what is kept changes."""
    vol, connectivity = _hip.check_label_volume(mask, connectivity)
    if int(n) != n or n < 1:
        raise ValueError("n must be a whole number of at least 1, not %r" % (n,))
    return _context(ctx).connected_components(vol, connectivity, _hip.PF_CCL_BINARY, component=False, stats=False,
                                              keep=lambda t: _largest(t["count"], int(n)))["selected"]


def _largest_per_value(count, value):
    """keep (C,) bool: for every distinct value its largest component; ties go to the lower component number."""
    keep = np.zeros(len(count), dtype=bool)
    order = np.lexsort((np.arange(len(count)), -count, value))
    first = np.ones(len(order), dtype=bool)
    first[1:] = value[order][1:] != value[order][:-1]
    keep[order[first]] = True
    return keep


def largest_component_per_label(labels, connectivity=6, ctx=None):
    """`labels` with everything but the largest component of every distinct non-zero value set to 0; the values and the
    dtype are kept.  Ties go to the component that comes first in C order."""
    labels = np.asarray(labels)
    vol, connectivity = _hip.check_label_volume(labels, connectivity)
    sel = _context(ctx).connected_components(vol, connectivity, _hip.PF_CCL_BY_VALUE, component=False, stats=False,
                                             keep=lambda t: _largest_per_value(t["count"], t["value"]))["selected"]
    return np.where(sel, labels, np.zeros((), dtype=labels.dtype))


def remove_small_components(mask, min_voxels=None, min_volume=None, spacing=1.0, connectivity=6, ctx=None):
    """(nx, ny, nz) bool: the components of the mask with at least `min_voxels` voxels, or with a volume of at least
    `min_volume` in the unit of `spacing` cubed.  Exactly one of the two thresholds is given."""
    vol, connectivity = _hip.check_label_volume(mask, connectivity)
    if (min_voxels is None) == (min_volume is None):
        raise ValueError("exactly one of min_voxels and min_volume must be given")
    if min_voxels is not None:
        if not np.isfinite(min_voxels) or min_voxels < 0:
            raise ValueError("min_voxels must be finite and not negative")
        choose = lambda t: t["count"] >= min_voxels  # noqa: E731
    else:
        if not np.isfinite(min_volume) or min_volume < 0:
            raise ValueError("min_volume must be finite and not negative")
        voxel = float(np.prod(_spacing(spacing)))
        choose = lambda t: t["count"] * voxel >= min_volume  # noqa: E731
    return _context(ctx).connected_components(vol, connectivity, _hip.PF_CCL_BINARY, component=False, stats=False, keep=choose)["selected"]


def fill_holes(mask, connectivity=6, ctx=None):
    """(nx, ny, nz) bool: the mask with its cavities filled: the components of the background, at `connectivity`, that do
    not reach the border of the volume.  With 6 this is `scipy.ndimage.binary_fill_holes`."""
    vol, connectivity = _hip.check_label_volume(mask, connectivity)
    sel = _context(ctx).connected_components(vol, connectivity, _hip.PF_CCL_BACKGROUND, component=False, stats=False,
                                             keep=lambda t: t["border"] == 0)["selected"]
    return (vol != 0) | sel
