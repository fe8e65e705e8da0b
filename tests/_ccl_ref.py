"""The definition of the connected components of include/pyfocusr_hip.h (pf_ccl_*) in plain numpy and Python; the device
returns these bytes.

A voxel of `vol` (nx, ny, nz) is labelled if it is non-zero (modes "binary" and "by_value") or zero (mode "background").
Two labelled voxels that differ by at most 1 on every axis, in at most 1 / 2 / 3 axes for connectivity 6 / 18 / 26, are joined
(in mode "by_value" only if their values are equal).  A component is a class of the transitive closure, its root its lowest
flat index, and components are numbered 1..C by ascending root.  `label` states that with a union-find over all joined
pairs; `label_flood` is the raster-order flood fill, which gives the numbering directly (slow: small volumes only)."""
import itertools

import numpy as np

MODES = ("binary", "by_value", "background")  # PF_CCL_BINARY, PF_CCL_BY_VALUE, PF_CCL_BACKGROUND
AXES = {6: 1, 18: 2, 26: 3}


def offsets(connectivity, half=True):
    """The neighbour offsets of the connectivity; half: only those that point forward in C order."""
    out = [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(x != 0 for x in o) <= AXES[connectivity]]
    return [o for o in out if o > (0, 0, 0)] if half else out


def labelled(vol, mode):
    vol = np.asarray(vol)
    return vol == 0 if mode == "background" else vol != 0


def joined_pairs(vol, connectivity, mode):
    """(a, b) flat indices, a < b, of every pair of joined neighbours."""
    vol = np.asarray(vol)
    on, idx = labelled(vol, mode), np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    a_all, b_all = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for off in offsets(connectivity):
        src = tuple(slice(max(0, -o), vol.shape[d] - max(0, o)) for d, o in enumerate(off))
        dst = tuple(slice(max(0, o), vol.shape[d] - max(0, -o)) for d, o in enumerate(off))
        both = on[src] & on[dst]
        if mode == "by_value":
            both &= vol[src] == vol[dst]
        a_all.append(idx[src][both])
        b_all.append(idx[dst][both])
    return np.concatenate(a_all), np.concatenate(b_all)


def label(vol, connectivity=6, mode="binary"):
    """(component (nx, ny, nz) int32, C)."""
    vol = np.asarray(vol)
    a, b = joined_pairs(vol, connectivity, mode)
    parent = np.arange(vol.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])  # the larger root under the smaller
        while True:  # every voxel to its root
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    on = labelled(vol, mode).reshape(-1)
    is_root = on & (parent == np.arange(vol.size))
    number = np.cumsum(is_root)  # ascending root
    component = np.where(on, number[parent], 0).astype(np.int32).reshape(vol.shape)
    return component, int(is_root.sum())


def label_flood(vol, connectivity=6, mode="binary"):
    """`label` as a flood fill from every unlabelled voxel in raster order."""
    vol = np.asarray(vol)
    on, values, shape = labelled(vol, mode).tolist(), vol.tolist(), vol.shape
    component = np.zeros(shape, dtype=np.int32)
    offs, n = offsets(connectivity, half=False), 0
    for seed in itertools.product(*[range(e) for e in shape]):
        if not on[seed[0]][seed[1]][seed[2]] or component[seed]:
            continue
        n += 1
        component[seed] = n
        stack = [seed]
        while stack:
            i, j, k = stack.pop()
            for di, dj, dk in offs:
                q = (i + di, j + dj, k + dk)
                if min(q) < 0 or q[0] >= shape[0] or q[1] >= shape[1] or q[2] >= shape[2]:
                    continue
                if not on[q[0]][q[1]][q[2]] or component[q]:
                    continue
                if mode == "by_value" and values[q[0]][q[1]][q[2]] != values[i][j][k]:
                    continue
                component[q] = n
                stack.append(q)
    return component, n


def statistics(vol, component, n, mode="binary"):
    """The tables of pf_ccl_fetch: count (C,) i64, value (C,) i32, root (C,) i32, lo (C, 3) i32, hi (C, 3) i32, border (C,)
    u8, sum (C, 3) i64."""
    vol = np.asarray(vol)
    c = component.reshape(-1).astype(np.int64)
    at = np.flatnonzero(c)
    c0 = c[at] - 1
    ijk = np.stack(np.unravel_index(at, vol.shape), axis=1).astype(np.int64)
    count = np.bincount(c0, minlength=n).astype(np.int64)
    root = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(root, c0, at)
    lo, hi = np.full((n, 3), np.iinfo(np.int32).max, dtype=np.int64), np.full((n, 3), -1, dtype=np.int64)
    total, border = np.zeros((n, 3), dtype=np.int64), np.zeros(n, dtype=np.uint8)
    for axis in range(3):
        np.minimum.at(lo[:, axis], c0, ijk[:, axis])
        np.maximum.at(hi[:, axis], c0, ijk[:, axis])
        total[:, axis] = _int_bincount(c0, ijk[:, axis], n)
        edge = (ijk[:, axis] == 0) | (ijk[:, axis] == vol.shape[axis] - 1)
        border[c0[edge]] = 1
    value = np.zeros(n, dtype=np.int32) if mode == "background" or not n else vol.reshape(-1)[root].astype(np.int32)
    return {"count": count, "value": value, "root": root.astype(np.int32), "lo": lo.astype(np.int32), "hi": hi.astype(np.int32),
            "border": border, "sum": total}


def _int_bincount(bins, weights, n):
    """np.bincount with integer weights, exactly (bincount's own weights are doubles)."""
    out = np.zeros(n, dtype=np.int64)
    np.add.at(out, bins, weights)
    return out


def components(vol, connectivity=6, mode="binary"):
    """(component, C, tables)."""
    component, n = label(vol, connectivity, mode)
    return component, n, statistics(vol, component, n, mode)


def select(component, keep):
    keep = np.concatenate([[False], np.asarray(keep, dtype=bool)])
    return keep[component]


def largest(count, n=1):
    """keep (C,) bool of the n largest counts; a tie goes to the lower number."""
    order = sorted(range(len(count)), key=lambda c: (-int(count[c]), c))
    keep = np.zeros(len(count), dtype=bool)
    keep[order[:n]] = True
    return keep


def keep_largest(mask, n=1, connectivity=6):
    component, _, t = components(np.asarray(mask) != 0, connectivity)
    return select(component, largest(t["count"], n))


def remove_small(mask, min_voxels, connectivity=6):
    component, _, t = components(np.asarray(mask) != 0, connectivity)
    return select(component, t["count"] >= min_voxels)


def largest_per_label(labels, connectivity=6):
    labels = np.asarray(labels)
    component, n, t = components(labels, connectivity, "by_value")
    keep = np.zeros(n, dtype=bool)
    for v in np.unique(t["value"]):
        members = np.flatnonzero(t["value"] == v)
        keep[members[largest(t["count"][members])]] = True
    return np.where(select(component, keep), labels, 0).astype(labels.dtype)


def fill_holes(mask, connectivity=6):
    mask = np.asarray(mask) != 0
    component, _, t = components(mask, connectivity, "background")
    return mask | select(component, t["border"] == 0)


def ball_mask(shape, centre, radius, spacing=(1.0, 1.0, 1.0)):
    g = np.meshgrid(*[np.arange(e, dtype=np.float64) for e in shape], indexing="ij")
    return sum(((g[a] - centre[a]) * spacing[a]) ** 2 for a in range(3)) <= radius * radius
