"""The definition of `pf_edt_create` (include/pyfocusr_hip.h) in numpy: the exact Euclidean distance transform of a mask
with anisotropic spacing and its feature transform, stage by stage as the header states it (`edt_staged`), the global
minimum it must equal bit for bit (`edt_brute`, for small volumes), the signed mode built from either, and the ball
morphology of `pyfocusr_amd.distance_transform` over the staged transform.  No device, no library."""
import numpy as np

_TABLE = 1 << 22  # doubles of one chunk's (lines, line, line) table: 32 MiB, so a volume of about 1e6 samples fits in memory


def _three(spacing):
    s = np.asarray(spacing, dtype=np.float64)
    return np.repeat(s, 3) if s.ndim == 0 else s.reshape(3)


def _stage(g, near, axis, s):
    """One stage along `axis`: out[.., c, ..] = min over c' of fl(g[.., c', ..] + (s (c - c')) (s (c - c'))), the lowest c'
    on a tie (argmin takes the first), and the `near` of that c'; a line whose g is +inf throughout keeps +inf and -1."""
    n = g.shape[axis]
    lines = np.moveaxis(g, axis, -1).reshape(-1, n)
    carried = np.moveaxis(near, axis, -1).reshape(-1, n)
    d = (np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64)
    t = (s * d) * (s * d)  # [c][c']
    out_g, out_n = np.empty_like(lines), np.empty_like(carried)
    step = max(1, _TABLE // (n * n))
    for a in range(0, len(lines), step):
        cost = lines[a:a + step, None, :] + t[None, :, :]  # [line][c][c']
        pick = np.argmin(cost, axis=2)
        out_g[a:a + step] = np.take_along_axis(cost, pick[:, :, None], axis=2)[:, :, 0]
        out_n[a:a + step] = np.take_along_axis(carried[a:a + step], pick, axis=1)
    out_n[np.isinf(out_g)] = -1
    shape = np.moveaxis(g, axis, -1).shape
    return np.moveaxis(out_g.reshape(shape), -1, axis), np.moveaxis(out_n.reshape(shape), -1, axis)


def edt_staged(mask, spacing=1.0):
    """(dist2 (nx, ny, nz) f64, nearest (nx, ny, nz) int32) by the three stages z, y, x of the header.  Stage z is the
    general stage over g = 0 at a feature and +inf elsewhere, each feature carrying its own flat index: fl(0 + t_z) = t_z."""
    feature = np.asarray(mask) != 0
    s = _three(spacing)
    g = np.where(feature, 0.0, np.inf)
    near = np.where(feature, np.arange(feature.size, dtype=np.int32).reshape(feature.shape), np.int32(-1)).astype(np.int32)
    for axis in (2, 1, 0):
        g, near = _stage(g, near, axis, s[axis])
    return np.ascontiguousarray(g), np.ascontiguousarray(near)


def cost(shape, spacing, p_flat, q_flat):
    """c(p, q) = (t_z + t_y) + t_x of the header for flat indices p and q (arrays that broadcast)."""
    s = _three(spacing)
    p, q = np.unravel_index(p_flat, shape), np.unravel_index(q_flat, shape)
    t = [(s[a] * (p[a] - q[a]).astype(np.float64)) * (s[a] * (p[a] - q[a]).astype(np.float64)) for a in range(3)]
    return (t[2] + t[1]) + t[0]


def edt_brute(mask, spacing=1.0):
    """(dist2, lowest (nx, ny, nz) int32): the global minimum of c(p, q) over all features q and the lowest flat index
    among its minimisers; +inf and -1 without a feature.  All pairs at once: small volumes only."""
    feature = np.asarray(mask) != 0
    q = np.flatnonzero(feature)  # ascending flat index
    if not len(q):
        return np.full(feature.shape, np.inf), np.full(feature.shape, -1, dtype=np.int32)
    c = cost(feature.shape, spacing, np.arange(feature.size)[:, None], q[None, :])
    pick = np.argmin(c, axis=1)
    return c[np.arange(feature.size), pick].reshape(feature.shape), q[pick].astype(np.int32).reshape(feature.shape)


def signed_from(mask, to_foreground, to_background):
    """(dist, dist2, nearest) of signed mode from the (dist2, nearest) of the mask and of its complement."""
    inside = np.asarray(mask) != 0
    dist = np.sqrt(to_foreground[0]) - np.sqrt(to_background[0])
    return dist, np.where(inside, to_background[0], to_foreground[0]), np.where(inside, to_background[1], to_foreground[1])


def edt_signed(mask, spacing=1.0, transform=edt_staged):
    inside = np.asarray(mask) != 0
    return signed_from(inside, transform(inside, spacing), transform(~inside, spacing))


def dilate(mask, radius, spacing=1.0):
    return edt_staged(mask, spacing)[0] <= radius * radius


def erode(mask, radius, spacing=1.0):
    """Outside the volume counts as background: one layer of it is where the nearest outside voxel lies."""
    complement = np.pad(np.asarray(mask) == 0, 1, mode="constant", constant_values=True)
    return ~dilate(complement, radius, spacing)[1:-1, 1:-1, 1:-1]


def ball(radius):
    """The structuring element {o : |o|^2 <= r^2} on the unit lattice, as scipy.ndimage takes it."""
    n = int(np.floor(radius))
    o = np.arange(-n, n + 1)
    return (o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= radius * radius


def ball_mask(shape, centre, radius, spacing=1.0):
    s = _three(spacing)
    axes = [(np.arange(shape[a]) - centre[a]) * s[a] for a in range(3)]
    return axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2 <= radius * radius
