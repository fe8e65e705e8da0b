"""The definition of `pf_isosurface_create` (include/pyfocusr_hip.h) in numpy: marching tetrahedra on the Kuhn
decomposition of every cube.  The device returns these bits.  The case table is derived here from the orientation rule;
nothing is typed in.  Also the small mesh checks the tests of the isosurface share (closedness, Euler characteristic,
components, signed volume)."""
import itertools

import numpy as np

# the edges that leave a lattice point, by kind
KINDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
KIND_OF = {d: k for k, d in enumerate(KINDS)}
PERMS = tuple(itertools.permutations(range(3)))


def tet_vertices(perm):
    """The four corners of the tetrahedron of the axis permutation (a, b, c), as offsets in the unit cube."""
    a, b, _ = perm
    v0 = np.zeros(3, dtype=np.int64)
    v1 = v0.copy()
    v1[a] += 1
    v2 = v1.copy()
    v2[b] += 1
    return np.array([v0, v1, v2, (1, 1, 1)], dtype=np.int64)


def _triangles_of_case(inside):
    """The triangles of a tetrahedron whose local vertices have the `inside` flags, before orientation: triples of
    local vertex pairs (m, n), m < n."""
    def e(p, q):
        return (min(p, q), max(p, q))

    ins = [v for v in range(4) if inside[v]]
    out = [v for v in range(4) if not inside[v]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(out) == 1:
        lone = ins[0] if len(ins) == 1 else out[0]
        rest = [v for v in range(4) if v != lone]
        return [(e(lone, rest[0]), e(lone, rest[1]), e(lone, rest[2]))]
    (a, b), (c, d) = ins, out
    ac, ad, bd, bc = e(a, c), e(a, d), e(b, d), e(b, c)
    return [(ac, ad, bd), (ac, bd, bc)]


def case_table():
    """table[tet][case] = list of triangles; a triangle is three edges, an edge (lower corner offset (3,), kind).  case
    bit v = local vertex v is inside.  A triangle is flipped (its last two vertices swapped) when, with the vertices at
    the edge midpoints of the unit cube, normal . (centroid of the outside corners - centroid of the inside corners) < 0."""
    table = []
    for perm in PERMS:
        tv = tet_vertices(perm)
        row = []
        for case in range(16):
            inside = [(case >> v) & 1 for v in range(4)]
            tris = []
            for tri in _triangles_of_case(inside):
                mid = [(tv[m] + tv[n]) / 2.0 for m, n in tri]
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                c_in = np.mean([tv[v] for v in range(4) if inside[v]], axis=0)
                c_out = np.mean([tv[v] for v in range(4) if not inside[v]], axis=0)
                s = float(np.dot(normal, c_out - c_in))
                assert s != 0.0
                if s < 0.0:
                    tri = (tri[0], tri[2], tri[1])
                tris.append(tuple((tuple(int(x) for x in tv[m]), KIND_OF[tuple(int(x) for x in tv[n] - tv[m])]) for m, n in tri))
            row.append(tris)
        table.append(row)
    return table


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    return _TABLE


def isosurface_ref(values, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), return_cases=False):
    """points (V, 3) f64, faces (F, 3) i32, vertex_key (V,) i64, face_cell (F,) i32 of the definition; with
    `return_cases` also the set of (tetrahedron, case) pairs that produced a face."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    nx, ny, nz = values.shape
    level = float(level)
    spacing = np.asarray(spacing, dtype=np.float64)
    origin = np.asarray(origin, dtype=np.float64)
    inside = values < level
    lin = np.arange(nx * ny * nz, dtype=np.int64).reshape(nx, ny, nz)

    # vertices: one per crossing lattice edge, ascending key
    keys, tpar, lower, delta = [], [], [], []
    for kind, (di, dj, dk) in enumerate(KINDS):
        lo = (slice(0, nx - di), slice(0, ny - dj), slice(0, nz - dk))
        hi = (slice(di, nx), slice(dj, ny), slice(dk, nz))
        cross = inside[lo] != inside[hi]
        vp, vq = values[lo][cross], values[hi][cross]
        t = (level - vp) / (vq - vp)
        idx = np.argwhere(cross).astype(np.int64)
        keys.append(7 * lin[lo][cross] + kind)
        tpar.append(t)
        lower.append(idx)
        delta.append(np.broadcast_to(np.array((di, dj, dk), dtype=np.int64), idx.shape))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    vertex_key = keys[order]
    t = np.concatenate(tpar)[order]
    lower = np.concatenate(lower)[order]
    upper = lower + np.concatenate(delta)[order]
    P = origin[None, :] + lower.astype(np.float64) * spacing[None, :]
    Q = origin[None, :] + upper.astype(np.float64) * spacing[None, :]
    points = P + t[:, None] * (Q - P)

    # faces: ascending cell, tetrahedra in permutation order, triangles in table order
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    ci, cj, ck = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    ci, cj, ck = ci.ravel(), cj.ravel(), ck.ravel()
    cell = (ci * cy + cj) * cz + ck
    table = _table()
    f_cell, f_rank, f_keys = [], [], []
    cases_hit = set()
    for ti, perm in enumerate(PERMS):
        tv = tet_vertices(perm)
        case = np.zeros(cell.shape, dtype=np.int64)
        for v in range(4):
            case |= inside[ci + tv[v, 0], cj + tv[v, 1], ck + tv[v, 2]].astype(np.int64) << v
        for c in range(1, 15):
            sel = np.nonzero(case == c)[0]
            if sel.size == 0:
                continue
            cases_hit.add((ti, c))
            for r, tri in enumerate(table[ti][c]):
                k3 = np.empty((sel.size, 3), dtype=np.int64)
                for e, (off, kind) in enumerate(tri):
                    k3[:, e] = 7 * lin[ci[sel] + off[0], cj[sel] + off[1], ck[sel] + off[2]] + kind
                f_cell.append(cell[sel])
                f_rank.append(np.full(sel.size, 2 * ti + r, dtype=np.int64))
                f_keys.append(k3)
    if f_cell:
        f_cell, f_rank, f_keys = np.concatenate(f_cell), np.concatenate(f_rank), np.concatenate(f_keys)
        order = np.lexsort((f_rank, f_cell))
        face_cell = f_cell[order].astype(np.int32)
        faces = np.searchsorted(vertex_key, f_keys[order]).astype(np.int32)
        assert np.array_equal(vertex_key[faces], f_keys[order])
    else:
        face_cell, faces = np.empty(0, dtype=np.int32), np.empty((0, 3), dtype=np.int32)
    out = (points, faces, vertex_key, face_cell)
    return out + (cases_hit,) if return_cases else out


# ---- mesh checks ------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed(faces):
    """every undirected edge is in exactly two faces"""
    e = np.sort(directed_edges(faces), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool(np.all(counts == 2))


def is_consistent(faces):
    """every directed edge occurs once"""
    e = directed_edges(faces)
    return len(np.unique(e, axis=0)) == len(e)


def euler_characteristic(n_points, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return int(n_points) - len(np.unique(e, axis=0)) + len(faces)


def n_components(n_points, faces):
    parent = np.arange(n_points)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in directed_edges(faces):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return len({find(a) for a in range(n_points)})


def signed_volume(points, faces):
    p = np.asarray(points)[np.asarray(faces, dtype=np.int64)]
    return float(np.sum(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2]))) / 6.0)


# ---- the fields of the issue's cases ----------------------------------------------------------------------------------
def grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def sphere_field():
    x, y, z = grid((9, 10, 11))
    return np.sqrt((x - 4.1) ** 2 + (y - 4.4) ** 2 + (z - 5.2) ** 2) - 3.3


def torus_field():
    x, y, z = grid((14, 14, 8))
    return np.sqrt((np.sqrt((x - 6.4) ** 2 + (y - 6.6) ** 2) - 4.0) ** 2 + (z - 3.3) ** 2) - 1.6


def one_voxel_field():
    v = np.ones((3, 3, 3))
    v[1, 1, 1] = -1.0
    return v


def random_field(seed=0):
    rng = np.random.default_rng(seed)
    return np.pad(rng.standard_normal((6, 7, 5)), 1, constant_values=3.0)


def wave_field(shape):
    x, y, z = grid(shape)
    return np.sin(0.37 * z + 0.9 * x - 0.5 * y) + 0.05
