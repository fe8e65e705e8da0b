"""Plain numpy / scipy restatement of the cotangent assembly of `pf_cotan.hip`, in float64 with the same orders of
summation (the yardstick of tests/test_cotangent.py; it needs no GPU).

Per face, at the corner p with edge vectors u, v to the next and the one-after-next corner:
    cot = (u . v) / |u x v|, the dot product and the squared norm as (a + b) + c;   area = |u x v| / 2 at corner 0.
w_ij = sum over the faces containing the undirected edge (i, j), in ascending face index, of half the cotangent opposite
the edge; d_i = sum_j w_ij left to right in column order; m_i = (sum of the incident faces' areas in ascending face
index) / 3.  S = M^-1/2 (D - W) M^-1/2 on the vertices with m_i > 0."""
import numpy as np
from scipy import sparse

EPS = np.finfo(np.float64).eps


class Degenerate(ValueError):
    pass


def _sum3(a):
    return (a[:, 0] + a[:, 1]) + a[:, 2]


def face_terms(points, faces):
    """half_cot [F][3] (corner k), area [F], inv_sin [F][3] = |u||v| / |u x v| at corner k."""
    p = np.asarray(points, dtype=np.float64)
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("triangles only")
    if f.size and (f.min() < 0 or f.max() >= len(p)):
        raise ValueError("face index out of range")
    if np.any((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])):
        raise Degenerate("a face repeats a vertex")
    half_cot = np.empty((len(f), 3))
    inv_sin = np.empty((len(f), 3))
    area = np.empty(len(f))
    for k in range(3):
        u = p[f[:, (k + 1) % 3]] - p[f[:, k]]
        v = p[f[:, (k + 2) % 3]] - p[f[:, k]]
        dot = _sum3(u * v)
        c = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        nrm = np.sqrt(_sum3(c * c))
        if np.any(~(nrm > 0.0)) or not np.all(np.isfinite(nrm)):
            raise Degenerate("a face has zero area")
        half_cot[:, k] = 0.5 * (dot / nrm)
        inv_sin[:, k] = np.sqrt(_sum3(u * u)) * np.sqrt(_sum3(v * v)) / nrm
        if k == 0:
            area[:] = nrm / 2.0
    return half_cot, area, inv_sin


def _segment_sums(first, count, values):
    """out[s] = values[first[s]] + values[first[s] + 1] + ... (count[s] terms), strictly left to right."""
    out = np.zeros(len(first))
    for t in range(int(count.max()) if len(count) else 0):
        m = count > t
        out[m] += values[first[m] + t]
    return out


def assemble(points, faces):
    """dict: rowptr, colidx (CSR, sorted columns), w, w_bound (sum over the edge's faces of 1 / sin(angle)), diag, mass,
    n_unreferenced, total_area."""
    p = np.asarray(points, dtype=np.float64)
    f = np.asarray(faces).astype(np.int64)
    n, nf = len(p), len(f)
    half_cot, area, inv_sin = face_terms(p, f)
    src, dst, val, snv, fid = [], [], [], [], []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        # the edge (k, a) lies opposite corner b; it is stored in both directions
        for s, d in ((k, a), (a, k)):
            src.append(f[:, s]), dst.append(f[:, d]), val.append(half_cot[:, b]), snv.append(inv_sin[:, b])
            fid.append(np.arange(nf))
    src, dst, val, snv, fid = (np.concatenate(x) if nf else np.zeros(0, dtype=y)
                               for x, y in ((src, np.int64), (dst, np.int64), (val, float), (snv, float), (fid, np.int64)))
    order = np.lexsort((fid, dst, src))  # by (row, column, face)
    src, dst, val, snv = src[order], dst[order], val[order], snv[order]
    new = np.ones(len(src), dtype=bool)
    new[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    first = np.flatnonzero(new)
    count = np.diff(np.append(first, len(src)))
    w = _segment_sums(first, count, val)
    w_bound = _segment_sums(first, count, snv)
    rows, cols = src[first], dst[first]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr)
    diag = _segment_sums(rowptr[:-1], np.diff(rowptr), w)
    # the faces at a vertex in ascending face index
    vf = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]) if nf else np.zeros(0, dtype=np.int64)
    ff = np.tile(np.arange(nf), 3)
    o = np.lexsort((ff, vf))
    vptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(vptr, vf + 1, 1)
    vptr = np.cumsum(vptr)
    mass = _segment_sums(vptr[:-1], np.diff(vptr), area[ff[o]]) / 3.0
    total = 0.0
    for b in range(0, nf, 256):  # one partial per 256 faces (a pairwise tree inside), the partials left to right
        chunk = np.zeros(256)
        chunk[:min(256, nf - b)] = area[b:b + 256]
        while len(chunk) > 1:
            chunk = chunk[:len(chunk) // 2] + chunk[len(chunk) // 2:]
        total += chunk[0]
    return dict(rowptr=rowptr.astype(np.int32), colidx=cols.astype(np.int32), w=w, w_bound=w_bound, diag=diag, mass=mass,
                n_unreferenced=int(np.sum(np.diff(vptr) == 0)), total_area=total, rows=rows)


def matrices(ref):
    """(L_c = D - W, M) as scipy matrices."""
    n = len(ref["mass"])
    W = sparse.csr_matrix((ref["w"], ref["colidx"], ref["rowptr"]), shape=(n, n))
    return sparse.csr_matrix(sparse.diags(ref["diag"]) - W), sparse.diags(ref["mass"])


def symmetric_operator(ref):
    """(S offdiag values in CSR order, S diagonal, hi = max_i sum_j |S_ij|)."""
    m = ref["mass"]
    sm = np.sqrt(m)
    rows, cols = ref["rows"], ref["colidx"]
    off = -(ref["w"] / (sm[rows] * sm[cols]))
    sdiag = np.zeros(len(m))
    np.divide(ref["diag"], m, out=sdiag, where=m > 0)
    row_abs = np.abs(sdiag) + _segment_sums(ref["rowptr"][:-1].astype(np.int64), np.diff(ref["rowptr"]).astype(np.int64), np.abs(off))
    return off, sdiag, float(row_abs.max())


def apply(ref, x):
    """M^-1 (D - W) x as sum_j w_ij (x_i - x_j) / m_i in extended precision, and the per-row sum of w_bound |x_j - x_i| / m_i
    (per column): what an error of w_bound per weight can move the result by."""
    x = np.asarray(x, dtype=np.float64).reshape(len(ref["mass"]), -1)
    rows, cols = ref["rows"], ref["colidx"].astype(np.int64)
    d = (x[rows] - x[cols]).astype(np.longdouble)
    out = np.zeros(x.shape, dtype=np.longdouble)
    np.add.at(out, rows, ref["w"].astype(np.longdouble)[:, None] * d)
    bound = np.zeros(x.shape)
    np.add.at(bound, rows, ref["w_bound"][:, None] * np.abs(x[rows] - x[cols]))
    m = ref["mass"]
    inv = np.zeros(len(m))
    np.divide(1.0, m, out=inv, where=m > 0)
    return (out * inv[:, None]).astype(np.float64), bound * inv[:, None]


def generalized_eigs(ref, k):
    """The k smallest non-null eigenpairs of L_c phi = lambda M phi on the referenced vertices (scipy shift-invert just
    below zero), plus the count of null pairs skipped.  phi^T M phi = I; rows of unreferenced vertices are 0."""
    from scipy.sparse.csgraph import connected_components
    from scipy.sparse.linalg import eigsh

    L, M = matrices(ref)
    keep = np.flatnonzero(ref["mass"] > 0)
    Lk, Mk = sparse.csc_matrix(L[keep][:, keep]), sparse.csc_matrix(M.tocsr()[keep][:, keep])
    n_comp = connected_components(abs(Lk), directed=False)[0]
    lam_scale = 4.0 * np.pi / ref["total_area"]  # (the first eigenvalue of a sphere of this area is twice that)
    vals, vecs = eigsh(Lk, k=k + n_comp, M=Mk, sigma=-1e-3 * lam_scale, which="LM", tol=0)
    o = np.argsort(vals)
    vals, vecs = vals[o], vecs[:, o]
    full = np.zeros((len(ref["mass"]), k))
    full[keep] = vecs[:, n_comp:n_comp + k]
    return vals[n_comp:n_comp + k], full, n_comp
