"""Numpy reference of the shape-population primitives (`pf_shapes_*`), of the generalized Procrustes alignment and of the
Gram PCA built on them (tests/test_shape_model.py), written from the definitions in include/pyfocusr_hip.h and from the
algorithm as pyfocusr_amd/shape_model.py documents it; and the populations the tests use.

Products and sums are written out one operation at a time in the stated order (numpy contracts nothing): T(.) is
`tree_sum` of `_map_quality_ref` (256 consecutive terms left to right from 0.0, 256 of those sums likewise, the rest in
order), dot3 is (a0 b0 + a1 b1) + a2 b2, sums over the shapes go left to right.  Only + - x / occur on the device, each
correctly rounded here and there, and the small dense steps (3 x 3 SVD, S x S eigh) are the same numpy calls on inputs that
are equal bit for bit: the device path is expected to return these bits."""
import numpy as np

from _map_quality_ref import GROUP, tree_sum

EIGENVALUE_FLOOR = 1e-10


def tree_sums(x):
    """`tree_sum` of every column of x (n, m) at once: (m,).  (test_tree_sums_is_tree_sum_per_column holds them together.)"""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(len(x), -1)
    for _ in range(2):
        pad = (-len(x)) % GROUP
        block = np.concatenate([x, np.zeros((pad, x.shape[1]))]).reshape(-1, GROUP, x.shape[1])
        acc = np.zeros((block.shape[0], x.shape[1]))
        for k in range(GROUP):
            acc = acc + block[:, k]
        x = acc
    total = np.zeros(x.shape[1])
    for v in x:
        total = total + v
    return total


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class RefShapes(object):
    """The state and the primitives of a `pf_shapes` handle, under the names of `_hip.DeviceShapes`."""

    def __init__(self, shapes, weights=None):
        self.X = np.array(shapes, dtype=np.float64)
        self.S, self.n = self.X.shape[:2]
        self.w = np.ones(self.n) if weights is None else np.array(weights, dtype=np.float64)  # 1.0 x = x: the same bits
        self.r = np.zeros((self.n, 3))
        self.weight_sum = tree_sum(self.w)

    def center(self):
        c = np.empty((self.S, 3))
        for s in range(self.S):
            c[s] = tree_sums(self.w[:, None] * self.X[s]) / self.weight_sum
            self.X[s] = self.X[s] - c[s]
        return c

    def mean(self, first=0, count=None, return_mean=True):
        count = self.S - first if count is None else count
        acc = self.X[first].copy()
        for s in range(first + 1, first + count):
            acc = acc + self.X[s]
        m = acc / float(count)
        d = m - self.r
        change = tree_sum(self.w * dot3(d, d))
        self.r = m
        return (m.copy() if return_mean else None), change

    def align_sums(self):
        H, q = np.empty((self.S, 3, 3)), np.empty(self.S)
        for s in range(self.S):
            wx = self.w[:, None] * self.X[s]
            H[s] = tree_sums(wx[:, :, None] * self.r[:, None, :]).reshape(3, 3)
            q[s] = tree_sum(self.w * dot3(self.X[s], self.X[s]))
        return H, q, tree_sum(self.w * dot3(self.r, self.r))

    def transform(self, R, scale=None, t=None):
        scale = np.ones(self.S) if scale is None else scale
        for s in range(self.S):
            x0, x1, x2 = self.X[s, :, 0], self.X[s, :, 1], self.X[s, :, 2]
            y = np.empty((self.n, 3))
            for b in range(3):
                y[:, b] = scale[s] * ((x0 * R[s][0][b] + x1 * R[s][1][b]) + x2 * R[s][2][b])
                if t is not None:
                    y[:, b] = y[:, b] + t[s][b]
            self.X[s] = y

    def gram(self):
        d = self.X - self.r
        G = np.empty((self.S, self.S))
        for s in range(self.S):
            G[s, s:] = tree_sums((self.w * dot3(d[s][None], d[s:])).T)
            G[s:, s] = G[s, s:]
        return G

    def combine(self, coeff):
        d = self.X - self.r
        out = np.zeros((len(coeff), self.n, 3))
        for k in range(len(coeff)):
            for s in range(self.S):
                out[k] = out[k] + coeff[k][s] * d[s]
        return out

    def scores(self, modes):
        d = self.X - self.r
        b = np.empty((self.S, len(modes)))
        for s in range(self.S):
            b[s] = tree_sums((self.w * dot3(d[s][None], modes)).T)
        return b

    def set_reference(self, ref):
        self.r = np.array(ref, dtype=np.float64)

    def download(self):
        return self.X.copy()


# ---- the algorithm -----------------------------------------------------------------------------------------------------
def kabsch(H, q, rho, scaling, reflection):
    """Rotation (applied as x R to a row vector) and scale of one shape onto the reference from H = sum w x r^T."""
    U, sv, Vt = np.linalg.svd(H)
    d = np.ones(3)
    if not reflection and np.linalg.det(U @ Vt) < 0.0:
        d[2] = -1.0
    R = (U * d) @ Vt
    if not scaling:
        return R, 1.0
    return R, ((sv[0] * d[0] + sv[1] * d[1]) + sv[2] * d[2]) / (rho * q)


def _matrices(R, scale):
    M = np.zeros((len(R), 4, 4))
    M[:, :3, :3] = scale[:, None, None] * np.transpose(R, (0, 2, 1))
    M[:, 3, 3] = 1.0
    return M


def generalized_procrustes(shapes, weights=None, scaling=True, reflection=False, max_iter=100, tol=1e-10, keep=False):
    """dict(aligned, mean, transforms, history, n_iter, converged) (and the RefShapes with `keep`)."""
    ref = RefShapes(shapes, weights)
    S, W = ref.S, ref.weight_sum
    eye = np.tile(np.eye(3), (S, 1, 1))
    M = np.tile(np.eye(4), (S, 1, 1))
    M[:, :3, 3] = -ref.center()
    if scaling:
        q = ref.align_sums()[1]
        k = 1.0 / np.sqrt(q / W)
        ref.transform(eye, k)
        M = _matrices(eye, k) @ M
    mean, _ = ref.mean(0, 1)
    history, converged = [], False
    for _ in range(max_iter):
        H, q, rho2 = ref.align_sums()
        rho = np.sqrt(rho2 / W)
        R, scale = np.empty((S, 3, 3)), np.empty(S)
        for s in range(S):
            R[s], scale[s] = kabsch(H[s], q[s], rho, scaling, reflection)
        ref.transform(R, scale)
        M = _matrices(R, scale) @ M
        mean, change = ref.mean()
        history.append(change)
        if np.sqrt(change / W) < tol * rho:
            converged = True
            break
    out = dict(aligned=ref.download(), mean=mean, transforms=M, history=np.array(history), n_iter=len(history), converged=converged,
               rho=rho, weight_sum=W)
    return (out, ref) if keep else out


def principal_modes(ref, n_modes=None):
    """dict(eigenvalues, all_eigenvalues, vectors (K, S) sign-fixed unit eigenvectors, coeff, modes, scores) of a RefShapes
    whose reference is the mean."""
    S = ref.S
    lam, U = np.linalg.eigh(ref.gram() / (S - 1))
    lam, U = lam[::-1], U[:, ::-1]
    keep = int(np.count_nonzero(lam[:S - 1] > EIGENVALUE_FLOOR * lam[0]))
    if n_modes is not None:
        keep = min(keep, n_modes)
    vectors, coeff = np.empty((keep, S)), np.empty((keep, S))
    for k in range(keep):
        u = U[:, k]
        if u[np.argmax(np.abs(u))] < 0.0:
            u = -u
        vectors[k] = u
        coeff[k] = u / np.sqrt((S - 1) * lam[k])
    modes = ref.combine(coeff)
    return dict(eigenvalues=lam[:keep].copy(), all_eigenvalues=lam.copy(), vectors=vectors, coeff=coeff, modes=modes,
                scores=ref.scores(modes))


def build_shape_model(shapes, weights=None, n_modes=None, **gpa):
    g, ref = generalized_procrustes(shapes, weights, keep=True, **gpa)
    p = principal_modes(ref, n_modes)
    total = float(np.sum(p["all_eigenvalues"][p["all_eigenvalues"] > 0.0]))
    return dict(g, explained_variance_ratio=p["eigenvalues"] / total, weights=weights, **p)


def project(model, points, weights=None, align=True, scaling=True, reflection=False):
    ref = RefShapes(np.asarray(points, dtype=np.float64)[None], weights)
    ref.set_reference(model["mean"])
    if align:
        ref.center()
        H, q, rho2 = ref.align_sums()
        R, scale = kabsch(H[0], q[0], np.sqrt(rho2 / ref.weight_sum), scaling, reflection)
        ref.transform(R[None], np.array([scale]))
    return ref.scores(model["modes"])[0]


def reconstruct(model, b):
    return model["mean"] + np.tensordot(b, model["modes"][:len(b)], axes=([0], [0]))


def inner(a, b, weights=None):
    """The weighted inner product sum_i w_i a_i . b_i of two (n, 3) fields (plain numpy: for the algebra checks)."""
    w = np.ones(len(a)) if weights is None else weights
    return float(np.sum(w * np.sum(a * b, axis=1)))


# ---- populations -------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    """A rotation matrix drawn uniformly (QR of a Gaussian matrix, the determinant made +1)."""
    Q, Rm = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(Rm))
    if np.linalg.det(Q) < 0.0:
        Q[:, 2] = -Q[:, 2]
    return Q


def rms_size(points, weights=None):
    w = np.ones(len(points)) if weights is None else weights
    c = (w[:, None] * points).sum(0) / w.sum()
    return float(np.sqrt(np.sum(w * np.sum((points - c) ** 2, axis=1)) / w.sum()))


def blob_points(n=700, seed=0):
    from pyfocusr_amd.meshgen import blob_mesh

    return np.ascontiguousarray(blob_mesh(n, seed=seed).points, dtype=np.float64)


def similarity_population(points, S=12, seed=0, scaling=True):
    """One shape under S random similarity transforms: scale 0.7 .. 1.3 (1 without `scaling`), any rotation, a
    translation of about 5 sizes."""
    rng = np.random.default_rng(seed)
    size = rms_size(points)
    out = np.empty((S,) + points.shape)
    for s in range(S):
        k = rng.uniform(0.7, 1.3) if scaling else 1.0
        out[s] = k * (points @ random_rotation(rng).T) + 5.0 * size * rng.standard_normal(3)
    return out


def planted_modes(points):
    """(centred points P, m1, m2): m1 an x-stretch, m2 = (0, y z, 0) orthogonalised against m1, both of unit Frobenius norm."""
    P = points - points.mean(0)
    m1 = np.zeros_like(P)
    m1[:, 0] = P[:, 0]
    m1 = m1 / np.linalg.norm(m1)
    m2 = np.zeros_like(P)
    m2[:, 1] = P[:, 1] * P[:, 2]
    m2 = m2 - np.sum(m2 * m1) * m1
    m2 = m2 / np.linalg.norm(m2)
    return P, m1, m2


def planted_population(points, S=12, seed=0, amplitudes=(0.3, 0.1)):
    """(shapes (S, n, 3), P, m1, m2, coefficients (S, 2)): P + a1 m1 + a2 m2 with a_j ~ N(0, (amplitude_j |P|)^2), under
    random rigid transforms."""
    P, m1, m2 = planted_modes(points)
    rng = np.random.default_rng(seed)
    norm = np.linalg.norm(P)
    size = rms_size(P)
    a = rng.standard_normal((S, 2)) * (np.asarray(amplitudes) * norm)
    out = np.empty((S,) + P.shape)
    for s in range(S):
        shape = P + a[s, 0] * m1 + a[s, 1] * m2
        out[s] = shape @ random_rotation(rng).T + 5.0 * size * rng.standard_normal(3)
    return out, P, m1, m2, a


def principal_angles(A, B):
    """The principal angles (radians, ascending) between the spans of the rows of A and of B ((k, n, 3) fields, plain inner
    product)."""
    Qa = np.linalg.qr(A.reshape(len(A), -1).T)[0]
    Qb = np.linalg.qr(B.reshape(len(B), -1).T)[0]
    return np.arccos(np.clip(np.linalg.svd(Qa.T @ Qb, compute_uv=False), -1.0, 1.0))


def vertex_areas(points, faces):
    """The barycentric vertex areas of a triangle mesh in plain numpy: a third of the area of the incident faces."""
    P, F = np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    a = 0.5 * np.linalg.norm(np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]), axis=1)
    return np.bincount(F.ravel(), weights=np.repeat(a, 3), minlength=len(P)) / 3.0
