"""What "equal" means for the surface queries on hostile inputs - test infrastructure shared by
tests/test_hostile_geometry.py (the references alone, on the CPU), tests/test_surface_hostile.py and the sweeps
tests/fuzz_surfaces.py, tests/fuzz_surface_nd.py.  The criteria are those of each unit's own test file, imported from it
where it has a helper: `test_signed_distance._assert_magnitude_exact`, `test_ray_casting._same`, `test_surface_nd._same`,
`test_winding_number.TOL`.

  closest, distance, nd closest, raycast   bit for bit against the brute-force references; documented sentinels on
                                           non-finite rows
  distance summary                         counts and argmax exact, sums at rtol 1e-12 over the device's own distances, max
                                           within one ulp (tests/test_surface_distance.py)
  signed                                   |sd| and face equal the unsigned call's bit for bit; the sign against the float64
                                           winding reference on `closed_oriented` meshes that are not `folded`, where
                                           |w - round(w)| < 1e-6 and the query is farther than 1e-9 diagonals from the surface
  winding, exact                           TOL + 8 x max |float64 reference - longdouble reference| over the kept queries:
                                           TOL was derived for coordinates of order 1; in a far frame the corner vectors
                                           a - q lose eps x offset before any formula sees them, and the longdouble
                                           evaluation of the same formula on the same float64 inputs measures what float64
                                           can deliver there; 8 allows for the device's other summation order and its FMA
  winding, beta = 2                        |w_beta - w| <= bound + that tolerance
  vertex normals                           16 eps x angle sum + 8 x the float64 restatement's own deviation from longdouble,
                                           on meshes without slivers or degenerate faces only
  rays                                     a ray for which the reference accepts a triangle with sigma = |det| / (|d| |e1|
                                           |e2|) < 1e-6 is left out (pruning is exact for sigma >= 8.2e-8); at most
                                           1 % of a case's rays, past that the case fails
  sign and winding filters together        at most 5 % of a case's finite queries left out"""
import numpy as np

import _hostile_geometry as hg
import _ray_ref as rr
import _signed_ref as sref
import _surface_nd_ref as ndref
from oracle import icp_port

EPS = np.finfo(np.float64).eps
SIGMA_MIN = 1e-6
RAY_CAP = 0.01
FILTER_CAP = 0.05
NEAR = 1e-9      # diagonals: closer than this to the surface w jumps and the sign is not compared
INTEGER = 1e-6   # |w - round(w)| of the float64 reference below which it decides inside / outside


def same_bits(a, b):
    """identical bits, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ longdouble references
def winding_number_longdouble(points, faces, queries, block=32):
    """`_signed_ref.winding_number`'s formula in np.longdouble on the same float64 inputs."""
    L = np.longdouble
    tri = sref.fan_triangles(np.asarray(faces))
    A, B, C = (points[tri[:, j]].astype(L) for j in range(3))
    out = np.empty(len(queries), dtype=L)

    def dot(x, y):
        return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]

    for s in range(0, len(queries), block):
        q = queries[s:s + block, None, :].astype(L)
        a, b, c = A[None] - q, B[None] - q, C[None] - q
        la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
        det = dot(a, np.cross(b, c))
        den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la
        out[s:s + block] = np.sum(L(2) * np.arctan2(det, den), axis=1) / (L(4) * L("3.14159265358979323846264338327950288"))
    return out


def vertex_normals_ref(points, faces, dtype=np.float64):
    """(sum over the corners at a vertex of angle x unit normal, sum of those angles): the restatement of
    tests/test_pool_hygiene.py and tests/test_mesh_units_small.py, in `dtype`."""
    tri = sref.fan_triangles(np.asarray(faces))
    X = points[tri].astype(dtype)

    def norm(x):
        return np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])

    cr = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    tn = cr / norm(cr)[:, None]
    vn, angsum = np.zeros(points.shape, dtype=dtype), np.zeros(len(points), dtype=dtype)
    for j in range(3):
        e1, e2 = X[:, (j + 1) % 3] - X[:, j], X[:, (j + 2) % 3] - X[:, j]
        ang = np.arctan2(norm(np.cross(e1, e2)), e1[:, 0] * e2[:, 0] + e1[:, 1] * e2[:, 1] + e1[:, 2] * e2[:, 2])
        np.add.at(vn, tri[:, j], ang[:, None] * tn)
        np.add.at(angsum, tri[:, j], ang)
    return vn, angsum


def rays_accepted_at_low_sigma(points, faces, origins, directions):
    """bool (n,): rays for which the reference's exact test accepts a fan triangle with sigma < SIGMA_MIN (or a sigma that
    is not a number: a zero edge)."""
    tri = sref.fan_triangles(np.asarray(faces))
    a, b, c = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    e1, e2 = b - a, c - a
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    out = np.zeros(len(origins), dtype=bool)
    valid = np.isfinite(origins).all(axis=1) & np.isfinite(directions).all(axis=1) & directions.any(axis=1)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(valid):
            d = directions[i] / np.max(np.abs(directions[i]))  # (sigma does not depend on |d|; keeps 2^+-30 out of the squares)
            det = np.einsum("ij,ij->i", e1, np.cross(d, e2))
            sigma = np.abs(det) / (np.linalg.norm(d) * l1 * l2)
            low = np.flatnonzero(~(sigma >= SIGMA_MIN))
            if len(low):
                out[i] = rr.cast(points, tri[low], origins[i:i + 1], directions[i:i + 1])[3][0] > 0
    return out


# ------------------------------------------------------------------------------------------------ the references of a case
class Reference(object):
    """Everything the checks compare against, from the CPU alone, for one mesh, its queries and ray directions; computed
    once and left unchanged.  `left_out` / `ray_left_out` are the shares the filters drop, `within_caps()` the caps."""

    def __init__(self, mesh, q, dirs, winding=True, rays=True):
        import test_winding_number as tw

        pts, faces, tags = mesh
        self.mesh, self.q, self.dirs = mesh, q, dirs
        self.finite = np.isfinite(q).all(axis=1)
        qf = q[self.finite]
        self.pt, self.face, self.d2 = icp_port.closest_points_on_surface(pts, faces, qf)
        assert np.all(np.isfinite(self.d2)), "a finite query without a finite distance: a defect of the generator"
        self.diag = hg.diagonal(pts, faces)
        self.off = np.sqrt(self.d2) >= NEAR * self.diag
        self.compare_sign = bool(tags["closed_oriented"]) and not tags["folded"]
        self.compare_normals = not (tags["has_slivers"] or tags["has_degenerate"])
        self.w = self.w_tol = self.sign_keep = None
        self.left_out = float(np.mean(~self.off)) if len(qf) else 0.0
        if winding:
            self.w = sref.winding_number(pts, faces, qf)
            w_ld = winding_number_longdouble(pts, faces, qf)
            dev = np.abs((self.w.astype(np.longdouble) - w_ld).astype(np.float64))
            self.w_dev = float(dev[self.off].max()) if self.off.any() else 0.0
            self.w_tol = tw.TOL + 8.0 * self.w_dev
            if self.compare_sign:
                self.sign_keep = self.off & (np.abs(self.w - np.round(self.w)) < INTEGER)
                self.left_out = float(np.mean(~self.sign_keep)) if len(qf) else 0.0
                # the generators' closed meshes are outward: w is 1 inside (tests/test_hostile_geometry.py asserts it on the
                # fixed cases).  A host volume sum would tell too, but not for parts 1e5 extents apart: it cancels.
                assert np.all(np.isin(np.round(self.w[self.sign_keep]), (0.0, 1.0))), "closed_oriented promises outward faces"
        self.ray = self.ray_keep = None
        self.ray_left_out = 0.0
        if rays:
            self.ray = rr.cast(pts, faces, q, dirs)
            low = rays_accepted_at_low_sigma(pts, faces, q, dirs)
            valid = ~np.isnan(self.ray[0])
            self.ray_keep = ~low
            self.ray_left_out = float(low.sum()) / max(1, int(valid.sum()))
        if self.compare_normals:
            self.vn, self.angsum = vertex_normals_ref(pts, faces)
            vn_ld, _ = vertex_normals_ref(pts, faces, np.longdouble)
            self.vn_dev = float(np.max(np.abs((self.vn.astype(np.longdouble) - vn_ld).astype(np.float64))))

    def within_caps(self):
        return self.left_out <= FILTER_CAP and self.ray_left_out <= RAY_CAP

    def figures(self):
        out = {"left_out": self.left_out, "ray_left_out": self.ray_left_out}
        if self.w_tol is not None:
            out["w_tol"] = self.w_tol
        if self.compare_normals:
            out["vn_dev"] = self.vn_dev
        return out


# ------------------------------------------------------------------------------------------------ device runs
def run_all(surf, q, dirs, normals=True):
    """Every query kind of one open DeviceSurface: name -> tuple of per-query arrays; "stats", "amb" apart."""
    out = {"closest": surf.closest(q)}
    d2, face, out["stats"] = surf.distance(q)
    out["distance"] = (d2, face)
    sd, sface, feature, out["amb"] = surf.signed_distance(q)
    out["signed"] = (sd, sface, feature)
    out["winding"] = surf.winding_number(q)
    out["winding_beta"] = surf.winding_number(q, beta=2.0)
    out["ray"] = surf.raycast(q, dirs)
    out["ray_count"] = surf.raycast(q, dirs, count=True)
    if normals:
        out["normals"] = surf.vertex_normals()
    return out


PER_QUERY = ("closest", "distance", "signed", "winding", "ray", "ray_count")  # (winding_beta: its packets follow the order)


def check_against_reference(out, R):
    """Section by section the criteria of the module docstring; returns the figures measured on the way."""
    import test_ray_casting as trc
    import test_signed_distance as tsd

    q, fin = R.q, R.finite
    nan_row = np.isnan(q).any(axis=1)
    fig = {}
    # closest and distance: bits
    cpt, cface, cd2 = out["closest"]
    d2, face = out["distance"]
    assert np.array_equal(cd2[fin], R.d2) and np.array_equal(cface[fin], R.face) and np.array_equal(cpt[fin], R.pt), "closest"
    assert np.all(cface[nan_row] == -1) and np.all(np.isnan(cpt[nan_row])), "closest: NaN query"
    assert np.array_equal(d2[fin], R.d2) and np.array_equal(face[fin], R.face), "distance"
    assert np.all(np.isnan(d2[~fin])) and np.all(face[~fin] == -1), "distance: non-finite query"
    # the summary: tests/test_surface_distance.py
    st = out["stats"]
    dist = np.sqrt(d2[fin])
    assert st["n_nan"] == int(np.sum(~fin)) and st["n_finite"] == int(fin.sum()), "summary counts"
    if fin.any():
        np.testing.assert_allclose(st["sum_d"], dist.sum(), rtol=1e-12)
        np.testing.assert_allclose(st["sum_d2"], np.sum(dist * dist), rtol=1e-12)
        assert abs(st["max_d"] - dist.max()) <= np.spacing(dist.max()), "summary max"
        assert st["argmax"] == np.flatnonzero(fin)[np.argmax(dist)], "summary argmax"
    else:
        assert st["argmax"] == -1
    # signed: magnitude and face are the unsigned call's; the sign where the reference can tell
    sd, sface, feature = out["signed"]
    tsd._assert_magnitude_exact(sd, sface, d2, face)
    assert np.all(feature[~fin] == -1) and np.all((feature[fin] >= 0) & (feature[fin] <= 2)), "feature"
    amb = out["amb"]
    fig["ambiguous"] = amb
    if R.sign_keep is not None and fin.any():
        wrong = ((sd[fin] < 0) != (np.round(R.w) == 1.0)) & R.sign_keep
        # a row the device counts as ambiguous comes back positive, whatever its side: such rows are left out
        assert wrong.sum() <= amb and np.all(sd[fin][wrong] > 0), ("sign", int(wrong.sum()), amb)
        fig["left_out_with_ambiguous"] = R.left_out + amb / float(fin.sum())
        assert fig["left_out_with_ambiguous"] <= FILTER_CAP, ("sign and winding filters", fig["left_out_with_ambiguous"])
    # winding
    if R.w is not None and fin.any():
        w, bound = out["winding"]
        assert np.all(bound[fin] == 0.0) and np.all(np.isnan(w[~fin])) and np.all(np.isnan(bound[~fin])), "winding sentinels"
        err = np.abs(w[fin] - R.w)[R.off]
        fig["w_err"] = float(err.max()) if len(err) else 0.0
        assert fig["w_err"] <= R.w_tol, ("winding", fig["w_err"], R.w_tol)
        wb, bb = out["winding_beta"]
        assert np.all(bb[fin] >= 0.0) and np.all(np.isnan(wb[~fin])), "winding beta sentinels"
        assert np.all((np.abs(wb[fin] - R.w) <= bb[fin] + R.w_tol)[R.off]), "winding beta"
    # rays
    if R.ray is not None:
        keep = R.ray_keep
        assert R.ray_left_out <= RAY_CAP, ("rays left out", R.ray_left_out)
        trc._same(tuple(g[keep] for g in out["ray_count"]), tuple(x[keep] for x in R.ray))
        trc._same(tuple(g[keep] for g in out["ray"]), tuple(x[keep] for x in R.ray[:3]))
    # vertex normals
    if R.compare_normals and "normals" in out:
        err = np.abs(out["normals"] - R.vn)
        fig["vn_err_over_allowance"] = float(np.max(err / (16 * EPS * R.angsum[:, None] + 8 * R.vn_dev + np.finfo(np.float64).tiny)))
        assert np.all(err <= 16 * EPS * R.angsum[:, None] + 8 * R.vn_dev), ("vertex normals", float(err.max()))
    return fig


def check_query_order(surf, q, dirs, out, seed=0):
    """A permutation of the queries permutes every per-query output and changes no bit; the summary keeps to its own
    criterion (counts and the maximum exact, the argmax one of the rows that attain it, the sums at 1e-12)."""
    perm = np.random.default_rng(seed).permutation(len(q))
    again = run_all(surf, np.ascontiguousarray(q[perm]), np.ascontiguousarray(dirs[perm]), normals=False)
    for name in PER_QUERY:
        for k, (g, w) in enumerate(zip(again[name], out[name])):
            assert same_bits(g, w[perm]), ("query order", name, k)
    a, b = again["stats"], out["stats"]
    assert a["n_finite"] == b["n_finite"] and a["n_nan"] == b["n_nan"] and a["max_d"] == b["max_d"] and again["amb"] == out["amb"]
    if b["argmax"] >= 0:
        d2 = out["distance"][0]
        assert d2[perm[a["argmax"]]] == d2[b["argmax"]], "query order: argmax"
        np.testing.assert_allclose(a["sum_d"], b["sum_d"], rtol=1e-12)
        np.testing.assert_allclose(a["sum_d2"], b["sum_d2"], rtol=1e-12)


def check_face_order(hip, ctx, mesh, q, dirs, out, seed=0):
    """A permutation of the faces leaves every d2, every t and every count bit-identical; a face index may change only to
    another face at exactly the same d2 / t (checked with the reference on that one face)."""
    pts, faces, _ = mesh
    perm = np.random.default_rng(seed).permutation(len(faces))
    surf = hip.DeviceSurface(pts, np.ascontiguousarray(faces[perm]), ctx=ctx)
    try:
        cpt, cface, cd2 = surf.closest(q)
        d2, face, _ = surf.distance(q)
        sd, sface, _, _ = surf.signed_distance(q)
        t, rface, _, count = surf.raycast(q, dirs, count=True)
    finally:
        surf.close()
    assert same_bits(cd2, out["closest"][2]) and same_bits(d2, out["distance"][0]), "face order: d2"
    assert same_bits(np.abs(sd), np.abs(out["signed"][0])), "face order: |sd|"
    # (by value: +0.0 and -0.0 from two triangles around an origin on the surface tie, and the order decides between them)
    assert np.array_equal(t, out["ray_count"][0], equal_nan=True) and np.array_equal(count, out["ray_count"][3]), "face order: t, count"
    for got, want in ((cface, out["closest"][1]), (face, out["distance"][1]), (sface, out["signed"][1])):
        back = np.where(got >= 0, perm[np.maximum(got, 0)], -1)
        for i in np.flatnonzero((back != want) & np.isfinite(q).all(axis=1)):
            assert want[i] >= 0 and back[i] >= 0
            _, _, tie = icp_port.closest_points_on_surface(pts, faces[[back[i]]], q[i:i + 1])
            assert tie[0] == out["distance"][0][i], ("face order: another face that does not tie", i)
    back = np.where(rface >= 0, perm[np.maximum(rface, 0)], -1)
    for i in np.flatnonzero(back != out["ray_count"][1]):
        assert rr.cast(pts, faces[[back[i]]], q[i:i + 1], dirs[i:i + 1])[0][0] == t[i], ("face order: a hit that does not tie", i)


def check_power_of_two(hip, ctx, mesh, q, dirs, out, k, scale_directions):
    """mesh and queries x 2^k: d2 x 4^k, sd, closest points and the summary's sums x 2^k bit for bit; faces, features,
    counts, winding numbers, (u, v) and vertex normals identical; t identical when the directions are scaled too, x 2^k
    when they are not."""
    pts, faces, _ = mesh
    surf = hip.DeviceSurface(hg.pow2(pts, k), faces, ctx=ctx)
    try:
        got = run_all(surf, hg.pow2(q, k), hg.pow2(dirs, k) if scale_directions else dirs)
    finally:
        surf.close()
    what = "2^%d" % k
    cpt, cface, cd2 = out["closest"]
    assert same_bits(got["closest"][0], hg.pow2(cpt, k)) and same_bits(got["closest"][2], hg.pow2(cd2, 2 * k)), (what, "closest")
    assert np.array_equal(got["closest"][1], cface), (what, "closest face")
    assert same_bits(got["distance"][0], hg.pow2(out["distance"][0], 2 * k)), (what, "distance")
    assert np.array_equal(got["distance"][1], out["distance"][1]), (what, "distance face")
    a, b = got["stats"], out["stats"]
    assert (a["n_finite"], a["n_nan"], a["argmax"]) == (b["n_finite"], b["n_nan"], b["argmax"]), (what, "summary")
    assert a["sum_d"] == np.ldexp(b["sum_d"], k) and a["sum_d2"] == np.ldexp(b["sum_d2"], 2 * k), (what, "summary sums")
    assert a["max_d"] == np.ldexp(b["max_d"], k), (what, "summary max")
    assert same_bits(got["signed"][0], hg.pow2(out["signed"][0], k)) and got["amb"] == out["amb"], (what, "signed")
    assert np.array_equal(got["signed"][1], out["signed"][1]) and np.array_equal(got["signed"][2], out["signed"][2]), (what, "signed")
    assert same_bits(got["winding"][0], out["winding"][0]), (what, "winding")
    for name in ("ray", "ray_count"):
        t = out[name][0] if scale_directions else hg.pow2(out[name][0], k)
        assert same_bits(got[name][0], t), (what, name, "t")
        for g, w in zip(got[name][1:], out[name][1:]):
            assert same_bits(g, w), (what, name)
    assert same_bits(got["normals"], out["normals"]), (what, "normals")


# ------------------------------------------------------------------------------------------------ d dimensions
ND_KEYS = ("face", "vertices", "bary", "d2")


def run_nd(surface, q):
    """(pruned, its last_search, exhaustive, its last_search) as dicts of `ND_KEYS`"""
    pruned = dict(zip(ND_KEYS, surface.closest(q)))
    stats = surface.last_search()
    exhaustive = dict(zip(ND_KEYS, surface.closest(q, exhaustive=True)))
    return pruned, stats, exhaustive, surface.last_search()


def check_nd(hip, ctx, coords, faces, q, want=None, must_prune=False, order_seed=None, pow2_k=None):
    """Pruned = exhaustive = the numpy brute force (`want`, if given) bit for bit by `test_surface_nd._same`; the
    exhaustive run staged every chunk for every packet, the pruned one fewer where `must_prune`; with `order_seed` a
    permutation of the queries permutes the outputs of both modes; with `pow2_k` everything x 2^k: face, corners and
    weights identical, d2 x 4^k."""
    import test_surface_nd as tnd

    with hip.DeviceSurfaceND(coords, faces, ctx=ctx) as surface:
        pruned, stats, exhaustive, stats_ex = run_nd(surface, q)
        tnd._same(pruned, exhaustive)
        if want is not None:
            tnd._same(pruned, want)
        n_chunks = (len(sref.fan_triangles(faces)) + 63) // 64
        assert stats["packets"] == (len(q) + 7) // 8 and stats["n_chunks"] == n_chunks, stats
        assert stats_ex["chunks_opened"] == stats["packets"] * n_chunks, stats_ex
        assert 0 <= stats["chunks_opened"] <= stats["packets"] * n_chunks, stats
        if must_prune:
            assert stats["chunks_opened"] < stats["packets"] * n_chunks, ("the pruned search did not prune", stats)
        if order_seed is not None:
            perm = np.random.default_rng(order_seed).permutation(len(q))
            p2, _, e2, _ = run_nd(surface, np.ascontiguousarray(q[perm]))
            tnd._same(p2, {key: pruned[key][perm] for key in ND_KEYS})
            tnd._same(e2, {key: pruned[key][perm] for key in ND_KEYS})
    if pow2_k is not None:
        with hip.DeviceSurfaceND(hg.pow2(coords, pow2_k), faces, ctx=ctx) as surface:
            scaled = dict(zip(ND_KEYS, surface.closest(hg.pow2(q, pow2_k))))
        tnd._same(scaled, dict(pruned, d2=hg.pow2(pruned["d2"], 2 * pow2_k)))
    return stats


def nd_reference(coords, faces, q):
    return ndref.closest_points_on_surface_nd(coords, faces, q)


_case_cache = {}


def fixed_case(name):
    """(mesh, q, kind, dirs, Reference) of `_hostile_geometry.CASES[name]`, computed once and left unchanged."""
    if name not in _case_cache:
        mesh, q, kind, dirs, _ = hg.build_case(name)
        _case_cache[name] = (mesh, q, kind, dirs, Reference(mesh, q, dirs))
    return _case_cache[name]
