"""The hostile-geometry generators (tests/_hostile_geometry.py) and the references of the surface checks
(tests/_surface_checks.py), before any GPU is involved: the same seed gives the same bytes; every tag holds; the
references are themselves exact under power-of-two scaling (so the device's metamorphic checks ask for nothing the
definition does not give); and on the fixed cases of tests/test_surface_hostile.py the references alone keep the caps of
what the comparisons may leave out."""
import numpy as np
import pytest

import _hostile_geometry as hg
import _ray_ref as rr
import _signed_ref as sref
import _surface_checks as sc
import _surface_nd_ref as ndref
from oracle import icp_port


def _bytes(mesh):
    return mesh[0].tobytes() + mesh[1].tobytes()


def _areas2(mesh):
    """|cross|^2 of every fan triangle, in float64 as the device sees them"""
    pts, faces, _ = mesh
    t = sref.fan_triangles(faces)
    cr = np.cross(pts[t[:, 1]] - pts[t[:, 0]], pts[t[:, 2]] - pts[t[:, 0]])
    return np.einsum("ij,ij->i", cr, cr)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_same_seed_same_bytes(name):
    a, b = hg.build_case(name, seed=3), hg.build_case(name, seed=3)
    assert _bytes(a[0]) == _bytes(b[0])
    assert a[0][0].dtype == np.float64 and a[0][1].dtype == np.int32 and a[0][0].flags.c_contiguous and a[0][1].flags.c_contiguous
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    other = hg.build_case(name, seed=4)
    assert other[1].tobytes() != a[1].tobytes() and other[3].tobytes() != a[3].tobytes()
    mesh, q = a[0], a[1]
    for d in (1, 3, 9, 16):
        x, y = hg.embedded_case(mesh, q, d, 3, 1.5, 1e3), hg.embedded_case(mesh, q, d, 3, 1.5, 1e3)
        assert x[0].shape == (len(mesh[0]), d) and x[2].shape == (len(q), d)
        assert x[0].tobytes() == y[0].tobytes() and x[2].tobytes() == y[2].tobytes()
        assert np.array_equal(np.isfinite(x[2]).all(axis=1), np.isfinite(q).all(axis=1))


def test_generators_differ_by_seed_and_packet_switch_sizes():
    assert _bytes(hg.soup(40, 65, 3, 1)) != _bytes(hg.soup(40, 65, 3, 2))
    assert _bytes(hg.slivers(hg.blob(100), 0.05, 1e-9, 1)) != _bytes(hg.slivers(hg.blob(100), 0.05, 1e-9, 2))
    for n in hg.PACKET_SWITCH:
        mesh, q, d = hg.packet_switch_case(n)
        assert len(sref.fan_triangles(mesh[1])) <= 128 and q.shape == d.shape == (n, 3)
        assert np.sum(~np.isfinite(q).all(axis=1)) == 2


def test_sizes_reach_every_structure():
    counts = {len(sref.fan_triangles(hg.CASES[name][0]()[1])) for name in hg.CASES}
    assert counts >= set(hg.TRIANGLE_COUNTS)
    assert {hg.CASES[name][1] for name in hg.CASES} == set(hg.QUERY_COUNTS)
    assert 257 <= max(hg.QUERY_COUNTS) <= 300


# ------------------------------------------------------------------------------------------------ tags
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_tags_hold(name):
    mesh = hg.CASES[name][0]()
    pts, faces, tags = mesh
    _, boundary, nonmanifold, inconsistent = sref.topology_counts(faces)
    assert tags["closed_oriented"] == ((boundary, nonmanifold, inconsistent) == (0, 0, 0))
    assert tags["has_degenerate"] == bool(np.any(_areas2(mesh) == 0.0))
    if tags["planar_axis"] is not None:
        t = sref.fan_triangles(faces)
        z = pts[t][:, :, tags["planar_axis"]]
        assert np.all(z == z[:, :1])  # zero thickness: every triangle, so every chunk of one layer
    if tags["has_slivers"]:
        assert tags["folded"] == hg.folded(pts, faces)
    else:
        assert not tags["folded"]
    if tags["coincident"]:
        t = np.sort(pts[sref.fan_triangles(faces)].reshape(-1, 9), axis=1)
        assert len(np.unique(t, axis=0)) < len(t)


@pytest.mark.parametrize("rel", [1e-6, 1e-9, 1e-13])
def test_sliver_heights_and_closedness(rel):
    base = hg.blob(600, 3)
    mesh = hg.slivers(base, 0.05, rel)
    pts, faces, tags = mesh
    assert sref.topology_counts(faces) == sref.topology_counts(base[1]) and np.array_equal(faces, base[1])
    ext = hg.extent(pts, faces)
    edges = tags["sliver_edges"]
    assert len(edges) == round(0.05 * len(faces) / 2)
    length = np.linalg.norm(pts[edges[:, 0]] - pts[edges[:, 1]], axis=1)
    # the moved end is rounded to the grid of coordinates of order 40: a few 1e-15 on a length of rel x extent
    assert np.all(np.abs(length - rel * ext) <= 1e-3 * rel * ext + 64 * np.finfo(np.float64).eps * 40.0)
    needles = 0
    for u, v in edges:
        both = (faces == u).any(axis=1) & (faces == v).any(axis=1)
        assert both.sum() == 2
        needles += 2
        for f in faces[both]:  # the height over the longest edge is at most the collapsed edge's length
            x = pts[f]
            longest = max(np.linalg.norm(x[i] - x[j]) for i, j in ((0, 1), (1, 2), (2, 0)))
            assert np.linalg.norm(np.cross(x[1] - x[0], x[2] - x[0])) / longest <= 1.001 * rel * ext + 1e-12
    assert needles == round(0.05 * len(faces) / 2) * 2
    assert len(np.unique(pts, axis=0)) == len(pts)  # no two points equal
    assert set(tags["fragile"]) == set(edges.ravel())
    assert not tags["folded"] and not hg.folded(pts, faces)  # so the sign is compared on it
    turned = hg.slivers(base, 0.05, rel)[0].copy()
    turned[edges[0, 1]] = 2.0 * turned[edges[0, 0]] - turned[edges[0, 1]]  # one needle through its own apex edge: turned over
    assert hg.folded(turned, faces)


def test_sheets_coincide_exactly_and_rays_stay_off_the_plane():
    mesh = hg.sheets(8, 8, 2, 3)
    pts, faces, tags = mesh
    t = sref.fan_triangles(faces)
    half = len(t) // 2
    assert np.array_equal(pts[t[:half]], pts[t[half:]]) and not np.array_equal(t[:half], t[half:])  # other points, same places
    assert np.all(pts == np.round(pts)) and np.all(pts[:, 2] == 0.0)
    framed = hg.frame(mesh, -3, 1.0, 1e3)
    assert np.array_equal(framed[0][t[:half]], framed[0][t[half:]])  # the frame keeps the coincidences
    q, _ = hg.queries(framed, 299)
    d, kind = hg.rays(framed, q, seed=1)
    assert np.all(np.abs(d[:, 2]) >= 0.1 * np.linalg.norm(d, axis=1) * (1 - 1e-15)) and set(kind) == {0, 1, 2, 3}
    quads = hg.sheets(6, 5, 3, 4)
    assert quads[1].shape == (90, 4) and len(np.unique(quads[0], axis=0)) * 3 == len(quads[0])


def test_far_parts_and_outlier_collapse_the_morton_key():
    a, b = hg.blob(100, 5), hg.blob(150, 6)
    pts, faces, _ = hg.far_parts(a, b)
    total = hg.extent(pts, faces)
    assert hg.extent(a[0]) / total < 2.0 ** -10 and hg.extent(b[0]) / total < 2.0 ** -10  # 10 bits an axis: one cell each
    pts, faces, _ = hg.outlier(hg.blob(200, 7))
    assert hg.extent(pts[:200]) / hg.extent(pts, faces) < 2.0 ** -10 and len(faces) == 397


def test_query_mix_and_ray_kinds():
    mesh = hg.blob(600, 3)
    q, kind = hg.queries(mesh, 299)
    assert len(q) == 299 and [int(np.sum(kind == k)) for k in range(len(hg.KINDS))] == [268, 13, 2, 2, 2, 4, 6, 1, 1]
    dup = q[kind == 6]
    assert all(np.sum(np.all(q == row, axis=1)) >= 2 for row in dup)
    assert np.isnan(q[kind == 7]).any() and np.isinf(q[kind == 8]).any()
    ext = hg.extent(*mesh[:2])
    near = np.sqrt(icp_port.closest_points_on_surface(mesh[0], mesh[1], q[kind == 1])[2])
    assert near.min() < 1e-11 * ext and near.max() > 1e-3 * ext  # from rounding distance to a tenth of the extent
    assert np.all(icp_port.closest_points_on_surface(mesh[0], mesh[1], q[(kind >= 2) & (kind <= 4)])[2] < (1e-14 * ext) ** 2)
    for n in hg.QUERY_COUNTS[:-1]:
        small, _ = hg.queries(mesh, n)
        assert small.shape == (n, 3) and np.all(np.isfinite(small))
    d, rk = hg.rays(mesh, q, seed=1)
    axis = d[rk == 1]
    assert np.all(np.sum(axis != 0.0, axis=1) == 1) and np.signbit(axis).any() and (np.signbit(axis) & (axis == 0.0)).any()
    big = np.abs(d[rk == 3]).max(axis=1)
    assert np.any(big > 2.0 ** 20) and np.any(big < 2.0 ** -20)
    assert np.all(np.isfinite(d)) and np.all(d.any(axis=1))


# ------------------------------------------------------------------------------------------------ references under 2^k
@pytest.mark.parametrize("name", ["torus_quads_2^20_offset_1", "slivers_1e-9", "sheets_coincident", "soup_hexagons_offset_1"])
def test_references_are_exact_under_power_of_two_scaling(name):
    mesh, q, _, d, _ = hg.build_case(name)
    pts, faces, _ = mesh
    q, d = q[:64], d[:64]
    fin = np.isfinite(q).all(axis=1)
    pt, face, d2 = icp_port.closest_points_on_surface(pts, faces, q[fin])
    w = sref.winding_number(pts, faces, q[fin])
    t, rface, uv, count = rr.cast(pts, faces, q, d)
    x, f, y = hg.embedded_case(mesh, q, 7)
    nd = ndref.closest_points_on_surface_nd(x, f, y)
    for k in (-20, -3, 7, 20):
        P, Q = hg.pow2(pts, k), hg.pow2(q, k)
        pt_k, face_k, d2_k = icp_port.closest_points_on_surface(P, faces, Q[fin])
        assert sc.same_bits(pt_k, hg.pow2(pt, k)) and sc.same_bits(d2_k, hg.pow2(d2, 2 * k)) and np.array_equal(face_k, face)
        assert sc.same_bits(sref.winding_number(P, faces, Q[fin]), w)
        for scaled in (True, False):
            got = rr.cast(P, faces, Q, hg.pow2(d, k) if scaled else d)
            assert sc.same_bits(got[0], t if scaled else hg.pow2(t, k))
            assert np.array_equal(got[1], rface) and sc.same_bits(got[2], uv) and np.array_equal(got[3], count)
        nd_k = ndref.closest_points_on_surface_nd(hg.pow2(x, k), f, hg.pow2(y, k))
        for key in ("face", "vertices", "bary"):
            assert sc.same_bits(nd_k[key], nd[key]), key
        assert sc.same_bits(nd_k["d2"], hg.pow2(nd["d2"], 2 * k))


# ------------------------------------------------------------------------------------------------ caps
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_references_alone_keep_the_caps(name):
    mesh, q, kind, dirs, R = sc.fixed_case(name)
    print(name, mesh[2]["name"], R.figures())
    assert R.left_out <= sc.FILTER_CAP and R.ray_left_out <= sc.RAY_CAP
    assert np.all(np.isfinite(R.d2))
    if len(q) >= 32:  # the mix does something: rays hit and miss, queries fall on both sides of a closed surface
        assert np.isfinite(R.ray[0]).any() and np.isinf(R.ray[0]).any()
        if R.sign_keep is not None:
            inside = np.round(R.w[R.sign_keep])
            assert set(inside) == {0.0, 1.0}  # outward faces: 1 inside, 0 outside, and queries on both sides
