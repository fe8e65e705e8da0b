"""The surface queries (`pf_surface_closest`, `_distance`, `_signed_distance`, `_winding`, `_raycast`, `_vertex_normals`,
`pf_surface_nd_closest`) on hostile geometry, frames and packet edges: the fixed cases of tests/_hostile_geometry.py, one per
generator x frame - needles down to 1e-13 extents, coincident sheets, soups, an anisotropic blob, parts 1e4 extents apart,
meshes scaled by 2^+-20 and moved 1 to 1e6 extents from the origin - at the triangle counts 1, 63, 64, 65, 4096, 4097, 4600
and the query counts 1, 3, 4, 5, 8, 9, 16, 17, 299.  Each case runs every query kind on one `DeviceSurface` against the
brute-force references by the criteria of tests/_surface_checks.py (those of each unit's own test file), then three
checks that need no reference: a permutation of the queries, a permutation of the faces, and a scaling of everything by a
power of two, which shows any absolute constant in a kernel.  The latter run on every row of 65 536 and 65 537 queries
too, where a wave takes 16 queries instead of 4.  tests/test_hostile_geometry.py checks the generators and the references
themselves on the CPU; the sweeps tests/fuzz_surfaces.py and tests/fuzz_surface_nd.py draw more of the same at random."""
import numpy as np
import pytest

import _hostile_geometry as hg
import _signed_ref as sref
import _surface_checks as sc

POWERS = (-20, -3, 7, 20)


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_every_query_kind_against_the_references(hip, ctx, name):
    mesh, q, kind, dirs, R = sc.fixed_case(name)
    surf = hip.DeviceSurface(mesh[0], mesh[1], ctx=ctx)
    try:
        out = sc.run_all(surf, q, dirs)
        fig = sc.check_against_reference(out, R)
        sc.check_query_order(surf, q, dirs, out, seed=1)
    finally:
        surf.close()
    print(name, mesh[2]["name"], dict(R.figures(), **fig))
    sc.check_face_order(hip, ctx, mesh, q, dirs, out, seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_power_of_two_scaling_changes_no_bit(hip, ctx, name):
    mesh, q, kind, dirs, _ = sc.fixed_case(name)
    surf = hip.DeviceSurface(mesh[0], mesh[1], ctx=ctx)
    try:
        out = sc.run_all(surf, q, dirs)
    finally:
        surf.close()
    for k in POWERS:
        for scale_directions in (True, False):
            sc.check_power_of_two(hip, ctx, mesh, q, dirs, out, k, scale_directions)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(hg.CASES))
def test_nd_closest_pruned_exhaustive_and_brute_force(hip, ctx, name):
    """d = 3, a generic depth (7 or 9) and 16, under the case's own frame: pruned = exhaustive = numpy bit for bit, a
    permutation of the queries, a power of two; on the blobs of 64 chunks and more the pruned run did prune."""
    mesh, q, _, _, _ = sc.fixed_case(name)
    k, s, offset = mesh[2]["frame"] or (0, 1.0, 0.0)
    q = q[:hg.ND_ROWS]
    n_tri = len(sref.fan_triangles(mesh[1]))
    for d in hg.CASES[name][2]:
        coords, faces, qd = hg.embedded_case(mesh, q, d, k, s, offset)
        want = sc.nd_reference(coords, faces, qd)
        stats = sc.check_nd(hip, ctx, coords, faces, qd, want=want, must_prune=name.startswith("blob") and n_tri >= 4096,
                            order_seed=3, pow2_k=POWERS[d % 4])
        print(name, "d =", d, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("n", hg.PACKET_SWITCH)
def test_packet_size_switch_on_every_row(hip, ctx, n):
    """65 536 and 65 537 queries and rays against 128 triangles: no brute force, every row through the query-order,
    face-order and power-of-two checks, in 3 and in 9 dimensions too."""
    mesh, q, dirs = hg.packet_switch_case(n)
    surf = hip.DeviceSurface(mesh[0], mesh[1], ctx=ctx)
    try:
        out = sc.run_all(surf, q, dirs)
        sc.check_query_order(surf, q, dirs, out, seed=4)
    finally:
        surf.close()
    fin = np.isfinite(q).all(axis=1)
    assert np.all(np.isfinite(out["distance"][0][fin])) and np.all(np.isnan(out["distance"][0][~fin]))
    assert np.isfinite(out["ray"][0]).any() and np.isinf(out["ray"][0]).any()
    sc.check_face_order(hip, ctx, mesh, q, dirs, out, seed=5)
    for i, k in enumerate(POWERS):
        sc.check_power_of_two(hip, ctx, mesh, q, dirs, out, k, scale_directions=bool(i % 2))
    for d, k in ((3, -20), (9, 7)):
        coords, faces, qd = hg.embedded_case(mesh, q, d)
        sc.check_nd(hip, ctx, coords, faces, qd, order_seed=6, pow2_k=k)
