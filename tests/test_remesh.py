"""Uniform mesh resampling by clustering (`pf_mesh_cluster`, `pyfocusr_amd.remesh`).

CPU: the cluster helpers on hand-made labels, argument errors before the library is loaded, the declaration, and the numpy
reference `_remesh_ref` on three blobs whose dual must be one closed orientable sphere of 2 m - 4 faces.  GPU: every
output of the device equal (`np.array_equal`: integers and bits) to the reference on the same points, faces, masses and
seeds - single update and assignment steps on shapes chosen for the paths they take, the whole call, the vote rule on a
hand-made fold, the error codes - and `resample_mesh` end to end.  Masses come from numpy so that bits can match."""
import os
import re

import numpy as np
import pytest

import _fps_ref
import _remesh_ref as rr
import _topology_ref as tref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, m, the iterations the definition takes on blob_mesh(n, seed=1) from farthest-point seeds)
BLOBS = {"700to100": (700, 100, 4), "5000to500": (5000, 500, 7), "5000to60": (5000, 60, 26)}
_cache = {}


def _frozen(d):
    for v in d.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


def blob(n):
    """(points, faces, numpy vertex areas) of blob_mesh(n, seed=1), computed once."""
    if ("blob", n) not in _cache:
        from pyfocusr_amd.meshgen import blob_mesh

        mesh = blob_mesh(n, seed=1)
        P, F = np.ascontiguousarray(mesh.points, dtype=np.float64), np.ascontiguousarray(mesh.faces, dtype=np.int32)
        _cache[("blob", n)] = tuple(_frozen({"P": P, "F": F, "a": rr.vertex_areas(P, F)}).values())
    return _cache[("blob", n)]


def case(n, m, n_iter):
    """(points, faces, masses, seeds, reference) of a blob case, computed once and never changed."""
    if (n, m, n_iter) not in _cache:
        P, F, a = blob(n)
        sel = _fps_ref.fps(P, m)[0]
        sel.setflags(write=False)
        _cache[(n, m, n_iter)] = (P, F, a, sel, _frozen(rr.cluster(P, F, a, sel, n_iter)))
    return _cache[(n, m, n_iter)]


# ------------------------------------------------------------------------------ CPU
def test_entry_point_is_declared_and_bound():
    import pyfocusr_amd
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    m = re.search(r"int\s+pf_mesh_cluster\s*\(([^)]*)\)\s*;", header)
    assert m, "pf_mesh_cluster is not declared in the header"
    assert len(m.group(1).split(",")) == 22
    assert len(_hip.SIGNATURES["pf_mesh_cluster"][1]) == 22
    assert callable(_hip.Context.cluster_mesh)
    for name in ("resample_mesh", "restrict_to_clusters", "prolong_from_clusters", "lift_point_map"):
        assert callable(getattr(pyfocusr_amd, name))
    assert "not geodesic" in pyfocusr_amd.remesh.__doc__ and "not guaranteed to be manifold" in pyfocusr_amd.remesh.__doc__


def test_cluster_helpers_on_hand_made_labels():
    from pyfocusr_amd import lift_point_map, prolong_from_clusters, restrict_to_clusters

    labels = np.array([2, 0, 0, 2, 1, 0, -1])
    mass = np.array([1.0, 1.0, 3.0, 0.0, 2.0, 0.0, 5.0])
    values = np.array([10.0, 1.0, 2.0, 99.0, -4.0, 50.0, 7.0])
    got = restrict_to_clusters(values, labels, mass, 4)
    assert got.shape == (4,) and np.array_equal(got[:3], [(1.0 + 6.0) / 4.0, -4.0, 10.0]) and np.isnan(got[3])
    vec = np.stack([values, 2.0 * values], axis=1)
    got2 = restrict_to_clusters(vec, labels, mass, 4)
    assert got2.shape == (4, 2) and np.array_equal(got2[:3, 1], 2.0 * got[:3])
    with pytest.raises(ValueError):
        restrict_to_clusters(values, labels, mass, 2)
    with pytest.raises(ValueError):
        restrict_to_clusters(values[:3], labels, mass, 4)

    coarse = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    assert np.array_equal(prolong_from_clusters(coarse, labels[:6]), coarse[[2, 0, 0, 2, 1, 0]])
    with pytest.raises(ValueError):
        prolong_from_clusters(coarse, labels)  # -1: a dropped cluster has no value

    T_coarse = np.array([1, 2, 0])           # coarse source j -> coarse target T_coarse[j]
    rep_target = np.array([40, 7, 19])       # the fine vertex behind each coarse target vertex
    lifted = lift_point_map(T_coarse, labels[:6], rep_target)
    assert lifted.dtype == np.int64 and lifted.tolist() == [40, 7, 7, 40, 19, 7]
    for bad in ((T_coarse, labels, rep_target), (np.array([1, 2, 3]), labels[:6], rep_target),
                (T_coarse, labels[:6], np.array([40, -1, 19])), (T_coarse.astype(float), labels[:6], rep_target)):
        with pytest.raises(ValueError):
            lift_point_map(*bad)


def test_argument_errors_before_the_library_is_loaded(monkeypatch):
    from pyfocusr_amd import PolyMesh, _hip, resample_mesh

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(_hip, "default_context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    pts, faces = tref.tetrahedron()
    pts, faces = np.asarray(pts, dtype=np.float64), np.asarray(faces, dtype=np.int32)
    mesh = PolyMesh(pts, faces)
    nan = pts.copy()
    nan[2, 1] = np.nan
    bad = [dict(n_vertices=0), dict(n_vertices=5), dict(n_vertices=2.5), dict(n_vertices=2, n_iter=-1),
           dict(n_vertices=2, placement="nearest"), dict(n_vertices=2, point_data="sum"), dict(n_vertices=2, mass=np.ones(3)),
           dict(n_vertices=2, mass=np.array([1.0, -1.0, 1.0, 1.0])), dict(n_vertices=2, mass=np.array([1.0, np.inf, 1.0, 1.0])),
           dict(n_vertices=2, seeds=[0, 4]), dict(n_vertices=2, seeds=[0, 1, 2]), dict(n_vertices=2, seeds=[0.0, 1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            resample_mesh(mesh, **kw)
    for broken in ((pts, np.array([[0, 1, 2, 3]], dtype=np.int32)), (pts, faces[:0]), (pts[:3], faces), (nan, faces)):
        with pytest.raises(ValueError):
            resample_mesh(broken, 2)
    big = np.zeros((2**21, 3))
    with pytest.raises(ValueError, match="2\\^21"):
        resample_mesh((big, faces), 2**21)


@pytest.mark.parametrize("name", sorted(BLOBS))
def test_reference_dual_is_a_closed_sphere(name):
    n, m, iterations = BLOBS[name]
    _, _, _, _, r = case(n, m, 40)
    assert r["n_iter_run"] == iterations and r["changed"][-1] == 0 and np.all(r["changed"][:-1] > 0)
    assert len(r["faces"]) == 2 * m - 4 == r["n_candidates"]
    assert np.all(r["count"] > 0) and r["count"].sum() == n and np.all(r["rep"] >= 0)
    assert np.array_equal(r["labels"][r["rep"]], np.arange(m))
    assert np.all(r["votes"][:, 0] >= 1) and not r["votes"][:, 1].any()          # no mixed votes
    assert np.array_equal(np.unique(r["faces"]), np.arange(m))                    # every cluster is used
    if name == "5000to60":
        assert r["count"].max() > 2 * rr.RUN  # three runs in one cluster: the two-level sum is exercised
    topo = tref.topology(m, r["faces"], r["centroids"], outward=True)
    assert topo["n_patches"] == 1 and topo["n_boundary_edges"] == 0 and topo["n_nonmanifold_edges"] == 0
    assert topo["n_inconsistent_edges"] == 0 and not topo["flip"].any()
    p = topo["patches"]
    assert p["closed"][0] and p["orientable"][0] and p["genus"][0] == 0 and p["n_faces"][0] == 2 * m - 4


def test_reference_two_level_sum_is_the_plain_sum_up_to_64_members():
    rng = np.random.default_rng(5)
    P, a = rng.standard_normal((200, 3)), rng.random(200)
    labels = np.repeat(np.arange(4), [64, 63, 72, 1]).astype(np.int32)[rng.permutation(200)]
    C = rr.update(P, a, labels, np.zeros((4, 3)))
    for j in range(4):
        members = np.flatnonzero(labels == j)
        num, den = np.zeros(3), 0.0
        if j == 2:  # 72 members: 64 and 8, then the two run sums
            parts = [(members[:64]), (members[64:])]
        else:
            parts = [members]
        run_sums = []
        for part in parts:
            s, d = np.zeros(3), 0.0
            for i in part:
                s, d = s + a[i] * P[i], d + a[i]
            run_sums.append((s, d))
        for s, d in run_sums:
            num, den = num + s, den + d
        assert np.array_equal(C[j], num / den)


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip.default_context()


def _assert_equals_reference(dev, r, what):
    for key in ("labels", "rep", "count", "changed", "faces", "face_src", "votes"):
        assert dev[key].dtype == np.int32 and np.array_equal(dev[key], r[key]), (what, key)
    assert dev["centroids"].tobytes() == r["centroids"].tobytes(), (what, "centroids")
    assert dev["n_iter_run"] == r["n_iter_run"] and dev["n_candidate_faces"] == r["n_candidates"], what


def _update_case():
    """Clusters of 64, 65, 129 and 7 members, an empty one and one of zero-mass vertices only, members interleaved."""
    rng = np.random.default_rng(11)
    sizes = [64, 65, 129, 0, 5, 7]
    n = sum(sizes)
    labels = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)[rng.permutation(n)]
    P = rng.standard_normal((n, 3)) * [1.0, 20.0, 0.05] + [100.0, -3.0, 0.0]
    a = rng.random(n) + 0.01
    a[labels == 4] = 0.0
    a[np.flatnonzero(labels == 2)[:3]] = 0.0  # zero masses inside a cluster that has others
    return P, a, labels, rng.standard_normal((len(sizes), 3))


@pytest.mark.gpu
def test_one_update_step_gives_the_centroids_bit_for_bit(ctx):
    P, a, labels, C0 = _update_case()
    want = rr.update(P, a, labels, C0)
    assert np.array_equal(want[3], C0[3]) and np.array_equal(want[4], C0[4])  # the two clusters without mass keep theirs
    dev = ctx.cluster_mesh(P, None, a, centroids=C0, labels=labels, n_iter=1, update_only=True)
    assert dev["centroids"].tobytes() == want.tobytes()
    assert np.array_equal(dev["labels"], labels) and dev["count"].tolist() == [64, 65, 129, 0, 5, 7]
    rep, _ = rr.representatives(P, want, labels)
    assert np.array_equal(dev["rep"], rep) and rep[3] == -1
    assert len(dev["faces"]) == 0 and len(dev["changed"]) == 0


def _assign_cases():
    P, _, _ = blob(700)
    rng = np.random.default_rng(3)
    flat, _ = rr.grid_mesh(20, 20)
    line = np.stack([np.linspace(-2.0, 5.0, 300), np.full(300, 1.5), np.full(300, -0.25)], axis=1)
    coincident = P[rng.choice(700, 40, replace=False)].copy()
    coincident[31] = coincident[4]   # two centroids in one place: the lower index wins
    coincident[17] = coincident[22]
    return {
        "blob": (P, P[rng.choice(700, 90, replace=False)] + 0.01 * rng.standard_normal((90, 3))),
        "blob_one_centroid": (P, P[5:6].copy()),
        "blob_many_centroids": (P, P[::2] + 1e-3),                                # m = n / 2: about one centroid per cell
        "flat_grid": (flat, flat[rng.choice(400, 37, replace=False)] + [0.05, -0.02, 0.0]),     # z has no extent
        "flat_grid_centroids_off_plane": (flat, flat[rng.choice(400, 37, replace=False)] + rng.standard_normal((37, 3))),
        "line": (line, line[rng.choice(300, 25, replace=False)] + [0.003, 0.0, 0.0]),          # one axis with an extent
        "line_against_blob_centroids": (line, P[rng.choice(700, 50, replace=False)]),
        "all_centroids_in_one_place": (P[:100], np.repeat(P[3:4], 6, axis=0)),                 # no axis has an extent
        "coincident_centroids": (P, coincident),
        "centroids_far_outside": (P, 50.0 + 3.0 * rng.standard_normal((60, 3))),
        "points_far_outside": (P * 40.0, rng.standard_normal((60, 3)) * [1.0, 1.0, 1e-3]),     # a thin grid, points beyond it
    }


_ASSIGN = None  # built on first use: the blob costs a moment


def _assign_case(name):
    global _ASSIGN
    if _ASSIGN is None:
        _ASSIGN = _assign_cases()
    return _ASSIGN[name]


ASSIGN_NAMES = ["blob", "blob_one_centroid", "blob_many_centroids", "flat_grid", "flat_grid_centroids_off_plane", "line",
                "line_against_blob_centroids", "all_centroids_in_one_place", "coincident_centroids", "centroids_far_outside",
                "points_far_outside"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ASSIGN_NAMES)
def test_one_assignment_step_equals_brute_force(ctx, name):
    P, C = _assign_case(name)
    P, C = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    want, _ = rr.assign(P, C)
    dx, dy, dz = (P[:, None, x] - C[None, :, x] for x in range(3))
    worst = np.argmax((dx * dx + dy * dy) + dz * dz, axis=1).astype(np.int32)  # the warm start must not matter
    mass = np.ones(len(P))
    for warm in (None, worst, want):
        dev = ctx.cluster_mesh(P, None, mass, centroids=C, labels=warm, n_iter=0)
        assert np.array_equal(dev["labels"], want), (name, int(np.count_nonzero(dev["labels"] != want)))
        assert dev["centroids"].tobytes() == C.tobytes() and dev["n_iter_run"] == 0
    rep, count = rr.representatives(P, C, want)
    assert np.array_equal(dev["rep"], rep) and np.array_equal(dev["count"], count)
    if name == "coincident_centroids":
        assert count[31] == 0 and count[22] == 0 and rep[31] == -1
    print("%s: %d x %d, %d distances evaluated, %d cells" % (name, len(P), len(C), dev["report"][4], dev["report"][3]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BLOBS))
def test_whole_call_equals_the_reference(ctx, name):
    n, m, iterations = BLOBS[name]
    P, F, a, sel, r = case(n, m, 40)
    dev = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=40)
    print("%s: %d iterations, %d faces, %.3f ms on the device, %d distances in %d assignments (brute force: %d)"
          % (name, dev["n_iter_run"], len(dev["faces"]), dev["device_ms"], dev["report"][4], dev["report"][5], dev["report"][5] * n * m))
    assert dev["n_iter_run"] == iterations
    _assert_equals_reference(dev, r, name)


@pytest.mark.gpu
def test_iteration_cap_stops_the_loop(ctx):
    P, F, a, sel, r = case(5000, 60, 3)
    dev = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=3)
    assert dev["n_iter_run"] == 3 and dev["changed"][-1] > 0
    _assert_equals_reference(dev, r, "5000to60 capped at 3")


@pytest.mark.gpu
def test_without_iterations_the_labels_are_the_sampling_owner(ctx):
    from pyfocusr_amd import farthest_point_sampling

    P, F, a = blob(5000)
    sel, owner = farthest_point_sampling(P, 500, return_owner=True, ctx=ctx)
    dev = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=0)
    assert np.array_equal(dev["labels"], owner) and dev["n_iter_run"] == 0 and len(dev["changed"]) == 0
    assert dev["centroids"].tobytes() == P[sel].tobytes()
    assert np.array_equal(dev["rep"], sel)  # a seed is at distance 0 from its own centroid
    _assert_equals_reference(dev, rr.cluster(P, F, a, sel, 0), "T = 0")


@pytest.mark.gpu
def test_every_vertex_a_seed_gives_the_input_faces_back(ctx):
    P, F, a = blob(700)
    sel = np.random.default_rng(2).permutation(700)
    dev = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=5)
    inv = np.empty(700, dtype=np.int64)
    inv[sel] = np.arange(700)
    assert np.array_equal(dev["labels"], inv) and dev["n_iter_run"] == 1 and dev["changed"].tolist() == [0]
    L = inv[F]
    r = np.argmin(L, axis=1)
    rows = np.arange(len(F))
    rotated = np.stack([L[rows, r], L[rows, (r + 1) % 3], L[rows, (r + 2) % 3]], axis=1)
    order = np.lexsort(np.sort(rotated, axis=1).T[::-1])
    assert np.array_equal(dev["faces"], rotated[order]) and np.array_equal(dev["face_src"], order)
    assert np.all(dev["votes"] == [1, 0]) and dev["n_candidate_faces"] == len(F)


@pytest.mark.gpu
def test_one_cluster_gives_no_faces(ctx):
    P, F, a = blob(700)
    dev = ctx.cluster_mesh(P, F, a, seeds=[13], n_iter=4)
    r = rr.cluster(P, F, a, [13], 4)
    assert len(dev["faces"]) == 0 and dev["n_candidate_faces"] == 0 and dev["count"].tolist() == [700]
    _assert_equals_reference(dev, r, "m = 1")  # 700 members: eleven runs


@pytest.mark.gpu
def test_single_steps_at_twenty_thousand_vertices(ctx):
    """blob_mesh(20000, seed=1) -> 2000, three iterations: the reference's state after every step goes into the device's
    single steps.  Integers and bits only; the dual has mixed votes and non-manifold edges here, and that is not judged."""
    P, F, a, sel, r = case(20000, 2000, 3)
    labels, cents = r["label_history"], r["centroid_history"]
    assert len(labels) == 4 and r["n_iter_run"] == 3
    start = ctx.cluster_mesh(P, None, a, seeds=sel, n_iter=0)
    assert np.array_equal(start["labels"], labels[0])
    for t in range(3):
        up = ctx.cluster_mesh(P, None, a, centroids=cents[t], labels=labels[t], n_iter=1, update_only=True)
        assert up["centroids"].tobytes() == cents[t + 1].tobytes(), t
        nxt = ctx.cluster_mesh(P, None, a, centroids=cents[t + 1], labels=labels[t], n_iter=0)
        assert np.array_equal(nxt["labels"], labels[t + 1]), t
        print("step %d: %d distances evaluated for %d x %d" % (t, nxt["report"][4], len(P), len(sel)))
    whole = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=3)
    _assert_equals_reference(whole, r, "20000to2000")
    assert len(r["faces"]) == 3997 and r["n_candidates"] == 4000 and np.count_nonzero(r["votes"][:, 1]) == 2


@pytest.mark.gpu
def test_votes_and_the_tie_rule_on_a_fold(ctx):
    """Nine points, every one its own cluster, so that the faces are label triples: {0, 1, 2} twice one way and once the
    other, {3, 4, 5} once each way with the reversed face first, {6, 7, 8} once one way and twice the other."""
    P = np.random.default_rng(8).standard_normal((9, 3))
    F = np.array([[1, 2, 0], [3, 5, 4], [0, 2, 1], [7, 6, 8], [4, 5, 3], [2, 0, 1], [6, 7, 8], [8, 7, 6]], dtype=np.int32)
    dev = ctx.cluster_mesh(P, F, np.ones(9), seeds=np.arange(9), n_iter=0)
    assert np.array_equal(dev["labels"], np.arange(9))
    assert dev["faces"].tolist() == [[0, 1, 2], [3, 5, 4], [6, 8, 7]]
    assert dev["votes"].tolist() == [[2, 1], [1, 1], [2, 1]]
    assert dev["face_src"].tolist() == [0, 1, 3] and dev["n_candidate_faces"] == 8
    want = rr.dual(F, np.arange(9))
    for key in ("faces", "votes", "face_src"):
        assert np.array_equal(dev[key], want[key])


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(ctx):
    P, F, a, sel, _ = case(5000, 60, 40)
    one, two = ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=40), ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=40)
    for key in sorted(one):
        if key != "device_ms":
            assert np.asarray(one[key]).tobytes() == np.asarray(two[key]).tobytes(), key


@pytest.mark.gpu
def test_library_refuses_bad_input_and_stays_usable(ctx):
    from pyfocusr_amd import _hip

    P, F, a, sel, r = case(700, 100, 40)

    def refused(code, text, **kw):
        args = dict(points=P, faces=F, mass=a, seeds=sel, n_iter=2)
        args.update(kw)
        with pytest.raises(_hip.PfError) as e:
            ctx.cluster_mesh(**args)
        assert e.value.code == code and text in str(e.value), str(e.value)

    twice = F.copy()
    twice[5] = [9, 4, 9]
    refused(_hip.PF_E_DEGENERATE, "face 5 repeats a vertex", faces=twice)
    beyond = F.copy()
    beyond[7, 1] = 700
    refused(-1, "references vertex", faces=beyond)
    refused(-1, "seed 3", seeds=np.r_[sel[:3], 700, sel[4:]])
    refused(-1, "seed 0", seeds=np.r_[-1, sel[1:]])
    nan = P.copy()
    nan[123, 2] = np.nan
    refused(-1, "vertex 123 is not finite", points=nan)
    negative = a.copy()
    negative[77] = -1e-300
    refused(-1, "mass of vertex 77", mass=negative)
    refused(-1, "21 bits", seeds=np.zeros(2**21, dtype=np.int64))
    refused(-1, "outside 1 .. n", seeds=np.zeros(701, dtype=np.int64))
    refused(-1, "labels_in[0]", labels=np.full(700, 100, dtype=np.int32))
    _assert_equals_reference(ctx.cluster_mesh(P, F, a, seeds=sel, n_iter=40), r, "after the refusals")


# ------------------------------------------------------------------------------ GPU: resample_mesh
@pytest.mark.gpu
def test_resample_mesh_end_to_end(ctx):
    from pyfocusr_amd import PolyMesh, mesh_topology, point_to_surface_distances, resample_mesh

    P, F, _ = blob(5000)
    height = np.ascontiguousarray(P[:, 2] * 3.0 + 1.0)
    colour = np.stack([P[:, 0], P[:, 1] ** 2], axis=1)
    mesh = PolyMesh(P.copy(), F.copy(), [("height", height), ("colour", colour)])
    new, info = resample_mesh(mesh, 500, return_info=True, ctx=ctx)
    assert np.array_equal(mesh.points, P) and np.array_equal(mesh.faces, F)  # the input is untouched
    m = len(new.points)
    assert m == 500 and len(new.faces) == 2 * m - 4 and info["n_candidate_faces"] == 996 and not info["votes"][:, 1].any()

    topo = mesh_topology(new, ctx=ctx)
    assert topo.n_patches == 1 and topo.n_boundary_edges == 0 and topo.n_nonmanifold_edges == 0 and not topo.flip.any()
    p = topo.patches
    assert p["closed"][0] and p["orientable"][0] and p["genus"][0] == 0

    # the default masses and seeds: the reference on the masses that were used, from the farthest-point seeds
    sel = _fps_ref.fps(P, 500)[0]
    r = rr.cluster(P, F, info["mass"], sel, 20)
    assert np.array_equal(info["kept"], np.arange(500))
    for key in ("labels", "rep", "count", "changed", "face_src", "votes"):
        assert np.array_equal(info[key], r[key]), key
    assert info["centroids"].tobytes() == r["centroids"].tobytes() and np.array_equal(new.faces, r["faces"])
    assert info["n_iter_run"] == r["n_iter_run"]
    np.testing.assert_allclose(info["mass"], rr.vertex_areas(P, F), rtol=1e-12)

    # "surface": on the input surface, up to rounding
    diagonal = float(np.linalg.norm(P.max(axis=0) - P.min(axis=0)))
    d = point_to_surface_distances(new.points, (P, F), ctx=ctx)[0]
    print("surface placement: max distance to the input surface %.3g of the diagonal" % (d.max() / diagonal))
    assert d.max() <= 1e-9 * diagonal
    off = point_to_surface_distances(info["centroids"], (P, F), ctx=ctx)[0]
    assert off.max() > 1e-6 * diagonal  # the centroids themselves are not on it: the projection did something

    # "vertex": a true sub-sampling; "centroid": the centroids
    by_vertex, info_v = resample_mesh(mesh, 500, placement="vertex", return_info=True, ctx=ctx)
    assert np.array_equal(by_vertex.points, P[info_v["rep"]]) and np.array_equal(info_v["rep"], r["rep"])
    by_centroid = resample_mesh(mesh, 500, placement="centroid", point_data=None, ctx=ctx)
    assert by_centroid.points.tobytes() == r["centroids"].tobytes() and by_centroid.point_data == []

    # the iterations do not raise the energy of the seeds' Voronoi cells
    _, info0 = resample_mesh(mesh, 500, n_iter=0, placement="centroid", return_info=True, ctx=ctx)
    e0 = rr.energy(P, info0["mass"], info0["centroids"], info0["labels"])
    e1 = rr.energy(P, info["mass"], info["centroids"], info["labels"])
    print("energy: %.6g with the seeds' cells, %.6g after %d iterations" % (e0, e1, info["n_iter_run"]))
    assert info0["n_iter_run"] == 0 and e1 <= e0

    # point data: the mass-weighted cluster means
    got = dict(new.point_data)
    den = np.bincount(info["labels"], weights=info["mass"], minlength=m)
    want_h = np.bincount(info["labels"], weights=info["mass"] * height, minlength=m) / den
    want_c = np.stack([np.bincount(info["labels"], weights=info["mass"] * colour[:, c], minlength=m) / den for c in range(2)], axis=1)
    assert got["height"].shape == (m,) and got["colour"].shape == (m, 2)
    np.testing.assert_allclose(got["height"], want_h, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["colour"], want_c, rtol=1e-13, atol=1e-300)


@pytest.mark.gpu
def test_compaction_drops_unused_clusters(ctx):
    """Two seeds in one place: the later one owns nothing, its cluster is dropped and the rest is renumbered."""
    from pyfocusr_amd import resample_mesh

    P, F, a, sel, _ = case(700, 100, 40)
    seeds = sel.copy()
    seeds[40] = seeds[10]
    r = rr.cluster(P, F, a, seeds, 0)
    assert r["count"][40] == 0
    new, info = resample_mesh((P, F), 100, n_iter=0, mass=a, seeds=seeds, placement="vertex", return_info=True, ctx=ctx)
    used = np.zeros(100, dtype=bool)
    used[r["faces"].ravel()] = True
    kept = np.flatnonzero(used & (r["count"] > 0))
    assert 40 not in kept and np.array_equal(info["kept"], kept) and len(new.points) == len(kept)
    new_id = np.full(100, -1)
    new_id[kept] = np.arange(len(kept))
    assert np.array_equal(info["labels"], new_id[r["labels"]]) and np.array_equal(new.faces, new_id[r["faces"]])
    assert np.array_equal(new.points, P[r["rep"][kept]]) and new.faces.min() == 0 and new.faces.max() == len(kept) - 1
    full = resample_mesh((P, F), 100, n_iter=0, mass=a, seeds=seeds, placement="vertex", compact=False, ctx=ctx)
    assert len(full.points) == 100 and np.array_equal(full.faces, r["faces"]) and np.array_equal(full.points[40], P[seeds[40]])


@pytest.mark.gpu
def test_a_coarse_match_lifts_to_the_fine_meshes(ctx):
    """Mesh B is mesh A renumbered, rotated and shifted.  Both are resampled from corresponding seeds, so coarse vertex j
    of A matches coarse vertex j of B; the lifted map puts every fine vertex of A on a vertex of B that lies in the
    cluster of its true match."""
    from pyfocusr_amd import lift_point_map, resample_mesh

    P, F, a = blob(5000)
    rng = np.random.default_rng(21)
    perm = rng.permutation(5000)              # B's vertex k is A's vertex perm[k]
    where = np.empty(5000, dtype=np.int64)    # A's vertex i is B's vertex where[i]: the true match
    where[perm] = np.arange(5000)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    PB = P[perm] @ Q.T + [0.3, -1.1, 0.7]
    FB = where[F].astype(np.int32)
    sel = _fps_ref.fps(P, 500)[0]
    _, A = resample_mesh((P, F), 500, mass=a, seeds=sel, placement="vertex", return_info=True, ctx=ctx)
    _, B = resample_mesh((PB, FB), 500, mass=a[perm], seeds=where[sel], placement="vertex", return_info=True, ctx=ctx)
    assert np.array_equal(A["kept"], np.arange(500)) and np.array_equal(B["kept"], np.arange(500))
    T_coarse = np.arange(500)
    lifted = lift_point_map(T_coarse, A["labels"], B["rep"])
    assert lifted.shape == (5000,) and lifted.dtype == np.int64
    assert np.array_equal(B["labels"][lifted], B["labels"][where])
    # and the landing vertex is as close to the true match as a cluster is wide
    gap = np.linalg.norm(PB[lifted] - PB[where], axis=1)
    radius = np.sqrt(np.max(rr.assign(PB, B["centroids"])[1]))
    assert gap.max() <= 2.0 * radius
