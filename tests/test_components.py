"""Connected components of masks and label maps (`pf_ccl_*`, pyfocusr_amd/components.py).

The CPU tests hold the numpy statement of the definition (tests/_ccl_ref.py) to scipy.ndimage, numbering included, and to a
raster-order flood fill; the GPU tests hold the device to that statement byte for byte, on the smallest shapes at which a
kernel can go wrong: z-lines that end on, cross and start a 64-bit word, more lines than a wave and than a block, as many
words as k_ccl_pack's and k_ccl_hook's blocks take and one more or fewer, extents of 1.  Everything is integers: every
comparison is array_equal plus dtype, and no tolerance appears."""
import os
import re

import numpy as np
import pytest

import _ccl_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNECTIVITIES = (6, 18, 26)


def _random_cases(seed=7):
    """72 (volume, connectivity): 6 shapes with extents 1..8, four densities, three connectivities; values 1..3."""
    rng = np.random.default_rng(seed)
    for _ in range(6):
        shape = tuple(int(e) for e in rng.integers(1, 9, size=3))
        for density in (0.05, 0.31, 0.6, 0.9):
            vol = np.where(rng.random(shape) < density, rng.integers(1, 4, size=shape), 0).astype(np.int32)
            for connectivity in CONNECTIVITIES:
                yield vol, connectivity


def _structure(ndimage, connectivity):
    return ndimage.generate_binary_structure(3, ref.AXES[connectivity])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------------------ the reference, on the CPU
def test_reference_equals_scipy_label_numbering_included():
    ndimage = pytest.importorskip("scipy.ndimage")
    n_cases = n_components = differences = 0
    for vol, connectivity in _random_cases():
        got, n = ref.label(vol, connectivity)
        want, m = ndimage.label(vol, _structure(ndimage, connectivity))
        differences += int(n != m) + int(np.count_nonzero(got != want))
        n_cases, n_components = n_cases + 1, n_components + n
    assert n_cases == 72 and n_components > 100 and differences == 0  # (the cases are not trivial ones)


def test_union_find_reference_equals_the_flood_fill():
    for vol, connectivity in _random_cases(seed=8):
        for mode in ref.MODES:
            got, n = ref.label(vol, connectivity, mode)
            want, m = ref.label_flood(vol, connectivity, mode)
            assert n == m and _same(got, want), (vol.shape, connectivity, mode)


def test_by_value_is_scipy_per_value_renumbered_by_root():
    ndimage = pytest.importorskip("scipy.ndimage")
    for vol, connectivity in _random_cases(seed=9):
        got, n = ref.label(vol, connectivity, "by_value")
        roots, parts = [], []
        for v in np.unique(vol[vol != 0]):
            lab, m = ndimage.label(vol == v, _structure(ndimage, connectivity))
            for c in range(1, m + 1):
                part = lab == c
                parts.append(part)
                roots.append(int(np.flatnonzero(part.reshape(-1))[0]))
        want = np.zeros(vol.shape, dtype=np.int32)
        for number, at in enumerate(np.argsort(roots), start=1):
            want[parts[at]] = number
        assert n == len(parts) and _same(got, want)


def test_background_mode_is_binary_mode_of_the_complement():
    for vol, connectivity in _random_cases(seed=10):
        got, n, t = ref.components(vol, connectivity, "background")
        want, m, u = ref.components((vol == 0).astype(np.int32), connectivity, "binary")
        assert n == m and _same(got, want)
        assert not t["value"].any() and all(_same(t[k], u[k]) for k in t if k != "value")


def test_fill_holes_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    mask = np.random.default_rng(11).random((9, 10, 11)) < 0.6
    filled = ref.fill_holes(mask)
    assert _same(filled, ndimage.binary_fill_holes(mask)) and int(filled.sum() - mask.sum()) > 5
    for connectivity in (18, 26):  # the connectivity is the background's
        want = ndimage.binary_fill_holes(mask, structure=_structure(ndimage, connectivity))
        assert _same(ref.fill_holes(mask, connectivity), want)


def test_statistics_are_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    for vol, connectivity in _random_cases(seed=12):
        comp, n, t = ref.components(vol, connectivity)
        assert [t[k].dtype for k in ("count", "value", "root", "lo", "hi", "border", "sum")] == [
            np.int64, np.int32, np.int32, np.int32, np.int32, np.uint8, np.int64]
        assert t["lo"].shape == t["hi"].shape == t["sum"].shape == (n, 3)
        if not n:
            continue
        index = np.arange(1, n + 1)
        assert np.array_equal(t["count"], ndimage.sum(np.ones(vol.shape), comp, index).astype(np.int64))
        for c, box in enumerate(ndimage.find_objects(comp)):
            assert [s.start for s in box] == t["lo"][c].tolist() and [s.stop - 1 for s in box] == t["hi"][c].tolist()
        mass = np.array(ndimage.center_of_mass(np.ones(vol.shape), comp, index)) * t["count"][:, None]
        assert np.array_equal(np.rint(mass).astype(np.int64), t["sum"]) and np.max(np.abs(mass - t["sum"])) < 1e-6
        flat = comp.reshape(-1)
        assert np.array_equal(t["root"], [np.flatnonzero(flat == c)[0] for c in index])
        assert np.array_equal(t["value"], vol.reshape(-1)[t["root"]])
        inner = np.zeros(vol.shape, dtype=bool)
        inner[1:-1, 1:-1, 1:-1] = True
        assert np.array_equal(t["border"], [int((~inner)[comp == c].any()) for c in index])


def test_checkerboard_and_touching_cubes():
    i, j, k = np.indices((6, 7, 8))
    board = ((i + j + k) % 2 == 0).astype(np.int32)
    assert [ref.label(board, c)[1] for c in CONNECTIVITIES] == [6 * 7 * 8 // 2, 1, 1]
    for name, want in (("face", [1, 1, 1]), ("edge", [2, 1, 1]), ("corner", [2, 2, 1])):
        assert [ref.label(_cubes(name), c)[1] for c in CONNECTIVITIES] == want, name


def test_entry_points_are_declared_and_bound():
    import sys

    import pyfocusr_amd
    from pyfocusr_amd import _hip

    header = open(os.path.join(REPO, "include", "pyfocusr_hip.h")).read()
    for name, res, arity in (("pf_ccl_create", "int", 11), ("pf_ccl_fetch", "int", 9), ("pf_ccl_select", "int", 3),
                             ("pf_ccl_info", "int", 2), ("pf_ccl_combine_stats", "int", 1), ("pf_ccl_free", "void", 1)):
        m = re.search(r"%s\s+%s\s*\(([^)]*)\)\s*;" % (res, name), header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity
        assert len(_hip.SIGNATURES[name][1]) == arity
    assert re.search(r"enum\s*\{\s*PF_CCL_BINARY\s*=\s*0\s*,\s*PF_CCL_BY_VALUE\s*=\s*1\s*,\s*PF_CCL_BACKGROUND\s*=\s*2\s*\}", header)
    assert (_hip.PF_CCL_BINARY, _hip.PF_CCL_BY_VALUE, _hip.PF_CCL_BACKGROUND) == (0, 1, 2)
    for words in ("Its root is its lowest flat index", "numbered 1..C by ascending root", "scipy.ndimage.label"):
        assert words in header
    assert callable(_hip.Context.connected_components) and _hip.DeviceComponents._free == "pf_ccl_free"
    for name in ("connected_components", "keep_largest_components", "largest_component_per_label", "remove_small_components",
                 "fill_holes", "component_boxes", "ComponentStats"):
        assert callable(getattr(pyfocusr_amd, name)), name
    assert "pf_ccl_select" in sys.modules["pyfocusr_amd.components"].__doc__


def test_argument_errors_come_before_the_library(monkeypatch):
    import pyfocusr_amd as pf
    from pyfocusr_amd import _hip

    def no_library(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")

    monkeypatch.setattr(_hip, "default_context", no_library)
    monkeypatch.setattr(_hip, "load_library", no_library)
    good = np.zeros((3, 4, 5), dtype=bool)
    good[1, 2, 3] = True
    every = (pf.connected_components, pf.keep_largest_components, pf.largest_component_per_label, pf.fill_holes,
             lambda v, **k: pf.remove_small_components(v, 2, **k))
    for f in every:
        with pytest.raises(ValueError, match="dimensions"):
            f(good[0])
        with pytest.raises(ValueError, match="at least 1"):
            f(good[:, :0, :])
        with pytest.raises(TypeError, match="boolean or a label map"):
            f(good.astype(np.float64))
        for connectivity in (7, 4, 0, None):
            with pytest.raises(ValueError, match="6, 18 or 26"):
                f(good, connectivity=connectivity)
    with pytest.raises(ValueError, match="fit int32"):
        pf.connected_components(good.astype(np.int64) << 40)
    with pytest.raises(ValueError, match="exclude each other"):
        pf.connected_components(good, by_value=True, background=True)
    for n in (0, -1, 1.5):
        with pytest.raises(ValueError, match="at least 1"):
            pf.keep_largest_components(good, n)
    with pytest.raises(ValueError, match="exactly one"):
        pf.remove_small_components(good)
    with pytest.raises(ValueError, match="exactly one"):
        pf.remove_small_components(good, 2, 3.0)
    with pytest.raises(ValueError, match="not negative"):
        pf.remove_small_components(good, -1)
    with pytest.raises(ValueError, match="positive and finite"):
        pf.remove_small_components(good, min_volume=1.0, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="one number or three"):
        pf.remove_small_components(good, min_volume=1.0, spacing=(1.0, 2.0))


def test_component_stats_arithmetic():
    import pyfocusr_amd as pf

    vol = _three_values()
    _, n, t = ref.components(vol, 6, "by_value")
    stats = pf.ComponentStats(vol.shape, *[t[k] for k in ("count", "value", "root", "lo", "hi", "border", "sum")])
    assert len(stats) == n == 6 and stats.border.dtype == bool
    spacing, origin = np.array([0.5, 1.0, 2.0]), np.array([10.0, -20.0, 30.0])
    assert np.array_equal(stats.volume(spacing), t["count"] * 1.0)
    assert np.array_equal(stats.centroid(spacing, origin), origin + spacing * (t["sum"] / t["count"][:, None]))
    assert np.array_equal(stats.centroid(), t["sum"] / t["count"][:, None])
    boxes = stats.bounding_box
    for c in range(n):
        assert [s.start for s in boxes[c]] == t["lo"][c].tolist() and [s.stop for s in boxes[c]] == (t["hi"][c] + 1).tolist()
    padded = pf.component_boxes(stats, 3)
    assert all(s.start >= 0 and s.stop <= e for box in padded for s, e in zip(box, vol.shape))
    assert padded[0][0] == slice(0, min(t["hi"][0][0] + 4, vol.shape[0]))
    with pytest.raises(ValueError, match="negative"):
        pf.component_boxes(stats, -1)


# ------------------------------------------------------------------------------ contents
def _cubes(touching):
    """Two cubes of 3 x 3 x 3 that share a face, only an edge or only a corner."""
    vol = np.zeros((8, 8, 8), dtype=np.int32)
    vol[1:4, 1:4, 1:4] = 1
    at = {"face": (4, 1, 1), "edge": (4, 4, 1), "corner": (4, 4, 4)}[touching]
    vol[at[0]:at[0] + 3, at[1]:at[1] + 3, at[2]:at[2] + 3] = 1
    return vol


def _serpentine(shape):
    """One voxel-wide path: the z-lines with even i and even j in turn, joined at alternating ends, the slabs of even i
    joined in turn too.  One component for every connectivity; its root (0, 0, 0) is one end of the path."""
    vol = np.zeros(shape, dtype=np.int32)
    end, previous = shape[2] - 1, None
    for a, i in enumerate(range(0, shape[0], 2)):
        js = list(range(0, shape[1], 2))
        for j in (js if a % 2 == 0 else js[::-1]):
            vol[i, j, :] = 1
            if previous is not None:  # the bridge from the previous line, at the end the path left it by
                pi, pj = previous
                vol[(pi + i) // 2, (pj + j) // 2, end] = 1
                end = shape[2] - 1 - end
            previous = (i, j)
    return vol


def _comb(shape):
    """Slabs of z-lines at every other j, joined only by one bar at the highest i: the merges arrive last."""
    vol = np.zeros(shape, dtype=np.int32)
    vol[:, ::2, :] = 1
    vol[-1, :, 0] = 1
    return vol


def _shell(tunnel):
    """A ball with a closed cavity; tunnel: one voxel wide, from the cavity to the border of the volume."""
    shape, centre = (13, 13, 13), (6, 6, 6)
    vol = (ref.ball_mask(shape, centre, 5.0) & ~ref.ball_mask(shape, centre, 2.5)).astype(np.int32)
    if tunnel:
        vol[6, 6, 6:] = 0
    return vol


def _three_values():
    """Values 1, 2, 1 in a row, touching: one component in binary mode, three by value.  The two blobs of value 1 tie in
    count.  Value 3: two components of different sizes, detached.  A speck of value 2."""
    vol = np.zeros((6, 14, 9), dtype=np.int32)
    vol[1:4, 0:4, 2:6] = 1
    vol[1:4, 4:8, 2:6] = 2
    vol[1:4, 8:12, 2:6] = 1
    vol[5, 0:2, 0:2] = 3
    vol[5, 5:10, 7:9] = 3
    vol[5, 13, 4] = 2
    return vol


def _random(shape, density, seed=0):
    rng = np.random.default_rng(list(shape) + [int(density * 100), seed])
    return np.where(rng.random(shape) < density, rng.integers(1, 4, size=shape), 0).astype(np.int32)


def _checker(shape):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2 == 0).astype(np.int32)


_EXTENTS = [(1, 1, 1), (1, 1, 300), (257, 1, 1), (1, 257, 1),  # extents of 1; 257 lines: past a block of k_ccl_hook
            (2, 3, 63), (2, 3, 64), (2, 3, 65), (3, 2, 129),  # runs that end on, cross and start a 64-bit word
            (65, 3, 2), (2, 257, 3), (17, 19, 70),  # lines past a wave and past a block
            (3, 5, 60), (4, 4, 64), (1, 17, 3),  # 15, 16, 17 words: a block of k_ccl_pack takes 16
            (15, 17, 2), (16, 16, 5)]  # 255, 256 words: a block of k_ccl_hook takes 256 (257: above)
_CASES = {"random31-%s" % "x".join(map(str, s)): (lambda s=s: _random(s, 0.31)) for s in _EXTENTS}
_CASES.update({
    "zeros-2x3x65": lambda: np.zeros((2, 3, 65), dtype=np.int32),
    "zeros-17x19x70": lambda: np.zeros((17, 19, 70), dtype=np.int32),
    "ones-2x3x65": lambda: np.ones((2, 3, 65), dtype=np.int32),
    "ones-17x19x70": lambda: np.full((17, 19, 70), 7, dtype=np.int32),
    # runs over whole interior words (all labelled, no start bit): the walks of k_ccl_runs and ccl_scan_up take several steps
    "ones-2x3x200": lambda: np.ones((2, 3, 200), dtype=np.int32),
    "ones-3x5x130": lambda: np.ones((3, 5, 130), dtype=np.int32),
    "random97-3x4x260": lambda: _random((3, 4, 260), 0.97),
    "one-value-97-3x4x260": lambda: (_random((3, 4, 260), 0.97) != 0).astype(np.int32),
    "random05-17x19x70": lambda: _random((17, 19, 70), 0.05),
    "random05-3x2x129": lambda: _random((3, 2, 129), 0.05),
    "random60-17x19x70": lambda: _random((17, 19, 70), 0.6),
    "random60-3x2x129": lambda: _random((3, 2, 129), 0.6),
    "negative-values-2x3x65": lambda: -_random((2, 3, 65), 0.5),
    "checker-6x7x8": lambda: _checker((6, 7, 8)),
    "checker-2x3x65": lambda: _checker((2, 3, 65)),
    "serpentine-9x9x70": lambda: _serpentine((9, 9, 70)),
    "serpentine-17x19x70": lambda: _serpentine((17, 19, 70)),
    "comb-17x19x70": lambda: _comb((17, 19, 70)),
    "comb-65x3x2": lambda: _comb((65, 3, 2)),
    "cubes-face": lambda: _cubes("face"),
    "cubes-edge": lambda: _cubes("edge"),
    "cubes-corner": lambda: _cubes("corner"),
    "shell-closed": lambda: _shell(False),
    "shell-tunnel": lambda: _shell(True),
    "three-values": _three_values,
})


def test_the_contents_are_what_they_claim():
    for shape in ((9, 9, 70), (17, 19, 70)):
        vol = _serpentine(shape)
        comp, n, t = ref.components(vol, 6)
        assert n == 1 and t["root"][0] == 0 and vol[-1, :, :].any()
        ends = np.argwhere((vol == 1) & (_neighbours(vol) == 1))
        assert len(ends) == 2 and tuple(ends[0]) == (0, 0, 0) and ends[1][0] == shape[0] - 1
        assert int((_neighbours(vol)[vol == 1] > 2).sum()) == 0  # a path: nowhere more than two neighbours
    vol = _comb((17, 19, 70))
    assert [ref.label(vol, c)[1] for c in CONNECTIVITIES] == [1, 1, 1]
    assert ref.label(vol[:-1], 26)[1] == 10  # without the bar: the slabs
    assert [ref.label(_three_values(), c)[1] for c in CONNECTIVITIES] == [4, 4, 4]
    assert [ref.label(_three_values(), c, "by_value")[1] for c in CONNECTIVITIES] == [6, 6, 6]
    three = (_three_values()[:5] != 0).astype(np.int32)  # the row 1, 2, 1 alone
    assert ref.label(three, 6)[1] == 1 and ref.label(_three_values()[:5], 6, "by_value")[1] == 3
    closed, tunnel = _shell(False), _shell(True)
    assert ref.label(closed, 26, "background")[1] == 2 and ref.label(tunnel, 6, "background")[1] == 1
    assert ref.fill_holes(closed).sum() > closed.sum() and np.array_equal(ref.fill_holes(tunnel), tunnel != 0)
    assert np.array_equal(_random((2, 3, 65), 0.31), _random((2, 3, 65), 0.31))
    dense = _CASES["one-value-97-3x4x260"]()  # some 64-bit word of it is labelled throughout and starts no run
    assert sum(int(dense[i, j, 64 * w - 1:64 * w + 64].all()) for i in range(3) for j in range(4) for w in (1, 2, 3)) >= 2


def _neighbours(vol):
    """The number of labelled 6-neighbours of every voxel."""
    on = np.pad(vol != 0, 1).astype(np.int32)
    return (on[:-2, 1:-1, 1:-1] + on[2:, 1:-1, 1:-1] + on[1:-1, :-2, 1:-1] + on[1:-1, 2:, 1:-1] + on[1:-1, 1:-1, :-2]
            + on[1:-1, 1:-1, 2:])


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


TABLES = ("count", "value", "root", "lo", "hi", "border", "sum")


def _assert_device_is(raw, vol, connectivity, mode, keep_seed=0):
    """The device's dict against the reference: C, component, every table, the report."""
    comp, n, t = ref.components(vol, connectivity, ref.MODES[mode])
    assert raw["n"] == n
    assert _same(raw["component"], comp)
    for k in TABLES:
        assert _same(raw[k], t[k]), k
    on = int(ref.labelled(vol, ref.MODES[mode]).sum())
    largest = int(t["count"].max()) if n else 0
    assert tuple(raw["report"][:3]) == (vol.size, on, n) and raw["report"][3] >= 0 and raw["report"][4] == largest
    assert np.all(raw["report"][5:] == 0)
    return comp, n, t


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_CASES))
def test_device_equals_the_reference(ctx, name):
    vol = _CASES[name]()
    rng = np.random.default_rng(len(name))
    for connectivity in CONNECTIVITIES:
        for mode in (0, 1, 2):
            keep = {}
            raw = ctx.connected_components(vol, connectivity, mode, keep=lambda t: keep.setdefault("k", rng.random(len(t["count"])) < 0.5))
            comp, n, _ = _assert_device_is(raw, vol, connectivity, mode)
            assert _same(raw["selected"], ref.select(comp, keep["k"])), (connectivity, mode)
            assert raw["device_ms"] > 0.0
    if name.startswith("serpentine") or name.startswith("comb"):
        print("%s: %d retries of the unions at 26" % (name, raw["report"][3]))


@pytest.mark.gpu
def test_the_counts_of_the_named_contents(ctx):
    board = _checker((6, 7, 8))
    assert [ctx.connected_components(board, c, stats=False)["n"] for c in CONNECTIVITIES] == [168, 1, 1]
    for name, want in (("face", [1, 1, 1]), ("edge", [2, 1, 1]), ("corner", [2, 2, 1])):
        assert [ctx.connected_components(_cubes(name), c, stats=False)["n"] for c in CONNECTIVITIES] == want, name
    three = _three_values()[:5]
    assert ctx.connected_components(three, 6, 0, stats=False)["n"] == 1 and ctx.connected_components(three, 6, 1, stats=False)["n"] == 3
    raw = ctx.connected_components(_serpentine((17, 19, 70)), 6)
    assert raw["n"] == 1 and raw["root"][0] == 0 and raw["count"][0] == raw["report"][1]


def _stable(raw):
    """A call's outputs without its timing and without the one count that depends on scheduling (the unions' retries)."""
    out = {k: v for k, v in raw.items() if k != "device_ms"}
    out["report"] = out["report"].copy()
    out["report"][3] = 0
    return out


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(ctx):
    from test_pool_hygiene import _flat

    for vol in (_random((17, 19, 70), 0.31), _serpentine((17, 19, 70))):
        for connectivity, mode in ((6, 0), (26, 1), (18, 2)):
            keep = np.arange(ref.label(vol, connectivity, ref.MODES[mode])[1]) % 3 == 0
            a, b = (_flat(_stable(ctx.connected_components(vol, connectivity, mode, keep=keep))) for _ in range(2))
            assert len(a) == 11 and a == b


@pytest.mark.gpu
def test_pool_contents_change_nothing(hip, ctx):
    """The four runs of tests/test_pool_hygiene.py for this unit: plain, every pool block filled with 0xFF, with 0x00, and
    after a neighbour twice as large per axis on the same ctx."""
    from test_pool_hygiene import _flat

    vol, big = _random((5, 6, 70), 0.31), _random((10, 12, 140), 0.31)
    keeps = {(c, m): np.arange(ref.label(vol, c, ref.MODES[m])[1]) % 2 == 0 for c in CONNECTIVITIES for m in (0, 1, 2)}

    def run(neighbour):
        if neighbour:
            ctx.connected_components(big, 26, 1)
        return {"%d/%d" % key: _stable(ctx.connected_components(vol, key[0], key[1], keep=keep)) for key, keep in keeps.items()}

    lib, runs = hip.load_library(), {}
    try:
        for mode, label in ((0, "plain"), (1, "0xFF"), (2, "0x00")):
            assert lib.pf_pool_poison(mode) == 0
            out = run(False)
            if mode == 0:
                for (c, m) in keeps:
                    _assert_device_is(out["%d/%d" % (c, m)], vol, c, m)
            runs[label] = _flat(out)
    finally:
        lib.pf_pool_poison(0)
    runs["after a larger neighbour"] = _flat(run(True))
    plain = runs.pop("plain")
    assert len(plain) == 9 * 11
    for label, got in runs.items():
        differ = [w for (w, a), (_, b) in zip(plain, got) if a != b]
        assert len(got) == len(plain) and not differ, "%s: %s differ from the plain run" % (label, ", ".join(differ))


@pytest.mark.gpu
def test_separate_statistics_atomics_give_the_same_tables(hip, ctx):
    lib, vol = hip.load_library(), _random((17, 19, 70), 0.6)
    try:
        assert lib.pf_ccl_combine_stats(0) == 0
        for connectivity in CONNECTIVITIES:
            _assert_device_is(ctx.connected_components(vol, connectivity, 0), vol, connectivity, 0)
        _assert_device_is(ctx.connected_components(np.ones((3, 5, 130), dtype=np.int32), 6, 0), np.ones((3, 5, 130), dtype=np.int32), 6, 0)
    finally:
        lib.pf_ccl_combine_stats(1)


@pytest.mark.gpu
def test_the_library_refuses_bad_input(hip, ctx):
    import ctypes as C

    lib, h = hip.load_library(), C.c_void_p()
    vol = np.ones(8, dtype=np.int32)

    def create(nx, ny, nz, connectivity=6, mode=0, flags=0, v=vol, handle=True, context=True):
        return lib.pf_ccl_create(ctx._h if context else None, hip._ptr(v), nx, ny, nz, connectivity, mode, flags,
                                 C.byref(h) if handle else None, None, None)

    assert create(2, 2, 0) == -1 and b"extents" in lib.pf_last_error()
    assert create(0, 2, 2) == -1 and b"extents" in lib.pf_last_error()
    assert create(2 ** 16, 2 ** 15, 1) == -1 and b"samples" in lib.pf_last_error()  # 2^31 samples: refused before any is read
    assert create(2 ** 31, 1, 1) == -1
    for connectivity in (7, 0, 4, 8, 27, -6):
        assert create(2, 2, 2, connectivity=connectivity) == -1 and b"connectivity" in lib.pf_last_error()
    assert create(2, 2, 2, mode=3) == -1 and b"mode" in lib.pf_last_error()
    assert create(2, 2, 2, mode=-1) == -1
    assert create(2, 2, 2, flags=1) == -1 and b"flags" in lib.pf_last_error()
    assert create(2, 2, 2, v=None) == -1 and b"NULL" in lib.pf_last_error()
    assert create(2, 2, 2, handle=False) == -1 and create(2, 2, 2, context=False) == -1
    assert not h.value
    assert lib.pf_ccl_fetch(None, None, None, None, None, None, None, None, None) == -1 and b"NULL" in lib.pf_last_error()
    assert lib.pf_ccl_info(None, None) == -1
    assert create(2, 2, 2) == 0 and h.value  # without report and device_ms
    n, out = C.c_int64(-1), np.zeros(8, dtype=np.uint8)
    assert lib.pf_ccl_info(h, C.byref(n)) == 0 and n.value == 1
    assert lib.pf_ccl_info(h, None) == -1
    assert lib.pf_ccl_fetch(h, None, None, None, None, None, None, None, None) == 0  # nothing asked for
    assert lib.pf_ccl_select(h, None, hip._ptr(out)) == -1 and lib.pf_ccl_select(h, hip._ptr(out), None) == -1
    assert lib.pf_ccl_select(h, hip._ptr(np.ones(1, dtype=np.uint8)), hip._ptr(out)) == 0 and out.all()
    lib.pf_ccl_free(h)
    lib.pf_ccl_free(None)
    # after the refusals the context still works
    raw = ctx.connected_components(_cubes("corner"), 18, 0)
    _assert_device_is(raw, _cubes("corner"), 18, 0)
    with hip.DeviceComponents(np.zeros((2, 2, 2), dtype=bool), ctx=ctx) as empty:  # no component: nothing to keep
        assert empty.n == 0 and not empty.select(np.zeros(0, dtype=bool)).any()
        with pytest.raises(ValueError, match="one entry per component"):
            empty.select(np.ones(1, dtype=bool))


@pytest.fixture(scope="module")
def organ():
    """A 96 x 100 x 130 mask: three overlapping ellipsoids, a detached one, specks outside and cavities inside."""
    shape, rng = (96, 100, 130), np.random.default_rng(3)
    mask = np.zeros(shape, dtype=bool)
    for centre, radius in (((40, 50, 60), 28.0), ((60, 45, 80), 20.0), ((30, 60, 40), 15.0), ((80, 85, 110), 9.0)):
        mask |= ref.ball_mask(shape, centre, radius, (1.0, 0.9, 0.8))
    return mask ^ (rng.random(shape) < 2e-3)


@pytest.mark.gpu
def test_a_volume_of_a_million_samples_against_scipy(ctx, organ):
    ndimage = pytest.importorskip("scipy.ndimage")
    for connectivity in CONNECTIVITIES:
        raw = ctx.connected_components(organ, connectivity)
        want, n = ndimage.label(organ, _structure(ndimage, connectivity))
        assert raw["n"] == n and n > 500 and _same(raw["component"], want.astype(np.int32))
        count = np.bincount(want.reshape(-1), minlength=n + 1)[1:]
        assert np.array_equal(raw["count"], count) and raw["report"][4] == count.max() > 10 ** 5
        print("connectivity %d: %d components, %d retries, %.3f ms on the device" % (connectivity, n, raw["report"][3], raw["device_ms"]))
    import pyfocusr_amd as pf

    assert _same(pf.fill_holes(organ, ctx=ctx), ndimage.binary_fill_holes(organ))
    faces = ndimage.label(organ)[0]  # 6-connectivity, the default of both
    assert _same(pf.keep_largest_components(organ, ctx=ctx), faces == int(np.argmax(np.bincount(faces.reshape(-1))[1:])) + 1)


@pytest.mark.gpu
def test_specks_and_cavities_go_and_nothing_else_changes(ctx):
    """A ball with 3 specks well away from it and 4 closed cavities: 8 surface patches before, 1 after, and the changed
    voxels are exactly the specks and the cavities."""
    import pyfocusr_amd as pf

    shape = (30, 30, 30)
    ball = ref.ball_mask(shape, (13, 13, 13), 9.0)
    assert pf.mesh_topology(pf.mask_to_mesh(ball, ctx=ctx), ctx=ctx).n_patches == 1  # the precondition: a manifold surface
    specks = [(26, 26, 26), (2, 25, 3), (25, 3, 20)]
    cavities = [(13, 13, 13), (9, 13, 13), (16, 10, 14), (13, 17, 9)]
    mask = ball.copy()
    for at in specks:
        assert not ball[at]
        mask[at] = True
    for at in cavities:
        assert ball[at]
        mask[at] = False
    assert pf.mesh_topology(pf.mask_to_mesh(mask, ctx=ctx), ctx=ctx).n_patches == 8
    cleaned = pf.fill_holes(pf.keep_largest_components(mask, ctx=ctx), ctx=ctx)
    assert cleaned.dtype == bool and pf.mesh_topology(pf.mask_to_mesh(cleaned, ctx=ctx), ctx=ctx).n_patches == 1
    assert sorted(map(tuple, np.argwhere(cleaned != mask))) == sorted(specks + cavities)
    assert np.array_equal(cleaned, ball)


@pytest.mark.gpu
def test_selectors_follow_the_reference(ctx):
    import pyfocusr_amd as pf

    vol = _three_values().astype(np.int16)
    for connectivity in CONNECTIVITIES:
        kept = pf.largest_component_per_label(vol, connectivity, ctx=ctx)
        assert _same(kept, ref.largest_per_label(vol, connectivity))
        # the two blobs of value 1 tie: the lower number, which comes first in C order, stays
        assert (kept[1:4, 0:4, 2:6] == 1).all() and not kept[1:4, 8:12, 2:6].any()
        assert (kept[5, 5:10, 7:9] == 3).all() and not kept[5, 0:2, 0:2].any() and not kept[5, 13, 4]
        for least in (0, 1, 2, 4, 5, 10, 11, 144, 145):
            assert _same(pf.remove_small_components(vol, least, connectivity=connectivity, ctx=ctx), ref.remove_small(vol, least, connectivity))
        for n in (1, 2, 3, 4, 9):
            assert _same(pf.keep_largest_components(vol, n, connectivity, ctx=ctx), ref.keep_largest(vol, n, connectivity))
        # a volume threshold in cubic millimetres: 10 voxels of 0.5 x 1 x 2 mm are 10 mm^3
        assert _same(pf.remove_small_components(vol, min_volume=10.0, spacing=(0.5, 1.0, 2.0), connectivity=connectivity, ctx=ctx),
                     ref.remove_small(vol, 10, connectivity))
    for tunnel in (False, True):
        for connectivity in CONNECTIVITIES:
            assert _same(pf.fill_holes(_shell(tunnel), connectivity, ctx=ctx), ref.fill_holes(_shell(tunnel), connectivity))
    assert pf.fill_holes(_shell(False), ctx=ctx).sum() > _shell(False).sum()
    assert np.array_equal(pf.fill_holes(_shell(True), ctx=ctx), _shell(True) != 0)
    labels, n, stats = pf.connected_components(vol, 6, by_value=True, return_stats=True, ctx=ctx)
    comp, m, t = ref.components(vol, 6, "by_value")
    assert n == m == 6 and _same(labels, comp) and all(np.array_equal(getattr(stats, k), t[k]) for k in TABLES)
    labels, n = pf.connected_components(vol, 26, background=True, ctx=ctx)
    assert _same(labels, ref.label(vol, 26, "background")[0]) and n == 1
