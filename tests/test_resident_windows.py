"""The resident filter kernel (csrc/pf_persist.hip) at the capacity limits of its window structures (csrc/pf_windows.hip,
row order of csrc/pf_reorder.hip).

Every matrix of tests/_window_ref.py sits exactly on or one past a limit (tests/test_window_ref.py shows that without a
GPU).  Here, per matrix: `window_info` equals the numpy restatement (coverage of both rings, outside rows and published
rows per window); the launch counters of `persist_state` move exactly as the restatement predicts (so a limit case ran
the path it was built for - or provably did not); every resident result has the bits of one step per launch; the source
slot is untouched and the destination's padding rows are zero; and the streamed result agrees with the float64 numpy
recurrence, which ties the bit comparison to a reference.

The vectors carry O(1) values in the first and last row of every window and in every planted row over a ~1e-3
background: a misrouted outside value costs far more than rounding.
"""
import contextlib
import os

import numpy as np
import pytest

import _exact as ex
import _window_ref as wr

pytestmark = pytest.mark.gpu

DEGREES = (7, 8, 9, 10, 11, 41, 145)  # every phase of the 4-slot ring, its wrap, the phase carried across launches
SINGLE = list(wr.CASES) + ["rows2048", "rows4096"]


@pytest.fixture(scope="module")
def hip():
    from pyfocusr_amd import _hip

    _hip.load_library()
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@contextlib.contextmanager
def switches(hip, enabled=True, two_step=1, halves=True, hold=None):
    """The process-wide switches of the resident path, restored to their defaults afterwards."""
    saved = os.environ.get("PF_PERSIST_HOLD")
    try:
        hip.persist_enable(enabled)  # (True also lifts a suspension an earlier test may have left)
        hip.persist_two_step(two_step)
        hip.persist_pair_halves(halves)
        if hold is None:
            os.environ.pop("PF_PERSIST_HOLD", None)
        else:
            os.environ["PF_PERSIST_HOLD"] = str(hold)
        yield
    finally:
        hip.persist_enable(True)
        hip.persist_two_step(1)
        hip.persist_pair_halves(True)
        if saved is None:
            os.environ.pop("PF_PERSIST_HOLD", None)
        else:
            os.environ["PF_PERSIST_HOLD"] = saved


class Case(object):
    """One matrix on the device with its restatement, its planted vector, and what is computed once and shared: the
    streamed results (one step per launch) and the numpy recurrence, per (degree, rho)."""

    def __init__(self, hip, ctx, name):
        self.hip, self.ctx, self.name = hip, ctx, name
        self.M, planted, self.ref = wr.case(name)
        M, n, w = self.M, self.M.shape[0], self.ref.win_rows
        self.g = hip.DeviceLaplacian(matrix=(M.indptr, M.indices, M.data), ctx=ctx)
        self.g.ws_ensure(4)
        rng = np.random.default_rng(len(name) + n)
        idx = np.unique(np.concatenate([np.arange(0, n, w), np.minimum(np.arange(w - 1, n + w - 1, w), n - 1), planted]))
        self.x = 1e-3 * rng.standard_normal(n)
        self.x[idx] = rng.uniform(1.0, 2.0, len(idx)) * np.where(rng.random(len(idx)) < 0.5, -1.0, 1.0)
        self.R = float(np.max(abs(M) @ np.ones(n)))  # the Gershgorin radius; c = e = R as in test_vector_kernels
        self.apps, self.rings = 0, False  # the graph's single applications so far; second-ring structures asked for
        self._streamed, self._numpy = {}, {}

    def numpy_recurrence(self, rho):
        if rho not in self._numpy:
            c = e = self.R
            ys = [self.x, (c * self.x - self.M @ self.x) / (e * rho)]
            for _ in range(40):
                ys.append((2.0 / (e * rho)) * (c * ys[-1] - self.M @ ys[-1]) - ys[-2] / rho**2)
            self._numpy[rho] = ys
        return self._numpy[rho]

    def streamed(self, degree, rho):
        """One step per launch (persist off), checked against the numpy recurrence up to degree 41."""
        key = (degree, rho)
        if key not in self._streamed:
            before = self.hip.persist_state(self.ctx)["launches"]
            with switches(self.hip, enabled=False):
                self.g.upload(0, self.x)
                self.g.cheb(0, 1, degree, self.R, self.R, rho)
                y = self.g.download_slots(1, 1)[:, 0].copy()
            assert self.hip.persist_state(self.ctx)["launches"] == before
            if degree <= 41:
                want = self.numpy_recurrence(rho)[degree]
                err, scale = float(np.max(np.abs(y - want))), float(np.max(np.abs(want)))
                print("%s degree %d rho %g: streamed against numpy %.3g, bound %.3g" % (self.name, degree, rho, err, 1e-12 * scale))
                assert err <= 1e-12 * scale, (self.name, degree, rho, err, scale)
            self._streamed[key] = y
        return self._streamed[key]

    def predict_single(self, degree, two_step):
        """(resident launches, of them two steps per exchange) of the next pf_cheb, as pf_persist_cheb decides it: nothing
        below degree 8; a graph with 1024-row windows gets its second-ring structures at its third single application and
        uses them from then on where they cover it; otherwise one step per exchange where the first ring covers it."""
        ref = self.ref
        if degree < 8:
            return 0, 0
        if two_step and ref.win_rows == 1024:
            if not self.rings:
                self.apps += 1
                self.rings = self.apps >= 3
            if self.rings and ref.two_step:
                return 1, 1
        return (1, 0) if ref.resident else (0, 0)

    def assert_padding_zero(self, slot, y):
        g = self.g
        depth = ex.reduction_depth(g.n)
        err = abs(float(g.dots(slot, slot, 1)[0]) - ex.exact_sumsq(y))
        assert err <= ex.dot_bound(y, y, depth), ("padding rows of the destination are not zero", self.name, err)


@pytest.fixture(scope="module")
def cases(hip, ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(hip, ctx, name)
        return cache[name]

    yield get
    for c in cache.values():
        c.g.close()


@contextlib.contextmanager
def no_timeout(hip, ctx, what):
    """A wait that ran out inside a resident launch is its own failure, not 'wrong bits'; nothing is run again."""
    before = hip.persist_state(ctx)["timeouts"]
    try:
        yield
    except hip.PfError as e:
        if e.code == hip.PF_E_PERSIST_TIMEOUT:
            pytest.fail("a wait inside the resident kernel ran out (PF_E_PERSIST_TIMEOUT), results were not compared: %r" % (what,))
        raise
    after = hip.persist_state(ctx)["timeouts"]
    if after != before:
        pytest.fail("persist_state timeouts rose from %d to %d: a wait inside the resident kernel ran out: %r" % (before, after, what))


def check_window_info(info, ref, name, rings):
    assert (info["win_rows"], info["n_windows"]) == (ref.win_rows, ref.n_windows), name
    assert info["state"] == int(ref.covered), (name, "first ring", info["state"], ref.ghosts.max(), ref.candidates.max())
    if ref.covered:
        assert np.array_equal(info["ghosts"], ref.ghosts), (name, info["ghosts"], ref.ghosts)
        need = info["need"]
        if ref.pattern_symmetric:
            assert np.array_equal(need, ref.need_lo), (name, need, ref.need_lo)  # = max(1, rows read by others): boundary rows lead
        else:
            assert np.all(ref.need_lo <= need) and np.all(need <= ref.need_hi), (name, need, ref.need_lo, ref.need_hi)
        assert np.array_equal(need, ref.need_exact), (name, need, ref.need_exact)  # the restated order, row for row
    else:
        assert info["ghosts"] is None and info["need"] is None, name
    if rings:
        assert info["state2"] == int(ref.covered2), (name, "second ring", info["state2"], getattr(ref, "ring_checks", None))
        if ref.covered2:
            assert np.array_equal(info["ghosts2"], ref.ghosts2), (name, info["ghosts2"], ref.ghosts2)
        else:
            assert info["ghosts2"] is None, name


def run_sequence(c, hip, ctx, rho, two_step, hold):
    g = c.g
    want = {d: c.streamed(d, rho) for d in DEGREES}
    with switches(hip, two_step=two_step, hold=hold):
        g.upload(0, c.x)
        for d in DEGREES:
            what = (c.name, "degree", d, "rho", rho, "two_step", two_step, "hold", hold)
            g.upload(1, np.full(g.n, 9.0))
            expect = c.predict_single(d, two_step)
            s0 = hip.persist_state(ctx)
            with no_timeout(hip, ctx, what):
                g.cheb(0, 1, d, c.R, c.R, rho)
                y = g.download_slots(1, 1)[:, 0]
            s1 = hip.persist_state(ctx)
            got = (s1["launches"] - s0["launches"], s1["launches_two_step"] - s0["launches_two_step"])
            assert got == expect, ("resident launches (all, two-step): got, predicted", got, expect, what)
            assert np.array_equal(y, want[d]), ("resident bits differ from one step per launch", what,
                                                int(np.sum(y != want[d])), np.flatnonzero(y != want[d])[:8])
            if g.n <= 10000 or d == DEGREES[-1]:
                c.assert_padding_zero(1, y)
        assert np.array_equal(g.download_slots(0, 1)[:, 0], c.x), ("source slot changed", c.name)


@pytest.mark.parametrize("name", SINGLE)
def test_single_graph_at_the_limits(hip, ctx, cases, name):
    """One graph per limit case, shape and window size.  Fresh graph: window_info (first ring) against the restatement;
    degrees 7..145 with two steps per exchange allowed - the launch counters show one-step launches for the first two
    applications and two-step launches from the third on exactly where the second ring is predicted (512 outside rows,
    a ring-1 row of 16 entries), none for 513 outside rows, a ring-1 row of 17 entries or windows of 2048 / 4096 rows,
    and no resident launch at all past the ghost list (1025), the candidate cap (4097), without stored entries, or where
    the spilled entries of a 300-entry row exceed the LDS budget; then window_info with the second ring; then rho 1.02,
    two_step 0 and PF_PERSIST_HOLD=0, all with the bits of one step per launch."""
    c = cases(name)
    fresh = c.g.window_info()
    assert fresh["state2"] == -1, name  # nobody has asked for the second ring yet
    check_window_info(fresh, c.ref, name, rings=False)
    run_sequence(c, hip, ctx, 1.0, 1, None)
    assert c.rings == (c.ref.win_rows == 1024)  # (the third application has asked for the second ring, where there can be one)
    check_window_info(c.g.window_info(rings=True), c.ref, name, rings=True)
    c.rings = True
    run_sequence(c, hip, ctx, 1.02, 1, None)
    run_sequence(c, hip, ctx, 1.0, 0, None)
    run_sequence(c, hip, ctx, 1.02, 1, "0")
    run_sequence(c, hip, ctx, 1.0, 0, "0")


PAIRS = [
    ("ghosts512", "ringrow16", ((41, 41), (10, 41), (145, 9), (7, 5))),   # both lists fit half a block: opposite halves
    ("ghosts513", "cand4096", ((41, 41), (9, 10))),                       # 513: the same-order pair kernel; a one-way graph
    ("spill", "n4096", ((41, 41), (8, 11))),                              # 8 windows beside 4; spilled entries
    ("n2", "block_diagonal", ((41, 41), (11, 8))),
    ("ghosts1024", "ghosts1025", ((41, 41), (10, 41))),                   # covered with not covered: the whole pair streams
    ("cand4097", "ghosts512", ((41, 41), (145, 9))),                      # the same, the other way round
    ("rows2048", "rows2048b", ((41, 41), (10, 41))),                      # 2048-row windows, 4 entries per row in registers
]


@pytest.mark.parametrize("name_a,name_b,degrees", PAIRS, ids=["%s+%s" % p[:2] for p in PAIRS])
def test_pairs_at_the_limits(hip, ctx, cases, name_a, name_b, degrees):
    """pf_cheb2 on two different cases, equal and unequal degrees, rho 1.0 beside 1.02: ONE resident launch where both
    graphs are covered and fit together, none where one of them is not covered (the whole pair streams) or below degree
    8; never a two-step launch; the bits of the same call with persist off, with the opposite-halves kernel on and off
    and PF_PERSIST_HOLD unset and 0; each graph's streamed result against its own numpy recurrence (the single-graph
    streamed bits, which Case.streamed has checked)."""
    a, b = cases(name_a), cases(name_b)
    resident = wr.pair_resident(a.ref, b.ref)
    assert resident == (a.ref.covered and b.ref.covered), (name_a, name_b)  # (none of these pairs is refused for its LDS need)
    for da, db in degrees:
        ra, rb = (a.g, (0, 2, da, a.R, a.R, 1.0)), (b.g, (0, 2, db, b.R, b.R, 1.02))
        a.g.upload(0, a.x)
        b.g.upload(0, b.x)
        s0 = hip.persist_state(ctx)
        with switches(hip, enabled=False):
            a.g.cheb2(ra[1], b.g, rb[1])
            want = (a.g.download_slots(2, 1)[:, 0].copy(), b.g.download_slots(2, 1)[:, 0].copy())
        assert hip.persist_state(ctx)["launches"] == s0["launches"]
        assert np.array_equal(want[0], a.streamed(da, 1.0)) and np.array_equal(want[1], b.streamed(db, 1.02)), (name_a, name_b, da, db)
        for halves in (True, False):
            for hold in (None, "0"):
                what = (name_a, name_b, da, db, "halves", halves, "hold", hold)
                with switches(hip, halves=halves, hold=hold):
                    a.g.upload(2, np.full(a.g.n, 9.0))
                    b.g.upload(2, np.full(b.g.n, 9.0))
                    s0 = hip.persist_state(ctx)
                    with no_timeout(hip, ctx, what):
                        a.g.cheb2(ra[1], b.g, rb[1])
                        ya, yb = a.g.download_slots(2, 1)[:, 0], b.g.download_slots(2, 1)[:, 0]
                    s1 = hip.persist_state(ctx)
                got = (s1["launches"] - s0["launches"], s1["launches_two_step"] - s0["launches_two_step"])
                expect = (1 if resident and max(da, db) >= 8 else 0, 0)
                assert got == expect, ("resident launches (all, two-step): got, predicted", got, expect, what)
                assert np.array_equal(ya, want[0]), ("resident bits differ from one step per launch (first graph)", what)
                assert np.array_equal(yb, want[1]), ("resident bits differ from one step per launch (second graph)", what)
        a.assert_padding_zero(2, ya)
        b.assert_padding_zero(2, yb)
        assert np.array_equal(a.g.download_slots(0, 1)[:, 0], a.x) and np.array_equal(b.g.download_slots(0, 1)[:, 0], b.x), "source slot changed"
