"""The test matrices of tests/_window_ref.py sit exactly on, and one past, the capacity limits of the resident filter's
window structures - checked here with numpy alone, so that tests/test_resident_windows.py (GPU) can rely on it."""
import numpy as np
import pytest
from scipy import sparse

import _window_ref as wr


def degrees(M):
    return np.diff(wr.offdiag(M)[0])


def test_window_rows_and_padding():
    assert [wr.n_pad_of(n) for n in (1, 2, 4096, 4097, 5000, 266240, 528384)] == [4096, 4096, 4096, 8192, 8192, 266240, 528384]
    assert [wr.window_rows(p) for p in (4096, 262144, 262145, 266240, 524288, 528384)] == [1024, 1024, 2048, 2048, 2048, 4096]


def test_base_matrix():
    M, _, r = wr.case("n4096")
    W = M - sparse.diags(M.diagonal())
    assert (abs(W - W.T)).nnz == 0 and W.data.min() >= -1.0 and W.data.max() <= -0.1
    i, j = W.nonzero()
    assert set(np.abs(i - j)) == {1, 2, 3}
    empty = wr.empty_rows(4096)
    assert np.all(np.diff(M.indptr)[empty] == 0) and np.all(np.diff(M.indptr)[~empty] > 1)
    d = M.diagonal()[~empty]
    assert d.min() >= 1.0 and d.max() <= 3.0
    assert (r.win_rows, r.n_windows) == (1024, 4)


@pytest.mark.parametrize("target", [1024, 1025, 512, 513])
def test_ghost_list_family(target):
    _, _, r = wr.case("ghosts%d" % target)
    assert r.ghosts.max() == target == r.ghosts[2] and r.pattern_symmetric
    assert r.candidates.max() <= wr.CAND_MAX and r.max_degree <= 8       # only the ghost list can refuse it; nothing spills
    assert r.covered == (target <= 1024) and r.resident == r.covered
    assert len(r.reads[2]) == target and np.sum(r.reads[2] // 1024 == 5) == target - 6   # distinct rows of window 5
    assert np.all(np.diff(r.reads[2][r.reads[2] // 1024 == 5]) == 1)                     # a contiguous run
    if target in (512, 513):
        checks = dict(r.ring_checks)
        assert checks.pop("ring1_rows") == (target == 512) and all(checks.values())       # half a block is the only refusal
        assert r.covered2 == r.two_step == (target == 512)


@pytest.mark.parametrize("target", [4096, 4097])
def test_candidate_cap_family(target):
    _, _, r = wr.case("cand%d" % target)
    base = wr.case("n4096")[2]
    assert r.candidates[3] == target == r.candidates.max() and len(r.oneway[3]) == 0
    assert r.ghosts.max() <= 16 and not r.pattern_symmetric               # far from the ghost list: only the cap can refuse it
    assert r.covered == (target == 4096)
    assert np.sum(r.reads[3] // 1024 == 6) == 5                           # the same few rows of window 6
    assert list(r.oneway[6]) == [3] and [len(o) for o in r.oneway].count(0) == 7
    assert len(r.reads[6]) == base.ghosts[2] == 6 and r.ghosts[6] == 7    # the band count and row 0 of window 3
    assert r.candidates[6] == r.entries[6] + 1
    assert np.all(r.need_exact >= r.need_lo) and np.all(r.need_exact <= r.need_hi)
    assert r.need_exact[3] > r.need_lo[3]                                  # one-way: boundary rows nobody reads lead too


@pytest.mark.parametrize("degree", [16, 17])
def test_ring_row_width_family(degree):
    M, _, r = wr.case("ringrow%d" % degree)
    assert r.max_degree == degree == degrees(M)[4096] and r.pattern_symmetric
    assert r.iperm[4096] in r.ring1[3] and r.ring1_width[3] == degree      # row 4096 is a ring-1 row of window 3
    assert r.covered and r.resident
    checks = dict(r.ring_checks)
    assert checks.pop("ring1_width") == (degree == 16) and all(checks.values())
    assert r.covered2 == r.two_step == (degree == 16)


def test_spilling_family():
    M, _, r = wr.case("spill")
    d = degrees(M)
    assert {9, 16, 40} <= set(d[1024:2048]) and d.max() == 40 and r.pattern_symmetric
    assert r.covered and r.resident                                         # rows wider than 8 spill to LDS, and it fits
    # the 40-entry row leads window 1's interior, right behind the few boundary rows: their slice is 40 wide, and those
    # boundary rows are ring-1 rows of windows 0 and 2 - the second ring is refused for its row width alone
    checks = dict(r.ring_checks)
    assert list(r.ring1_width[:3]) == [40, 6, 40] and not checks.pop("ring1_width") and all(checks.values())
    M, _, r = wr.case("spill300")
    d = degrees(M)
    r0 = int(np.argmax(d))
    assert d[r0] == 300 and {9, 16, 40} <= set(d[1024:2048]) and r.pattern_symmetric
    cols = M.indices[M.indptr[r0]:M.indptr[r0 + 1]]
    assert set(cols // 1024) == {3, 4, 5}
    assert r.covered and not r.resident and r.lds > wr.LDS_LIMIT            # the structures hold it, the LDS budget does not


def test_shape_family():
    r = wr.case("n2")[2]
    assert (r.n_windows, r.sell_entries) == (4, 64) and r.covered and not r.ghosts.any() and np.all(r.need_exact == 1)
    r = wr.case("n4096")[2]
    assert r.n_windows == 4 and list(r.ghosts) == [3, 6, 6, 3]
    for name, rows_last in (("n4097", 1), ("n5000", 5000 - 4096)):
        r = wr.case(name)[2]
        assert r.n_windows == 8 and r.covered
        assert not r.ghosts[5:].any() and not r.candidates[5:].any() and np.all(r.need_exact[5:] == 1)   # padding only
        assert r.ghosts[4] == 3 and r.read_by_others[4] == min(rows_last, 3)  # window 4 reads rows 4093..4095 whatever it holds
    r = wr.case("block_diagonal")[2]
    assert r.covered and r.covered2 and not r.ghosts.any() and not r.ghosts2.any() and np.all(r.need_exact == 1)
    r = wr.case("diagonal")[2]
    assert r.sell_entries == 0 and not r.covered and not r.resident


@pytest.mark.parametrize("name,win_rows", [("rows2048", 2048), ("rows2048b", 2048), ("rows4096", 4096)])
def test_large_windows(name, win_rows):
    M, planted, r = wr.case(name)
    d = degrees(M)
    assert r.win_rows == win_rows and r.n_windows <= 256 and r.pattern_symmetric
    assert {5, 6, 7, 8} <= set(d) and d.max() == 8 and len(planted) >= 400
    assert r.covered and r.resident and not r.covered2                      # (two steps: 1024-row windows only)
    assert r.ghosts.max() > 6                                               # the long-range edges are seen
    if win_rows == 2048:
        assert wr.pair_resident(r, r)                                       # jr = 4: two entries of every row spill
    else:
        assert wr.lds_need([r, r]) == -1 and r.lds > 2 * 4096 * 16          # one graph only, and its rows spill (jr = 4)


@pytest.mark.parametrize("name", list(wr.CASES) + list(wr.LARGE))
def test_need_and_order(name):
    """need as the issue states it - for a symmetric pattern max(1, rows read by others), for a general one between that
    and the number of boundary rows - agrees with the restated order; and that order keeps windows and puts the boundary
    rows first."""
    M, _, r = wr.case(name)
    assert np.array_equal(np.sort(r.perm), np.arange(r.n)) and np.array_equal(r.perm // r.win_rows, np.arange(r.n) // r.win_rows)
    if r.pattern_symmetric:
        assert np.array_equal(r.need_exact, r.need_lo) and np.array_equal(r.need_lo, r.need_hi)
    else:
        assert np.all(r.need_lo <= r.need_exact) and np.all(r.need_exact <= r.need_hi)
    assert np.all(r.ghosts[r.n_windows - (r.n_pad - r.n) // r.win_rows:] == 0)


def test_need_depends_on_the_boundary_first_order():
    """need taken in the CALLER's order (no sort inside windows) is far from the number of rows read: a restatement that
    forgets the order cannot pass."""
    _, _, r = wr.case("ghosts512")
    indptr, rows, cols = wr.offdiag(wr.case("ghosts512")[0])
    out = rows // 1024 != cols // 1024
    naive = np.zeros(8, np.int64)
    np.maximum.at(naive, cols[out] // 1024, cols[out] % 1024 + 1)
    assert naive[2] > r.need_exact[2] and naive[1] == 1024 and r.need_exact[1] == 6
