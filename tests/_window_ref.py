"""A numpy restatement of the window structures of the resident filter kernel (csrc/pf_windows.hip, the in-window row
order of csrc/pf_reorder.hip and the LDS budgets of csrc/pf_persist.hip), and the test matrices that sit on and one past
every capacity limit of those structures.  No GPU, no library: tests/test_window_ref.py checks the matrices against
their targets on any machine, tests/test_resident_windows.py compares the device with `analyse`.

The input is a scipy CSR operator as handed to `pf_graph_from_matrix`; only its off-diagonal pattern matters.  Such a graph
keeps the caller's row order up to a sort inside windows of win_rows rows, so caller row i lies in window i // win_rows
and all counts below are stated in caller rows.  Where the ORDER inside a window matters (which row is a window's row 0,
how wide a SELL-64 slice is, how many leading rows a window publishes) `solver_order` restates the sort: boundary rows
first, then the rows one hop behind them, then descending degree, ties by position.
"""
import numpy as np
from scipy import sparse

GHOSTS_MAX = 1024   # PF_WIN_GHOSTS: outside rows per window
CAND_MAX = 4096     # WB_CAP: outside entries per window before deduplication
G1_MAX = 512        # PF_WIN_G1: ring-1 rows per window (and half a block: the pair kernel with opposite halves)
GW_MAX = 16         # PF_WIN_GW: entries per ring-1 row
WINDOWS_MAX = 256
LDS_LIMIT = 160 * 1024 - 512
SLICE = 64


def n_pad_of(n):
    return (n + 4095) // 4096 * 4096


def window_rows(n_pad):
    return 1024 if n_pad <= 262144 else (2048 if n_pad <= 524288 else 4096)


def offdiag(M):
    """(indptr, rows, cols) of the stored off-diagonal entries of a CSR matrix."""
    M = sparse.csr_matrix(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    keep = rows != M.indices
    rows, cols = rows[keep].astype(np.int64), M.indices[keep].astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M.shape[0]))])
    return indptr, rows, cols


def solver_order(n, indptr, rows, cols, wr):
    """perm[new] = caller row, iperm[caller row] = new: inside every window a stable sort by (boundary rows, rows next
    to a boundary row, the rest), then descending degree (capped at 1023)."""
    out = rows // wr != cols // wr
    boundary = np.zeros(n, bool)
    boundary[rows[out]] = True
    boundary[cols[out]] = True
    near = np.zeros(n, bool)
    near[rows[boundary[cols]]] = True   # reads a boundary row
    near[cols[boundary[rows]]] = True   # is read by one
    cls = np.where(boundary, 0, np.where(near, 1, 2))
    deg = np.minimum(np.diff(indptr), 1023)
    pos = np.arange(n)
    perm = np.lexsort((pos, 1023 - deg, cls, pos // wr))
    iperm = np.empty(n, np.int64)
    iperm[perm] = pos
    return perm, iperm


class WindowRef(object):
    pass


def analyse(M, rings=True):
    """Everything the device tests compare: per-window counts, the predicted coverage of both rings, need, LDS bytes."""
    n = M.shape[0]
    indptr, rows, cols = offdiag(M)
    r = WindowRef()
    r.n, r.n_pad = n, n_pad_of(n)
    wr = r.win_rows = window_rows(r.n_pad)
    nw = r.n_windows = r.n_pad // wr
    rw, cw = rows // wr, cols // wr
    out = rw != cw
    r.entries = np.bincount(rw[out], minlength=nw)
    pair = np.unique(rw[out] * r.n_pad + cols[out])          # (window, outside row it reads), distinct
    cut = np.searchsorted(pair // r.n_pad, np.arange(nw + 1))
    r.reads = [pair[cut[A]:cut[A + 1]] % r.n_pad for A in range(nw)]
    n_reads = np.bincount(pair // r.n_pad, minlength=nw)
    adj = np.zeros((nw, nw), bool)
    adj[rw[out], cw[out]] = True                              # adj[A, B]: A reads B
    one = adj.T & ~adj                                        # one[A, B]: B reads A, A does not read B
    r.oneway = [np.flatnonzero(one[A]) for A in range(nw)]
    n_one = one.sum(axis=1)
    r.candidates = r.entries + n_one
    r.ghosts = n_reads + n_one
    read_rows = np.unique(cols[out])
    r.read_by_others = np.bincount(read_rows // wr, minlength=nw)
    r.need_lo = np.maximum(1, r.read_by_others)
    r.need_hi = np.maximum(1, np.bincount(np.union1d(read_rows, rows[out]) // wr, minlength=nw))
    r.pattern_symmetric = bool((sparse.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)) !=
                                sparse.csr_matrix((np.ones(len(rows)), (cols, rows)), shape=(n, n))).nnz == 0)
    r.max_degree = int(np.max(np.diff(indptr))) if n else 0
    # the order inside windows: slice widths, stored entries, the rows a window publishes
    perm, iperm = solver_order(n, indptr, rows, cols, wr)
    r.perm, r.iperm = perm, iperm
    deg_new = np.zeros(r.n_pad, np.int64)
    deg_new[:n] = np.diff(indptr)[perm]
    r.slice_width = deg_new.reshape(-1, SLICE).max(axis=1)
    r.sell_entries = int(r.slice_width.sum()) * SLICE
    r.covered = bool(nw <= WINDOWS_MAX and r.sell_entries > 0 and r.candidates.max() <= CAND_MAX and r.ghosts.max() <= GHOSTS_MAX)
    scol = iperm[cols]
    need = np.zeros(nw, np.int64)
    np.maximum.at(need, cw[out], scol[out] - cw[out] * wr + 1)
    r.need_exact = np.maximum(1, need)                        # (row 0 of every window is always published)
    r.lds = lds_need([r]) if r.covered else -1
    r.resident = bool(r.covered and 0 <= r.lds <= LDS_LIMIT)
    r.ring2 = r.ghosts2 = None
    r.covered2, r.lds2 = False, -1
    if rings and r.covered and wr == 1024:
        _second_ring(r, indptr, cols, scol)
    r.two_step = bool(r.covered2 and 0 <= r.lds2 <= LDS_LIMIT)
    return r


def _second_ring(r, indptr, cols, scol):
    wr, nw = r.win_rows, r.n_windows
    ring1, ring2, gw = [], [], np.zeros(nw, np.int64)
    cand = np.zeros(nw, np.int64)
    holds = np.zeros((nw, nw), bool)
    for A in range(nw):
        r1 = np.union1d(r.iperm[r.reads[A]], r.oneway[A] * wr)        # solver rows; row 0 of every one-way reader
        ring1.append(r1)
        if len(r1) == 0:
            ring2.append(np.zeros(0, np.int64))
            continue
        old = r.perm[r1]
        c = np.concatenate([scol[indptr[o]:indptr[o + 1]] for o in old])
        c = c[(c // wr != A) & ~np.isin(c, r1)]
        r2 = np.unique(c)
        ring2.append(r2)
        gw[A], cand[A] = r.slice_width[r1 // SLICE].max(), len(c)
        holds[A, np.concatenate([r1, r2]) // wr] = True
    r.ring1, r.ring2, r.ring1_width = ring1, ring2, gw
    r.ghosts2 = np.array([len(x) for x in ring2])
    # every condition on its own, so that a test can say WHICH limit refuses a matrix
    r.ring_checks = dict(ring1_rows=bool(r.ghosts.max() <= G1_MAX), ring2_candidates=bool(cand.max() <= CAND_MAX),
                         ring1_width=bool(gw.max() <= GW_MAX), both_rings=bool((r.ghosts + r.ghosts2).max() <= GHOSTS_MAX),
                         holds_symmetric=bool(np.array_equal(holds, holds.T)))
    r.covered2 = all(r.ring_checks.values())
    if r.covered2:
        worst = 0
        for A in range(nw):
            g1, g2, w = len(ring1[A]), len(ring2[A]), int(gw[A])
            g1p = (g1 + 63) & ~63
            need = ((16 + 1) * 4 + 15) & ~15
            need += (1024 + ((g1 + g2 + 1) & ~1)) * 8 + (1024 + ((g1 + 1) & ~1)) * 8 + g1p * 16 + w * g1p * 8 + g1p * 8
            need += ((g1 + g2 + 3) & ~3) * 4 + max(w - 8, 0) * g1p * 2
            sw = r.slice_width[A * 16:(A + 1) * 16]
            need += int(np.maximum(sw - 8, 0).sum()) * SLICE * 10 + 16
            worst = max(worst, need)
        r.lds2 = worst


def lds_need(refs):
    """Dynamic LDS of the one-step kernel for one graph or a pair (lds_need of pf_persist.hip); -1: no such kernel."""
    ng, wr = len(refs), refs[0].win_rows
    nwk = wr // 1024
    if any(x.win_rows != wr for x in refs) or (ng, nwk) not in ((1, 1), (2, 1), (1, 2), (2, 2), (1, 4)):
        return -1
    jr = 8 if ng * nwk <= 2 else 4
    per = wr // SLICE
    worst = 0
    for w in range(max(x.n_windows for x in refs)):
        need, ov = ((ng * nwk * 16 + 1) * 4 + 15) & ~15, 0
        for x in refs:
            if w >= x.n_windows:
                continue
            need += 2 * (wr + ((int(x.ghosts[w]) + 1) & ~1)) * 8
            ov += int(np.maximum(x.slice_width[w * per:(w + 1) * per] - jr, 0).sum()) * SLICE
        worst = max(worst, need + ov * 10 + 16)
    return worst


def pair_resident(a, b):
    """Does a paired application of two analysed graphs run as ONE resident launch?"""
    if not (a.covered and b.covered):
        return False
    need = lds_need([a, b])
    return 0 <= need <= LDS_LIMIT


# ------------------------------------------------------------------------------------------------------ matrices
def _symmetric_from_edges(n, i, j, rng):
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    w = -rng.uniform(0.1, 1.0, len(i))
    return sparse.csr_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n))


def empty_rows(n):
    e = np.zeros(n, bool)
    e[5::37] = True
    return e


def band_offdiag(n, seed=0, empties=True):
    """Symmetric band i +- 1, 2, 3 without wrap, weights in [-1, -0.1]; every 37th row (from row 5) and its column empty."""
    rng = np.random.default_rng(seed)
    i = np.concatenate([np.arange(n - k) for k in (1, 2, 3)])
    j = np.concatenate([np.arange(k, n) for k in (1, 2, 3)])
    if empties:
        e = empty_rows(n)
        keep = ~e[i] & ~e[j]
        i, j = i[keep], j[keep]
    return _symmetric_from_edges(n, i, j, rng)


def finish(W, seed=1):
    """Off-diagonals + a diagonal in [1, 3] on the rows that have entries (an empty row stays empty)."""
    W = sparse.csr_matrix(W)
    W.sum_duplicates()
    n = W.shape[0]
    rng = np.random.default_rng(seed)
    d = np.where(np.diff(W.indptr) > 0, rng.uniform(1.0, 3.0, n), 0.0)
    M = (W + sparse.diags(d)).tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def _live(n, lo, hi, margin=8):
    """Non-empty rows of [lo, hi) at least `margin` rows away from both ends."""
    r = np.arange(lo + margin, hi - margin)
    return r[~empty_rows(n)[r]]


def plant_rows(M, *arrays):
    """The rows whose vector entries the device tests make O(1): ends of every window and everything planted."""
    return np.unique(np.concatenate([np.asarray(a, np.int64).ravel() for a in arrays])) if arrays else np.zeros(0, np.int64)


def ghost_case(target, n=8192, seed=3):
    """Rows of window 2 read `k` distinct rows of a contiguous run of window 5, and back: max(ghosts) == target."""
    rng = np.random.default_rng(seed)
    W = band_offdiag(n)
    base = analyse(finish(W), rings=False)
    k = target - int(base.ghosts[2])
    src = _live(n, 2048, 3072)
    assert 0 < k <= 1024 and base.ghosts[5] + min(k, len(src)) <= target
    i, j = src[np.arange(k) % len(src)], 5120 + np.arange(k)  # (the run takes window 5's empty rows along)
    M = finish(W + _symmetric_from_edges(n, i, j, rng))
    return M, plant_rows(M, i, j)


def candidate_case(target, n=8192, seed=4):
    """One way: the rows of window 3 all read the same five rows of window 6; candidates[3] == target.  Window 6 reads
    nothing of window 3, so it gets row 0 of window 3 as an extra outside row."""
    rng = np.random.default_rng(seed)
    W = band_offdiag(n)
    base = analyse(finish(W), rings=False)
    k = target - int(base.candidates[3])
    src, dst = _live(n, 3072, 4096, margin=0), _live(n, 6144, 7168)[100:105]
    assert 0 < k <= len(src) * len(dst)
    i, j = np.tile(src, len(dst))[:k], np.repeat(dst, len(src))[:k]
    M = finish(W + sparse.csr_matrix((-rng.uniform(0.1, 1.0, k), (i, j)), shape=(n, n)))
    return M, plant_rows(M, i, j)


def ring_width_case(degree, n=8192, seed=5):
    """Row 4096 - window 4's first row, a ring-1 row of window 3 - gets in-window neighbours up to `degree` entries."""
    rng = np.random.default_rng(seed)
    W = band_offdiag(n)
    r0 = 4096
    have = int(np.diff(W.indptr)[r0])
    j = _live(n, 4096, 5120, margin=16)[::7][:degree - have]
    assert len(j) == degree - have
    i = np.full(len(j), r0)
    M = finish(W + _symmetric_from_edges(n, i, j, rng))
    return M, plant_rows(M, i, j)


def spill_case(wide=True, n=8192, seed=6):
    """In-window rows of degree 9, 16 and 40 (window 1) and, if `wide`, one row of degree 300 across windows 3, 4, 5."""
    rng = np.random.default_rng(seed)
    W = band_offdiag(n)
    ii, jj = [], []
    have = np.diff(W.indptr)

    def widen(r0, degree, pool):
        others = pool[np.abs(pool - r0) > 3][:degree - have[r0]]
        assert len(others) == degree - have[r0]
        ii.append(np.full(len(others), r0))
        jj.append(others)

    live = _live(n, 1024, 2048, margin=16)
    for r0, degree, step in ((live[100], 9, 3), (live[300], 16, 5), (live[500], 40, 7)):
        widen(r0, degree, live[step::step + 8])
    if wide:
        widen(4096 + 511, 300, np.concatenate([_live(n, lo, lo + 1024)[::9][:100] for lo in (3072, 4096, 5120)]))
    i, j = np.concatenate(ii), np.concatenate(jj)
    M = finish(W + _symmetric_from_edges(n, i, j, rng))
    return M, plant_rows(M, i, j)


def shape_case(kind):
    if kind == "n2":
        return finish(_symmetric_from_edges(2, [0], [1], np.random.default_rng(7))), np.zeros(0, np.int64)
    if kind in ("n4096", "n4097", "n5000"):
        return finish(band_offdiag(int(kind[1:]))), np.zeros(0, np.int64)
    if kind == "block_diagonal":
        W = band_offdiag(8192).tocoo()
        keep = W.row // 1024 == W.col // 1024
        return finish(sparse.csr_matrix((W.data[keep], (W.row[keep], W.col[keep])), shape=W.shape)), np.zeros(0, np.int64)
    if kind == "diagonal":
        return sparse.diags(np.random.default_rng(8).uniform(1.0, 3.0, 4096)).tocsr(), np.zeros(0, np.int64)
    raise KeyError(kind)


def large_case(n, seed=9, edges=300):
    """The band at n rows (2048- or 4096-row windows) plus `edges` symmetric long-range edges between distinct live rows,
    each row taking at most two of them: rows of degree 5 (next to an empty row) to 8."""
    rng = np.random.default_rng(seed)
    W = band_offdiag(n)
    live = np.flatnonzero(~empty_rows(n))
    pick = rng.choice(live, 2 * edges, replace=False)
    half = edges // 2  # (half of the picked rows take a second edge)
    i, j = np.concatenate([pick[:edges], pick[:half]]), np.concatenate([pick[edges:], np.roll(pick[edges:edges + half], 1)])
    M = finish(W + _symmetric_from_edges(n, i, j, rng))
    return M, plant_rows(M, i, j)


CASES = {
    "ghosts1024": lambda: ghost_case(1024), "ghosts1025": lambda: ghost_case(1025),
    "ghosts512": lambda: ghost_case(512), "ghosts513": lambda: ghost_case(513),
    "cand4096": lambda: candidate_case(4096), "cand4097": lambda: candidate_case(4097),
    "ringrow16": lambda: ring_width_case(16), "ringrow17": lambda: ring_width_case(17),
    "spill": lambda: spill_case(False), "spill300": lambda: spill_case(True),
    "n2": lambda: shape_case("n2"), "n4096": lambda: shape_case("n4096"), "n4097": lambda: shape_case("n4097"),
    "n5000": lambda: shape_case("n5000"), "block_diagonal": lambda: shape_case("block_diagonal"),
    "diagonal": lambda: shape_case("diagonal"),
}
LARGE = {"rows2048": (266240, 9), "rows2048b": (266240, 10), "rows4096": (528384, 9)}  # (n, seed)

_built = {}


def case(name):
    """(matrix, planted rows, analysis) of a named case, built once per process and never changed."""
    if name not in _built:
        M, rows = CASES[name]() if name in CASES else large_case(*LARGE[name])
        _built[name] = (M, rows, analyse(M))
    return _built[name]
