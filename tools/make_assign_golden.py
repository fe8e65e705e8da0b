#!/usr/bin/env python3
"""Generate `tests/golden/assign_pairs.npz`: scipy's optimal one-to-one assignment of the spectral coordinates of the
two bundled pairs (CPU only, no GPU, no oracle).

    pair_5k:  coords_s_w (5000 x 3)  -> coords_t_w (5000 x 3)
    pair_15k: coords_s_w (14996 x 5) -> coords_t_w (14998 x 5)   (rectangular)

For each pair the file holds `<name>_col_ind` (int64, scipy's `col_ind` of `linear_sum_assignment(cdist(A, B))`;
`row_ind` is `arange(n_A)`) and `<name>_total_cost` (float64, the sum of the assigned distances).  The 15k pair takes
about three minutes of one CPU core and 1.8 GB of host memory.

    python tools/make_assign_golden.py
"""
import os
import time

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def main():
    out = {}
    for name in ("pair_5k", "pair_15k"):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            a, b = np.ascontiguousarray(z["coords_s_w"]), np.ascontiguousarray(z["coords_t_w"])
        t0 = time.perf_counter()
        cost = cdist(a, b)
        rows, cols = linear_sum_assignment(cost)
        dt = time.perf_counter() - t0
        assert np.array_equal(rows, np.arange(a.shape[0]))
        out[name + "_col_ind"] = cols.astype(np.int64)
        out[name + "_total_cost"] = np.float64(cost[rows, cols].sum())
        print("%s: %d x %d, d = %d, total cost %.17g, %.1f s" % (name, a.shape[0], b.shape[0], a.shape[1],
                                                                 out[name + "_total_cost"], dt), flush=True)
        del cost
    np.savez_compressed(os.path.join(GOLDEN, "assign_pairs.npz"), **out)


if __name__ == "__main__":
    main()
