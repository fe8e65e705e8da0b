#!/usr/bin/env python3
"""Time the device assignment (`euclidean_assignment` / `pf_assign`) against scipy's
`linear_sum_assignment(cdist(A, B))`.

Inputs: the bundled pairs' spectral coordinates (`coords_s_w` -> `coords_t_w`): 2k (the first 2000 rows of pair_5k),
5k (pair_5k), 15k (pair_15k, 14996 x 14998, d = 5); then the device alone at 50k and 250k on a synthetic 5-D embedding
(a smooth image of a 3-D cloud against its shuffled copy, displaced by a quarter of the point spacing).  scipy runs up
to --scipy-max rows (the 15k pair takes about three minutes of one CPU core).  One JSON line per size.

    python tools/bench_assign.py [--scipy-max 15000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(n, 3))
    A = np.stack([x[:, 0], x[:, 1], x[:, 2], 0.5 * x[:, 0] * x[:, 1], 0.5 * np.sin(2 * x[:, 2])], axis=1)
    B = A[rng.permutation(n)] + rng.normal(scale=0.25 * n ** (-1.0 / 3.0), size=A.shape)
    return A, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scipy-max", type=int, default=15000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="2k,5k,15k,50k,250k")
    args = ap.parse_args()
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist

    from pyfocusr_amd import _hip

    ctx = _hip.default_context()
    golden = os.path.join(REPO, "tests", "golden")
    for size in args.sizes.split(","):
        if size in ("2k", "5k", "15k"):
            with np.load(os.path.join(golden, "pair_15k.npz" if size == "15k" else "pair_5k.npz")) as z:
                A, B = np.ascontiguousarray(z["coords_s_w"]), np.ascontiguousarray(z["coords_t_w"])
            if size == "2k":
                A, B = A[:2000].copy(), B[:2000].copy()
            source = "pair_15k" if size == "15k" else "pair_5k"
        else:
            A, B = synthetic(int(size[:-1]) * 1000, seed=7)
            source = "synthetic"
        ctx.assign(A[:64], B[:64])  # module load, first launches
        times, stats, col = [], None, None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            col, stats = ctx.assign(A, B)
            times.append(time.perf_counter() - t0)
        out = dict(size=size, source=source, n_rows=A.shape[0], n_cols=B.shape[0], d=A.shape[1],
                   device_s=min(times), device_s_all=times, stats=stats.as_dict(),
                   dense_bid_share=stats.dense_bids / max(stats.bids + stats.dense_bids, 1))
        if A.shape[0] <= args.scipy_max:
            t0 = time.perf_counter()
            _, cs = linear_sum_assignment(cdist(A, B))
            out["scipy_s"] = time.perf_counter() - t0
            out["equal_to_scipy"] = bool(np.array_equal(col, cs))
            out["speedup"] = out["scipy_s"] / out["device_s"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
