"""Time of a statistical shape model of a synthetic population (profiles/shape_model.md).

    python tools/bench_shape_model.py --S 100 --n 250000 --repeats 3

The population: one blob under `--planted` smooth deformations with random amplitudes plus a little noise, every shape
under a random similarity transform.  One JSON line:

* `build_ms`: the whole call `build_shape_model(shapes)` (host clock: argument checks, one upload, the alignment's
  iterations with their 3 x 3 SVDs on the host, Gram, `eigh`, the modes and the scores, every download), first call
  discarded, median and spread of the repeats; `gpa_iterations`, `n_modes`;
* `primitive_ms`: per primitive of `_hip.DeviceShapes` on the resident population the whole call and the library's own
  device time (`device_ms`, HIP events between the call's uploads and downloads), medians of the repeats; `combine` and
  `scores` with `--modes` modes;
* `numpy_ms`: what a numpy user would write for the same model on the same host (vectorised Procrustes loop with
  `einsum`, PCA through the Gram matrix), and how far the two models' eigenvalues are apart."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(REPO)


def _stats(values):
    return dict(median=float(np.median(values)), min=float(np.min(values)), max=float(np.max(values)))


def _rotation(rng):
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0.0:
        Q[:, 2] = -Q[:, 2]
    return Q


def population(S, n, planted, seed):
    from pyfocusr_amd.meshgen import blob_mesh

    P = np.ascontiguousarray(blob_mesh(n, seed=seed).points, dtype=np.float64)
    P = P - P.mean(0)
    n = len(P)
    rng = np.random.default_rng(seed)
    size = np.sqrt(np.sum(P * P) / n)
    fields = []
    for j in range(planted):  # smooth fields: a coordinate function times a direction
        f = np.zeros_like(P)
        f[:, j % 3] = P[:, (j + 1) % 3] * (P[:, (j + 2) % 3] if j >= 3 else 1.0)
        fields.append(f / np.sqrt(np.sum(f * f) / n))
    X = np.empty((S, n, 3))
    for s in range(S):
        shape = P + 0.002 * size * rng.standard_normal(P.shape)
        for j, f in enumerate(fields):
            shape = shape + (0.1 * size / (j + 1)) * rng.standard_normal() * f
        X[s] = rng.uniform(0.7, 1.3) * (shape @ _rotation(rng).T) + 5.0 * size * rng.standard_normal(3)
    return X


def numpy_model(X, max_iter, tol):
    """The same alignment and Gram PCA in vectorised numpy (no fixed summation order): (eigenvalues, iterations)."""
    S, n = X.shape[:2]
    X = X - X.mean(1, keepdims=True)
    X = X / np.sqrt(np.einsum("sna,sna->s", X, X) / n)[:, None, None]
    ref = X[0]
    for it in range(max_iter):
        H = np.einsum("sna,nb->sab", X, ref)
        q = np.einsum("sna,sna->s", X, X)
        rho = np.sqrt(np.sum(ref * ref) / n)
        U, sv, Vt = np.linalg.svd(H)
        d = np.ones((S, 3))
        d[:, 2] = np.sign(np.linalg.det(U @ Vt))
        R = (U * d[:, None, :]) @ Vt
        X = (np.sum(sv * d, axis=1) / (rho * q))[:, None, None] * (X @ R)
        mean = X.mean(0)
        change = np.sum((mean - ref) ** 2)
        ref = mean
        if np.sqrt(change / n) < tol * rho:
            break
    D = (X - ref).reshape(S, -1)
    lam = np.linalg.eigh(D @ D.T / (S - 1))[0][::-1]
    return lam, it + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=100)
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--planted", type=int, default=5)
    ap.add_argument("--modes", type=int, default=10, help="modes of the timed combine and scores calls")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy timing")
    args = ap.parse_args()

    from pyfocusr_amd import _hip, build_shape_model

    X = population(args.S, args.n, args.planted, args.seed)
    S, n = X.shape[:2]
    ctx = _hip.default_context()
    builds, model = [], None
    for it in range(1 + args.repeats):
        ctx.sync()
        t0 = time.perf_counter()
        model = build_shape_model(X, n_modes=min(args.modes, S - 1), tol=args.tol, max_iter=args.max_iter, ctx=ctx)
        if it > 0:
            builds.append(1e3 * (time.perf_counter() - t0))
    out = dict(S=S, n=n, planted=args.planted, repeats=args.repeats, build_ms=_stats(builds), gpa_iterations=int(len(model.history)),
               n_modes=int(model.n_modes), population_mb=X.nbytes / 2**20,
               explained_variance_ratio=[float(v) for v in model.explained_variance_ratio[:args.planted + 1]])

    rng = np.random.default_rng(args.seed + 1)
    K = min(args.modes, S)
    R, coeff, modes = np.stack([_rotation(rng) for _ in range(S)]), rng.standard_normal((K, S)), rng.standard_normal((K, n, 3))
    t0 = time.perf_counter()
    dev = _hip.DeviceShapes(X, ctx=ctx)
    out["create_ms"] = 1e3 * (time.perf_counter() - t0)
    calls = [("center", dev.center), ("align_sums", dev.align_sums), ("transform", lambda: dev.transform(R, np.ones(S))),
             ("mean", lambda: dev.mean(return_mean=False)), ("gram", dev.gram), ("combine", lambda: dev.combine(coeff)),
             ("scores", lambda: dev.scores(modes))]
    primitive = {}
    dev.device_ms(True)
    for name, call in calls:
        rows = []
        for it in range(1 + args.repeats):
            t0 = time.perf_counter()
            call()
            rows.append((1e3 * (time.perf_counter() - t0), dev.device_ms(True)))
        a = np.array(rows[1:])
        primitive[name] = dict(call_ms=float(np.median(a[:, 0])), device_ms=float(np.median(a[:, 1])))
    dev.close()
    out["primitive_ms"] = primitive
    out["timed_modes"] = K
    if not args.no_reference:
        times = []
        for _ in range(max(1, min(args.repeats, 2))):
            t0 = time.perf_counter()
            lam, its = numpy_model(X, args.max_iter, args.tol)
            times.append(1e3 * (time.perf_counter() - t0))
        k = model.n_modes
        out.update(numpy_ms=_stats(times), numpy_iterations=int(its),
                   eigenvalues_relative_difference=float(np.max(np.abs(lam[:k] - model.eigenvalues) / model.eigenvalues[0])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
