#!/usr/bin/env python3
"""Randomised sweep of the surface queries on hostile geometry: each case draws a generator of tests/_hostile_geometry.py
(blob, torus of quads, needles, coincident sheets, soup, anisotropic, far parts, outlier), a frame (2^k s, an offset of 0 to
1e6 extents), sizes from its lists and a query and ray mix, then runs closest, distance, signed distance, winding numbers
(exact and beta = 2), ray casts and vertex normals against the brute-force references by tests/_surface_checks.py, and
the query-order check.  Not collected by pytest:  python tests/fuzz_surfaces.py SEED N_CASES [--poison]   on the GPU box.
`--poison`: case i runs under `pf_pool_poison(i % 3)` (off, 0xFF bytes, zero bytes); the checks are the same.
An AssertionError is a counted failure and the sweep goes on; any other exception (a `PfError` included: no case asks for a
refusal) ends the sweep at once with a non-zero exit, so that nothing more is started on a device that reported an error."""
import os
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
try:
    import torch  # noqa: F401,E402  (before the library: one HIP runtime for both, as tests/conftest.py does)
except ImportError:
    pass
import _hostile_geometry as hg  # noqa: E402
import _surface_checks as sc  # noqa: E402
from pyfocusr_amd import _hip  # noqa: E402

ctx = _hip.default_context()
rng = np.random.default_rng(int(sys.argv[1]))
N = int(sys.argv[2])
POISON = "--poison" in sys.argv[3:]
fails, t0 = 0, time.time()
for it in range(N):
    if POISON:
        _hip.pool_poison(it % 3)
    mesh = hg.draw_mesh(rng)
    n = int(rng.choice(hg.QUERY_COUNTS, p=[0.06] * 8 + [0.52]))
    q, _ = hg.queries(mesh, n, seed=int(rng.integers(0, 2 ** 31)))
    dirs, _ = hg.rays(mesh, q, seed=int(rng.integers(0, 2 ** 31)))
    what = "%s, %d fan triangles, %d queries" % (mesh[2]["name"], len(sc.sref.fan_triangles(mesh[1])), n)
    try:
        R = sc.Reference(mesh, q, dirs)
        assert R.within_caps(), ("a generator defect: the filters leave out too much", R.figures())
        surf = _hip.DeviceSurface(mesh[0], mesh[1], ctx=ctx)
        try:
            out = sc.run_all(surf, q, dirs)
            fig = sc.check_against_reference(out, R)
            sc.check_query_order(surf, q, dirs, out, seed=it)
        finally:
            surf.close()
        print("ok   case %d: %s %s" % (it, what, {k: float("%.3g" % v) for k, v in dict(R.figures(), **fig).items()}), flush=True)
    except AssertionError:
        fails += 1
        print("FAIL case %d: %s\n%s" % (it, what, traceback.format_exc()[-900:]), flush=True)
print("done: %d failures of %d, %.1fs" % (fails, N, time.time() - t0))
