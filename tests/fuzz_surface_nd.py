#!/usr/bin/env python3
"""Randomised sweep of `pf_surface_nd_closest` on hostile geometry: each case draws a mesh and a frame as
tests/fuzz_surfaces.py does, a depth d = 1 ... 16, embeds mesh and queries (`_hostile_geometry.embedded_case`, under the same
frame) and checks pruned = exhaustive = the numpy brute force bit for bit, a permutation of the queries and a scaling by a
power of two (tests/_surface_checks.py: `check_nd`).  Not collected by pytest:
python tests/fuzz_surface_nd.py SEED N_CASES [--poison]   on the GPU box.
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
    d = int(rng.integers(1, 17))
    n = int(rng.choice(hg.QUERY_COUNTS, p=[0.06] * 8 + [0.52]))
    q, _ = hg.queries(mesh, n, seed=int(rng.integers(0, 2 ** 31)))
    k, s, offset = mesh[2]["frame"]
    coords, faces, qd = hg.embedded_case(mesh, q[:hg.ND_ROWS], d, k, s, offset)
    what = "%s, d = %d, %d fan triangles, %d queries" % (mesh[2]["name"], d, len(sc.sref.fan_triangles(faces)), len(qd))
    try:
        stats = sc.check_nd(_hip, ctx, coords, faces, qd, want=sc.nd_reference(coords, faces, qd), order_seed=it,
                            pow2_k=int(rng.choice([-20, -3, 7, 20])))
        print("ok   case %d: %s %s" % (it, what, stats), flush=True)
    except AssertionError:
        fails += 1
        print("FAIL case %d: %s\n%s" % (it, what, traceback.format_exc()[-900:]), flush=True)
print("done: %d failures of %d, %.1fs" % (fails, N, time.time() - t0))
