#!/usr/bin/env python3
"""Dense correspondences between two samplings of one surface from their Laplace-Beltrami spectra alone: heat and wave
kernel signatures, a functional map fitted to them, its point map, ZoomOut.

    python examples/descriptor_correspondences.py [target.vtk source.vtk]"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pyfocusr_amd as pf  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

if len(sys.argv) == 3:
    target, source = pf.read_vtk_mesh(sys.argv[1]), pf.read_vtk_mesh(sys.argv[2])
else:
    target, source = blob_mesh(700, seed=0), blob_mesh(900, seed=0)  # one surface, sampled twice

T, C = pf.descriptor_correspondences(target, source, k_init=8, k_end=20)
print("functional map %s, diagonal %s" % (C.shape, np.round(np.abs(np.diag(C))[:6], 2)))
print("mean distance source vertex -> matched target vertex: %.4f"
      % np.mean(np.linalg.norm(np.asarray(target.points)[T] - np.asarray(source.points), axis=1)))

vals, vecs = pf.laplace_beltrami_spectrum(source, 20)
hks, times = pf.heat_kernel_signature(vals, vecs, n_times=16)
pf.signature_on_mesh(source, hks[:, [0, 8, 15]], "hks")  # three scales, stored as point data hks_0 .. hks_2
print("stored:", [name for name, _ in source.point_data])
