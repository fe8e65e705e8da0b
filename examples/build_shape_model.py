#!/usr/bin/env python3
"""A statistical shape model of a population of surfaces: every subject expressed on one template's vertices, generalized
Procrustes alignment, principal modes, and the scores of a new subject.

    python examples/build_shape_model.py [template.vtk subject1.vtk subject2.vtk ...] [--register]

Without files the population is synthetic: one blob under two smooth deformations with random amplitudes, every subject
in its own pose and size.  With `--register` (and always with files) the subjects' vertices are NOT taken to correspond:
each subject is registered to the template with `Focusr` first (`population_from_template`), one run per subject."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pyfocusr_amd as pf  # noqa: E402
from pyfocusr_amd.meshgen import blob_mesh  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--register"]
register = "--register" in sys.argv[1:] or len(args) >= 3

rng = np.random.default_rng(0)
if len(args) >= 3:
    template, subjects = pf.read_vtk_mesh(args[0]), [pf.read_vtk_mesh(a) for a in args[1:]]
else:
    template = blob_mesh(700, seed=0)
    P = np.asarray(template.points) - np.asarray(template.points).mean(0)
    stretch = np.zeros_like(P)
    stretch[:, 0] = P[:, 0]
    bend = np.zeros_like(P)
    bend[:, 1] = P[:, 1] * P[:, 2]
    subjects = []
    for s in range(5 if register else 12):
        shape = P + 0.15 * rng.standard_normal() * stretch + 0.1 * rng.standard_normal() * bend
        Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        Q = Q * np.sign(np.linalg.det(Q))
        subjects.append(pf.PolyMesh(rng.uniform(0.8, 1.2) * shape @ Q.T + rng.standard_normal(3), np.asarray(template.faces).copy()))

if register:  # the template's vertices on every subject: (S, n_template, 3)
    shapes = pf.population_from_template(template, subjects, positions="weighted", n_spectral_features=3, verbose=False)
else:  # the synthetic subjects share the template's vertices already
    shapes = np.ascontiguousarray(np.stack([np.asarray(m.points, dtype=np.float64) for m in subjects]))

areas = pf.discrete_curvatures(template).area  # the template's vertex areas weight every sum
model = pf.build_shape_model(shapes, weights=areas, scaling=True)
print("%d shapes of %d points: %d alignment iterations, %d modes" % (shapes.shape[0], shapes.shape[1], len(model.history), model.n_modes))
print("explained variance:", np.round(model.explained_variance_ratio[:5], 4), "compactness:", np.round(model.compactness()[:5], 4))

b = model.project(shapes[0])  # a subject in any pose: aligned to the mean first
print("scores of subject 0 (in standard deviations):", np.round(b[:3] / np.sqrt(model.eigenvalues[:3]), 2))
print("largest distance of its reconstruction from two modes: %.3g"
      % np.max(np.linalg.norm(model.reconstruct(b[:2]) - model.reconstruct(b), axis=1)))

for sign in (-2.0, 2.0):  # the first mode at -2 and +2 standard deviations, as meshes of the template's connectivity
    mesh = model.mode_on_mesh(template, 0, sign)
    print("mode 0 at %+.0f sd: extent" % sign, np.round(np.ptp(np.asarray(mesh.points), axis=0), 3))
