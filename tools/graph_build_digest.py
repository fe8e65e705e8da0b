#!/usr/bin/env python3
"""Do two builds of the library build the same graphs, to the bit?  (profiles/graph_build_refactor.md)

    PYFOCUSR_HIP_LIB=/path/to/one/libpyfocusr_hip.so python tools/graph_build_digest.py > a.txt
    PYFOCUSR_HIP_LIB=/path/to/other/libpyfocusr_hip.so python tools/graph_build_digest.py > b.txt
    diff a.txt b.txt

One line per array, "<graph> <what> <shape> <sha256 of its raw bytes>".  Per graph: the fields of `pf_graph_get_info`,
every array of `pf_graph_download` (labels included), `pf_graph_window_info` with the second ring asked for (both states,
both outside-row counts, the published rows), and one resident filter application (degree 9) on a fixed vector, made the
way tests/test_resident_windows.py makes it.  The graphs sit at the smallest sizes where each path of the build can go
wrong:
    blob4095      general sort (n < 4096)                 blob4097    order by counting, more than one chunk
    blob20000     20 windows                              piled       the counting sort gives up: the robust rebuild
    repeated      repeated directed edges (k_compact_rows has work)
    open          faces removed: asymmetric W, the second-ring check refuses
    matrix20000   blob20000's W handed in as a matrix: no geometry
    cotan5000     a cotangent graph: pf_compute_order with points and without an m-space
    blob263000 / blob525000   n_pad above 262 144 / 524 288: windows of 2048 / 4096 rows
and two pair builds (`pf_graph_build_device2`), clean + clean and clean + shrinking, each in both orders.
A tool, not a test: no digest is kept as a golden file."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def line(graph, what, array):
    a = np.ascontiguousarray(array)
    print("%-22s %-20s %-12s %s" % (graph, what, "x".join(str(s) for s in a.shape) or "scalar", hashlib.sha256(a.tobytes()).hexdigest()))


def graph_lines(hip, name, dev, radius=1.0):
    """Everything the build left behind in `dev`, then one filter application.  radius: c = e of the filter (the operators of
    mesh graphs have their spectrum in [0, 2]; a matrix brings its Gershgorin radius)."""
    print("%-22s %-20s %s" % (name, "info", " ".join("%s=%r" % kv for kv in sorted(dev.info.as_dict().items()))))
    print("%-22s %-20s %d" % (name, "rows_compacted", dev.rows_compacted))
    out = dev.download(labels=True)
    for key in sorted(out):
        line(name, "download." + key, out[key])
    win = dev.window_info(rings=True)
    print("%-22s %-20s win_rows=%d n_windows=%d state=%d state2=%d" % (name, "window_info", win["win_rows"], win["n_windows"], win["state"], win["state2"]))
    for key in ("ghosts", "ghosts2", "need"):
        if win[key] is not None:
            line(name, "window_info." + key, win[key])
    rng = np.random.default_rng(dev.n)
    x = 1e-3 * rng.standard_normal(dev.n)
    idx = np.arange(0, dev.n, 257)
    x[idx] = rng.uniform(1.0, 2.0, len(idx))
    before = hip.persist_state(dev.ctx)["launches"]
    dev.ws_ensure(4)
    dev.upload(0, x)
    dev.cheb(0, 1, 9, radius, radius, 1.0)
    line(name, "cheb9", dev.download_slots(1, 1)[:, 0])
    print("%-22s %-20s %d" % (name, "resident_launches", hip.persist_state(dev.ctx)["launches"] - before))


def main():
    from scipy import sparse

    from pyfocusr_amd import _hip as hip
    from pyfocusr_amd.meshgen import blob_mesh, messy_blob_mesh

    hip.load_library()
    print("library: %s" % hip.LIB_PATH, file=sys.stderr)
    ctx = hip.default_context()

    def single(name, points, faces, **kw):
        dev = hip.DeviceLaplacian(points, faces, ctx=ctx, **kw)
        try:
            graph_lines(hip, name, dev)
        finally:
            dev.close()

    for n in (4095, 4097, 20000):
        m = blob_mesh(n, seed=n % 97)
        single("blob%d" % n, m.points, m.faces)
    b20 = blob_mesh(20000, seed=20000 % 97)

    m = blob_mesh(8000, seed=31)  # tests/test_gpu_parity.py::test_assembly_piled_vertices
    n0 = len(m.points)
    pts = np.concatenate([m.points * 1e-3, [[900.0, 0.0, 0.0], [0.0, -700.0, 0.0], [0.0, 0.0, 800.0]]])
    single("piled", pts, np.concatenate([m.faces, [[n0, n0 + 1, n0 + 2], [0, n0, n0 + 1]]]).astype(np.int32))

    m = blob_mesh(6000, seed=16)
    single("repeated", m.points, np.concatenate([m.faces, np.repeat(m.faces[11:40], 3, axis=0)]).astype(np.int32))
    single("open", b20.points, b20.faces[np.arange(len(b20.faces)) % 7 != 3])

    dev = hip.DeviceLaplacian(b20.points, b20.faces, ctx=ctx)
    h = dev.download()
    dev.close()
    W = sparse.csr_matrix((h["w"], h["colidx"], h["rowptr"]), shape=(b20.points.shape[0],) * 2)
    L = sparse.csr_matrix(sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W)
    L.sort_indices()
    dev = hip.DeviceLaplacian(matrix=(L.indptr, L.indices, L.data), ctx=ctx)
    try:
        graph_lines(hip, "matrix20000", dev, radius=float(np.max(abs(L) @ np.ones(L.shape[0]))))
    finally:
        dev.close()

    m = blob_mesh(5000, seed=5)
    dev = hip.DeviceLaplacian(m.points, m.faces, ctx=ctx, cotangent=True)
    try:
        graph_lines(hip, "cotan5000", dev, radius=0.5 * dev.hi)
    finally:
        dev.close()

    for n in (263000, 525000):
        m = blob_mesh(n, seed=n % 97)
        single("blob%d" % n, m.points, m.faces)

    messy = messy_blob_mesh(20000, seed=15)  # tests/test_front_of_step.py: rows that shrink
    clean2 = blob_mesh(9000, seed=12)
    meshes = dict(blob20000=b20, blob9000=clean2, messy20000=messy)
    for na, nb in (("blob20000", "blob9000"), ("blob9000", "blob20000"), ("blob20000", "messy20000"), ("messy20000", "blob20000")):
        a, b = meshes[na], meshes[nb]
        ma, mb = hip.DeviceMesh(a.points, a.faces, ctx=ctx), hip.DeviceMesh(b.points, b.faces, ctx=ctx)
        da, db = hip.DeviceLaplacian.build_pair(ma, mb)
        try:
            graph_lines(hip, "%s+%s:a" % (na, nb), da)
            graph_lines(hip, "%s+%s:b" % (na, nb), db)
        finally:
            da.close()
            db.close()
            ma.close()
            mb.close()


if __name__ == "__main__":
    main()
