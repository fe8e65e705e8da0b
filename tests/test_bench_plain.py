"""`bench.py` without `--full`: set-up, warm-up, the timed steps, `--dump-outputs` and the result line - none of the
measurements that take runs of their own (those are `--full`'s).  GPU: one small pair, in a fresh process."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only `--full` puts in the line (`split_pair` needs two ranks as well)
FULL_ONLY = ("roofline_streaming_kernel", "bundled_15k_pair", "single_graph_solve", "messy_250k_pair", "c5_1m_k10",
             "cpu_baseline", "parity_at_full_size", "speedup_vs_cpu_baseline", "split_pair")


@pytest.mark.gpu
def test_plain_bench_run_is_lean(tmp_path):
    steps, k = 2, 5
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--vertices", "20000", "--dump-outputs", str(tmp_path / "dump")],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["metric"].startswith("lowest-k eigenpairs/sec") and line["unit"] == "eigenpairs/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == steps
    assert line["value"] == pytest.approx(2 * k / (1e-3 * line["ms_per_step"]), rel=1e-12)
    assert sorted(set(FULL_ONLY) & set(line)) == []
    assert "achievable_hbm_copy_GBps" not in line["roofline"] and "skipped" in line["roofline_knn"]
    assert line["roofline_assembly"]["ms_per_step"] > 0 and line["max_eig_residual"] < 1e-6
    assert sorted(os.listdir(tmp_path / "dump")) == ["correspondence.npy", "source_eig_vals.npy", "source_eig_vecs.npy",
                                                    "spectral_weights.npy", "target_eig_vals.npy", "target_eig_vecs.npy"]
