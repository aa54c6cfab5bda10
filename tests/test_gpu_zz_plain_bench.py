"""A plain `bench.py` run (no --full) on a small workload: it times the steps it is asked for and prints the line, with none of the side legs
(CPU baseline, parity legs, bootstraps, child runs), and --dump-outputs writes the last step's result as float64 .npy files that two runs
with the same arguments reproduce exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("est_counts", "tpm", "eff_lens", "alpha_before_zeroes", "flens", "n_processed", "em_rounds")


def _plain_run(tmp_path, tag, pairs, steps):
    import bench
    env = dict(os.environ, KAMD_BENCH_CACHE=str(tmp_path / "cache"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "KAMD_BENCH_SHARE_GPU"):
        env.pop(k, None)
    out = tmp_path / f"dump_{tag}"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genes", "1500", "--pairs", str(pairs), "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(out), "--detail-file", str(tmp_path / f"detail_{tag}.json")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < bench.CONTRACT_MAX_BYTES, lines
    return json.loads(lines[0]), {k: np.load(out / f"{k}.npy") for k in NAMES}, sorted(os.listdir(out))


def test_plain_bench_is_lean_and_dumps_reproducible_outputs(tmp_path):
    import bench
    if not os.path.exists(bench.REF_BIN):
        pytest.skip("oracle/_ref/kallisto not built: cannot create the index of the bench workload")
    pairs = 200_000
    line, a, files = _plain_run(tmp_path, "a", pairs, 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(pairs / line["ms_per_step"] / 1e3, rel=5e-3)   # M pairs/s from the same clock as ms_per_step
    for k in ("cpu_baseline", "stress", "gencode_size", "bootstrap", "other_scaling", "config2"):
        assert k not in line, k
    assert all(v is None for v in line["parity"].values()), line["parity"]
    assert files == sorted(f"{k}.npy" for k in NAMES)
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert a["n_processed"][0] == pairs and a["em_rounds"][0] >= 1 and a["flens"].sum() > 0
    assert np.all(a["est_counts"] >= 0) and abs(a["tpm"].sum() - 1e6) < 1e-3
    assert a["est_counts"].shape == a["tpm"].shape == a["eff_lens"].shape == (line["config"]["targets"],)
    line_b, b, _ = _plain_run(tmp_path, "b", pairs, 3)
    assert line_b["steps"] == 3
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
