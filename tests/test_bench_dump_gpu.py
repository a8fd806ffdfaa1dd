"""bench.py --dump-outputs on the device: what the last timed step returned, one file per array, consistent with the
bench line the same run prints (forward, sampling-direction and trainer paths)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload,names", [("config2", {"z", "sums"}), ("config4", {"x"}),
                                            ("config2_train", {"z", "reconstruction", "sums", "theta", "grad"})])
def test_bench_dump_outputs_write_the_last_timed_step(workload, names, tmp_path):
    import bench
    from gnf_amd.flow import log_prob_from_sums
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", workload, "--steps", "3", "--warmup", "1",
           "--repeats", "2", "--prewarm-ms", "0", "--no-cpu-baseline", "--no-secondary", "--latency-steps", "0",
           "--kernel-timing-steps", "1", "--graphs-per-gpu", "16", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=800, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads(lines[0])
    assert set(line["dumped_outputs"]) == names and sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    a = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    n, d = line["config"]["nodes_rank0"], bench.HP["D"]
    for name in names & {"z", "x", "reconstruction"}:
        assert a[name].dtype == np.float32 and a[name].shape == (n, d) and np.isfinite(a[name]).all(), name
    if "sums" in names:
        s = a["sums"]
        assert s.dtype == np.float64 and s.shape == (3,) and s[2] == n
        assert log_prob_from_sums(s.tolist(), d)["log_prob_xs_per_node"] == line["log_prob_xs_per_node"]
        assert abs(float((a["z"].astype(np.float64) ** 2).sum()) - s[1]) <= 1e-5 * s[1]
    if "theta" in names:
        full = line["dumped_outputs"]["theta"]["shape"]
        assert line["dumped_outputs"]["grad"]["shape"] == full
        for name in ("theta", "grad"):
            assert a[name].dtype == np.float32 and a[name].size == min(full[0], bench.DUMP_ARRAY_BYTES // 4)
            assert np.isfinite(a[name]).all() and np.abs(a[name]).max() > 0, name
