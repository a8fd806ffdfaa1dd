"""bench.py's two kinds of run on the device: the plain command (`--gpus 1 --steps K --warmup W`) prints the headline line
and nothing it does not need; `--full` prints the same headline over the same timed steps plus the figures that take runs
of their own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "spread", "config",
            "log_prob_xs_per_node", "steps_landed_on_host", "consistency"}
FULL_ONLY = {"latency", "graph_replay", "secondary_D100", "with_csr_rebuild_each_step", "two_streams", "host_fed", "roofline",
             "kernel_a", "cpu_baseline", "speedup_vs_cpu_baseline", "secondary_workloads"}


def _line(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=800, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_plain_run_prints_the_headline_and_full_adds_the_rest():
    plain = _line([])
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain), sorted(plain)
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["steps_landed_on_host"] == 3 and plain["consistency"] == []
    # (the CPU baseline and the secondary workloads are the slow part of --full: left out here, their code runs in the
    # bench's own --full run and in test_multirank_gpu.py's sharded --full line)
    full = _line(["--full", "--no-cpu-baseline", "--no-secondary-workloads", "--latency-steps", "10", "--kernel-timing-steps", "2"])
    assert HEADLINE <= set(full)
    assert FULL_ONLY - {"cpu_baseline", "speedup_vs_cpu_baseline", "secondary_workloads"} <= set(full), sorted(full)
    assert full["roofline"]["kernel_us"] > 0 and full["consistency"] == []
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert full[k] == plain[k], k
    # (config's `csr` entry quotes the CSR build's wall time)
    assert {k: v for k, v in full["config"].items() if k != "csr"} == {k: v for k, v in plain["config"].items() if k != "csr"}
    # same seeded batch and weights through the same (bitwise reproducible) kernels: the same batch log-prob
    assert full["log_prob_xs_per_node"] == plain["log_prob_xs_per_node"]
