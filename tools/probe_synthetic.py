#!/usr/bin/env python3
"""Developer probe: from "want a batch" to "batch and both CSRs ready on the device" for the GRevNet driver's synthetic
datasets, by the host route and by the device route (include/gnf_synthetic.h), in one process.
  host    DATASETS_MAP[name].get_next_batch(B, device) + csr_of twice: one RandomState and one data dict per graph, the
          concatenation, the upload of nodes and index arrays, gnf_build_csr by receiver and by sender
  device  DeviceSyntheticDataset(name, device).get_next_batch(B) + csr_of twice (cache hits): gnf_synthetic_nodes, and for the
          datasets whose graphs vary in size the upload of the B counts and gnf_synthetic_topology
Shapes: moons_100 x 32, mom_6_10_20 x 32, mog_9 x 32.  Then the wall time per training iteration of examples/run_grevnet.py's
default flags (dm_self_attn 8 x 10 / 10 / C 80, relu MLP 256 x 5, batch norm, 12 coupling layers, moons_100 x 32, Adam) with
the batches from either route, on one trainer.
After a warm-up, `repeats` timed regions per route, the routes alternating inside every repeat; a region is `calls` batches
(or iterations) between two readings of the host clock, the second after a device synchronise, so host work counts - it is
what the host route consists of.  Median and min .. max go out as one JSON line per measurement.
    python tools/probe_synthetic.py [--repeats R] [--calls C] [--iters I] > profiles/synthetic_probe.jsonl"""
import json
import os
import random
import sys
import time
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def main():
    import torch
    from gnf_amd import gnn
    from gnf_amd.graphs import csr_of
    from gnf_amd.grevnet_synthetic_data import DATASETS_MAP, DeviceSyntheticDataset
    from gnf_amd.train import GRevNetTrainer
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    repeats, calls, iters = int(arg("--repeats", 9)), int(arg("--calls", 20)), int(arg("--iters", 10))
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    batch, seed = 32, 12345
    random.seed(seed)
    np.random.seed(seed)
    gnn.set_random_seed(seed)

    def timed(fns, count, warm):
        out = {k: [] for k in fns}
        for fn in fns.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(count):
                    fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e3 / count)
        med = lambda v: sorted(v)[len(v) // 2]
        return {k + "_ms": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in out.items()}

    def ready(get):
        g = get()
        return g, csr_of(g), csr_of(g, by_sender=True)

    for name in ("moons_100", "mom_6_10_20", "mog_9"):
        host, device = DATASETS_MAP[name], DeviceSyntheticDataset(name, dev, seed)
        g, csr, csr_t = ready(lambda: device.get_next_batch(batch))
        row = {"measurement": "ready_batch", "dataset": name, "graphs": batch, "nodes": int(g.nodes.shape[0]),
               "edges": int(g.senders.shape[0]), "repeats": repeats, "calls_per_region": calls}
        row.update(timed({"ready_host": lambda: ready(lambda: host.get_next_batch(batch, dev)),
                          "ready_device": lambda: ready(lambda: device.get_next_batch(batch))}, calls, 3))
        row["host_over_device"] = round(row["ready_host_ms"]["median"] / row["ready_device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)

    # examples/run_grevnet.py with its default flags
    mlp = partial(gnn.make_mlp_model, 256, 1.0, 5, gnn.relu, 0.1, 0.1)
    make_gnn_fn = partial(gnn.dm_self_attn_gnn, kq_dim=10, v_dim=10, make_mlp_fn=mlp, num_heads=8, concat_heads_output_dim=80,
                          concat=True, residual=False, layer_norm=False)
    trainer = GRevNetTrainer(gnn.GRevNet(make_gnn_fn, 12, 2, use_batch_norm=True), lr=1e-4, adam_beta1=0.9, adam_beta2=0.9)
    host, device = DATASETS_MAP["moons_100"], DeviceSyntheticDataset("moons_100", dev, seed)
    row = {"measurement": "train_iteration", "driver": "examples/run_grevnet.py, default flags", "dataset": "moons_100",
           "graphs": batch, "repeats": repeats, "iterations_per_region": iters}
    row.update(timed({"iteration_host_batches": lambda: trainer.step(host.get_next_batch(batch, dev)),
                      "iteration_device_batches": lambda: trainer.step(device.get_next_batch(batch))}, iters, 3))
    row["host_minus_device_ms"] = round(row["iteration_host_batches_ms"]["median"] - row["iteration_device_batches_ms"]["median"], 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
