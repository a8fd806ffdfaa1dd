#!/usr/bin/env python
"""In-process A/B of two gnf_set_option settings on a bench workload's forward step (developer tool, run on the GPU box):

    python tools/ab_options.py --a force_shape=12 --b force_shape=0 [--workload config2] [--rounds 15] [--steps 50]

One process, one batch, one set of weights; the arms alternate round by round (A B A B ...), each round is `--steps` steps of
bench.py's single-GPU step (forward + log-prob sums into pinned host memory) between two synchronisations.  Printed per arm:
the median over rounds of ms_per_step, the round-to-round spread (max - min over rounds, first round of each arm dropped as
warm-up), and the log-prob of the last step; then B against A.  Separate bench.py runs land 2 % apart between boxes
(CHANGELOG 4.4); the interleaved arms of one process resolve 0.1 %."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def parse_opts(text):
    out = {}
    for item in filter(None, text.split(",")):
        name, _, val = item.partition("=")
        out[name.strip()] = int(val or 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="arm A: name=value[,name=value]")
    ap.add_argument("--b", required=True, help="arm B")
    ap.add_argument("--workload", default="config2", choices=[w for w, d in bench.WORKLOADS.items() if not d.get("train") and not d["inverse"]])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    arms = {"A": parse_opts(args.a), "B": parse_opts(args.b)}

    bench.WORKLOAD = bench.WORKLOADS[args.workload]
    bench.GRAPHS_PER_GPU = bench.WORKLOAD["graphs"]
    bench.HP.update(bench.WORKLOAD["hp"])
    from gnf_amd import _abi
    from gnf_amd.factories import make_product_grevnet
    from gnf_amd.flow import forward_shard_sums, log_prob_from_sums
    from gnf_amd.graphs import build_csr_device, data_dicts_to_graphs_tuple
    _abi.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dicts, n_global, _ = bench.make_batch(1, 0)
    graph = data_dicts_to_graphs_tuple(dicts, dev)
    net = make_product_grevnet(bench.HP, bench.make_params(bench.WEIGHT_SEED, bench.HP, bench.FINAL_SCALE))
    net.fused = True
    build_csr_device(graph)
    host = torch.zeros(2, 3, dtype=torch.float64).pin_memory()
    host[:, 2] = float(graph.nodes.shape[0])

    def use(opts):
        for name in set(arms["A"]) | set(arms["B"]):
            _abi.set_option(name, opts.get(name, 0))

    def region(row):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            forward_shard_sums(net, graph, host[row])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    times = {"A": [], "B": []}
    for r in range(args.rounds + 1):           # round 0 of each arm: warm-up (kernel load, allocator), dropped
        for row, arm in enumerate("AB"):
            use(arms[arm])
            ms = region(row)
            if r:
                times[arm].append(ms)
    use({})
    out = {"workload": args.workload, "rounds": args.rounds, "steps_each": args.steps, "nodes": n_global}
    for row, arm in enumerate("AB"):
        t = times[arm]
        out[arm] = {"options": arms[arm], "ms_per_step_median": round(statistics.median(t), 5), "ms_per_step_min": round(min(t), 5),
                    "ms_per_step_max": round(max(t), 5), "spread": round(max(t) - min(t), 5),
                    "log_prob_xs_per_node": log_prob_from_sums(host[row].tolist(), bench.HP["D"])["log_prob_xs_per_node"],
                    "rounds_ms": [round(v, 5) for v in t]}
    gain = out["A"]["ms_per_step_median"] - out["B"]["ms_per_step_median"]
    sp = max(out["A"]["spread"], out["B"]["spread"])
    out["A_minus_B_ms"] = round(gain, 5)
    out["larger_spread_ms"] = sp
    out["B_below_A_by_more_than_3_spreads"] = bool(gain > 3 * sp)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
