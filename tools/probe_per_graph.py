#!/usr/bin/env python3
"""Developer probe: what per-graph log-likelihoods cost.  On the config-2 bench batch (2718 nodes, 64 graphs) it times
  f            GRevNet.f (gnf_grevnet_from_f32): the batch scalar only
  f_per_graph  GRevNet.f_per_graph (gnf_grevnet_per_graph_f32): the same pass + every graph's terms
  single_calls the only way to per-graph values without it: 64 calls of f, one graph each
with HIP events around whole passes.  The three are ALTERNATED inside every repeat (other work shares the machine: a
difference is judged against the spread of the repeats), the median and the min .. max over the repeats are printed as
one JSON line.  Each measurement round runs in a child process under a time limit of its own, and the probe ends at the
first one that fails.
    python tools/probe_per_graph.py [--repeats R] [--iters K]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(iters):
    import numpy as np
    import torch
    import per_graph_ref as P
    from helpers import graph_from_arrays, make_product_grevnet
    from test_fullsize_gpu import _bench_batch
    dev = "cuda:0"
    g_cpu, p, hp = _bench_batch()
    nn, ne = g_cpu.n_node.numpy(), g_cpu.n_edge.numpy()
    s, r, x = g_cpu.senders.numpy(), g_cpu.receivers.numpy(), g_cpu.nodes.numpy()
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, x, dev)
    singles = [graph_from_arrays(*one, dev) for one in P.single_graph_batches(nn, ne, s, r, x)]

    def single_calls():
        for g in singles:
            net.f(g)

    fns = {"f": lambda: net.f(graph), "f_per_graph": lambda: net.f_per_graph(graph), "single_calls": single_calls}
    for fn in fns.values():   # warm-up: caches, workspaces, first launches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {}
    for name, fn in fns.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k = max(iters // 16, 2) if name == "single_calls" else iters
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) / k
    print(json.dumps(out), flush=True)


def main():
    if "--child" in sys.argv:
        return child(int(sys.argv[sys.argv.index("--child") + 1]))
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 7
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 200
    rows = []
    for _ in range(repeats):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(iters)], capture_output=True, text=True,
                             timeout=240)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"probe_per_graph: a measurement round failed with status {res.returncode}; stopping")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": "config2", "nodes": 2718, "graphs": 64, "repeats": repeats, "iters": iters}
    for name in ("f", "f_per_graph", "single_calls"):
        v = [row[name] for row in rows]
        out[name + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["overhead_over_f"] = round(med([row["f_per_graph"] / row["f"] - 1.0 for row in rows]), 4)
    out["single_calls_over_f_per_graph"] = round(med([row["single_calls"] / row["f_per_graph"] for row in rows]), 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
