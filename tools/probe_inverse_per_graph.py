#!/usr/bin/env python3
"""Developer probe: what the per-graph likelihood of generated graphs costs.  On the config-2 bench batch (2718 nodes, 64
graphs, message passing, no batch norm) and on the data driver's default flow (dm_attn, one head of 64 / 64, 2048 x 3 nets,
D = 200, 10 coupling layers, batch norm, 32 complete graphs of 8 .. 19 nodes) it times
  g                 GRevNet.g (gnf_grevnet_from_f32, GNF_INVERSE): the sample only
  g_per_graph       GRevNet.g_per_graph (gnf_grevnet_inverse_per_graph_f32): the same pass + every graph's log-det and sum z^2
  g_then_f_per_graph  the route it replaces: g, then f_per_graph on its output - a second full pass
as regions of `iters` calls that each end in a synchronise, the three ALTERNATED inside every repeat (other work shares the
machine: a difference is judged against the spread of the repeats); the median and the min .. max over the repeats are
printed as one JSON line per workload.  For the flow with batch norm it also prints how far the second route's per-graph
log-det is from minus g_per_graph's: f normalises with the moments of the batch it is given, g de-normalises with the moving
statistics, so the two were never the same quantity.  Each workload runs in a child process under a time limit of its own,
and the probe ends at the first one that fails.
    python tools/probe_inverse_per_graph.py [--repeats R] [--iters K] [--workload config2|data_driver]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _config2():
    from test_fullsize_gpu import _bench_batch
    g_cpu, p, hp = _bench_batch()
    return (hp, g_cpu.n_node.numpy(), g_cpu.n_edge.numpy(), g_cpu.senders.numpy(), g_cpu.receivers.numpy(), g_cpu.nodes.numpy(), p)


def _data_driver():
    import numpy as np
    import graph_attn_ref as R
    from oracle import gnf_oracle as O
    rng = np.random.default_rng(12345)
    nn = rng.integers(8, 20, size=32).astype(np.int64)
    s, r = R.complete_edges(nn)
    d, latent, k, t = 200, 2048, 3, 10
    akw = dict(num_heads=1, kq_dim=64, v_dim=64, out_dim=64, concat=True, kq_dim_division=True, residual=False)
    hp = dict(D=d, latent=latent, K=k, T=t, agg="mean", combine="agg", epsilon=0.0, activation="relu", weight_sharing=False,
              attn=akw, use_batch_norm=True)
    p = O.make_attn_grevnet_params(3, d // 2, latent, k, t, weight_sharing=False, final_scale=0.1, **akw)
    p["bn"] = O.make_bn_params(5, d // 2, t)
    z = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    return hp, nn, nn ** 2, s, r, z, p


def child(workload, repeats, iters):
    import numpy as np
    import torch
    from gnf_amd import _abi
    from helpers import graph_from_arrays, make_product_grevnet
    dev = "cuda:0"
    hp, nn, ne, s, r, z, p = _config2() if workload == "config2" else _data_driver()
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, z, dev)

    def both():
        net.f_per_graph(net.g(graph))

    fns = {"g": lambda: net.g(graph), "g_per_graph": lambda: net.g_per_graph(graph), "g_then_f_per_graph": both}
    routes = {}
    for name, fn in fns.items():   # warm-up: caches, workspaces, first launches
        for _ in range(3):
            fn()
        routes[name] = sorted(_abi.last_route())
    torch.cuda.synchronize()
    rows = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            rows[name].append((time.perf_counter() - t0) * 1e3 / iters)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": workload, "nodes": int(np.sum(nn)), "graphs": int(len(nn)), "batch_norm": bool(hp.get("use_batch_norm", False)),
           "repeats": repeats, "iters": iters, "routes": routes}
    for name, v in rows.items():
        out[name + "_ms"] = {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["overhead_over_g"] = round(med([b / a - 1.0 for a, b in zip(rows["g"], rows["g_per_graph"])]), 4)
    out["second_pass_route_over_g_per_graph"] = round(med([c / b for b, c in zip(rows["g_per_graph"], rows["g_then_f_per_graph"])]), 3)
    # the two routes' numbers side by side: -logdet_g against f_per_graph's log-det at x = g(z), per node of each graph
    xg, logdet_g = net.g_per_graph(graph)
    logdet_g = logdet_g.clone()
    _, logdet_f = net.f_per_graph(xg)
    torch.cuda.synchronize()
    diff = ((logdet_f + logdet_g).abs().cpu().numpy() / np.maximum(np.asarray(nn, np.float64), 1.0))
    out["second_pass_logdet_minus_true_per_node"] = {"max": float(diff.max()), "median": float(np.median(diff))}
    out["logdet_g_per_node_range"] = [float((logdet_g.cpu().numpy() / np.maximum(nn, 1)).min()),
                                      float((logdet_g.cpu().numpy() / np.maximum(nn, 1)).max())]
    print(json.dumps(out), flush=True)


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    repeats, iters = int(arg("--repeats", 7)), int(arg("--iters", 200))
    if "--child" in sys.argv:
        return child(arg("--child", "config2"), repeats, iters)
    only = arg("--workload", None)
    for workload in ("config2", "data_driver"):
        if only and workload != only:
            continue
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", workload, "--repeats", str(repeats), "--iters",
                              str(iters)], capture_output=True, text=True, timeout=420)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"probe_inverse_per_graph: workload {workload} failed with status {res.returncode}; stopping")
        print(res.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
