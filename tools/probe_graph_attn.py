#!/usr/bin/env python3
"""Developer probe: kernel time of the whole-graph attention family against the edge family on the same batch.
run_grevnet.py's defaults - 32 complete 100-node graphs (self loops), D = 2, T = 12, 8 heads of kq = v = 10, C = 80,
relu MLPs 256 x 5 - timed with HIP events: one forward (gnf_grevnet_from_f32) and one trainer step (loss_and_grads +
Adam), for --make_gnn_fn multihead_self_attn and dm_self_attn.  Prints one JSON line per family.
    python tools/probe_graph_attn.py [multihead_self_attn|dm_self_attn|both] [--iters K]
Kernel-level numbers: run it under `rocprofv3 --kernel-trace --stats -- python tools/probe_graph_attn.py <family>`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import graph_attn_ref as R
from gnf_amd.flow import forward_shard_sums
from gnf_amd.graphs import GraphsTuple
from gnf_amd.factories import make_product_grevnet
from gnf_amd.train import GRevNetTrainer
from oracle import gnf_oracle as O

HEADS = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80)


def batch(dev, graphs=32, nodes=100, d=2, seed=0):
    nn = np.full(graphs, nodes, np.int64)
    s, r = R.complete_edges(nn)
    x = np.random.default_rng(seed).standard_normal((graphs * nodes, d)).astype(np.float32)
    t = lambda a, dt: torch.as_tensor(np.asarray(a, dt)).to(dev)
    return GraphsTuple(nodes=t(x, np.float32), edges=None, receivers=t(r, np.int32), senders=t(s, np.int32), globals=None,
                       n_node=t(nn, np.int32), n_edge=t(nn * nn, np.int32))


def build(family, d=2, latent=256, k=5, t=12):
    if family == "multihead_self_attn":
        attn = dict(HEADS, scope="graph", kq_dim_division=True)
        p = R.make_graph_attn_grevnet_params(1, d // 2, latent, k, t, final_scale=0.25, **HEADS)
    else:
        attn = dict(HEADS, concat=True, kq_dim_division=False, residual=False)
        p = O.make_attn_grevnet_params(1, d // 2, latent, k, t, final_scale=0.25, **HEADS)
    hp = dict(D=d, latent=latent, K=k, T=t, agg="sum", combine="agg", epsilon=0.0, activation="relu",
              weight_sharing=False, attn=attn)
    return make_product_grevnet(hp, p)


def events_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def probe(family, iters, dev):
    graph = batch(dev)
    net = build(family)
    tr = GRevNetTrainer(net, lr=1e-5, use_lr_decay=False)
    for _ in range(3):   # warm-up: caches, workspaces, first launches
        forward_shard_sums(net, graph)
        tr.step(graph)
    torch.cuda.synchronize()
    fwd = events_ms(lambda: forward_shard_sums(net, graph), iters)
    step = events_ms(lambda: tr.step(graph), iters)
    return {"family": family, "graphs": 32, "nodes_per_graph": 100, "D": 2, "T": 12, "forward_ms": round(fwd, 4),
            "train_step_ms": round(step, 4), "iters": iters}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    which = args[0] if args and args[0] != str(iters) else "both"
    fams = ["multihead_self_attn", "dm_self_attn"] if which == "both" else [which]
    dev = torch.device("cuda:0")
    for f in fams:
        print(json.dumps(probe(f, iters, dev)), flush=True)


if __name__ == "__main__":
    main()
