#!/usr/bin/env python3
"""Developer probe: the encoder's forward pass, one library call against the route a user has without it.
  device  gnn.TimestepGNN(graph, is_training=True) (gnf_timestep_gnn_f32): T module calls, their batch norms (moments, normalise,
          moving-average update) and the residual in one call
  torch   T separate block(graph) calls (gnf_gnn_apply_f32) with snt.BatchNorm's arithmetic, its moving-average update and the
          residual as torch operations between them - the same nets and variables
  nonorm  the device route with use_batch_norm=False on the same nets: device - nonorm is what the norm stage costs
on
  config2   the config-2 batch (64 community_medium graphs drawn as the trainer draws them) at D = 64: avg_then_mlp
            (epsilon 2.0, run_gnn.py:106-108), latent 256, K = 5, T = 10, batch norm
  run_gnn   run_gnn.py's default flags on a batch of 8 complete graphs (8 .. 19 nodes, self loops): D = 100, dm_attn with 2 heads
            of 64 / 64 (C = 64, kq_dim_division), latent 2048 x 3, T = 10, batch norm, weight sharing
All routes run on one machine, after a warm-up, as repeated timed regions (20 calls each) that end in a device synchronise;
the routes are alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload
with torch_over_device and norm_fraction.  Before anything is timed the two routes' outputs are compared.
    python tools/probe_timestep_gnn.py [--repeats R]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, repeats, sync):
    """fns: name -> (callable, calls per timed region); milliseconds per call"""
    out = {k: [] for k in fns}
    for k, (fn, _) in fns.items():
        fn()                       # warm-up
    sync()
    for _ in range(repeats):
        for k, (fn, calls) in fns.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            out[k].append((time.perf_counter() - t0) * 1e3 / calls)
    med = lambda v: sorted(v)[len(v) // 2]
    return {k + "_ms": {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in out.items()}


def main():
    import numpy as np
    import torch
    from gnf_amd import datasets, encoder, gnn
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 7)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    gnn.set_random_seed(0)
    rng = np.random.default_rng(0)
    sizes = rng.integers(8, 20, size=8)
    complete = datasets.transform_example(rng.standard_normal((int(sizes.sum()), 100)).astype(np.float32), sizes, dev)
    workloads = {
        "config2": (datasets.GraphDataset("graph_rnn_community_medium", 64).get_next_train_batch(64, dev),
                    dict(node_dim=64, latent=256, K=5, activation="leaky_relu", agg="mean", combine="agg", epsilon=2.0,
                         num_timesteps=10, use_batch_norm=True, residual=False)),
        "run_gnn": (complete,
                    dict(node_dim=100, latent=2048, K=3, activation="relu", agg="sum", combine="agg", epsilon=0.0,
                         attn=dict(num_heads=2, kq_dim=64, v_dim=64, out_dim=64, concat=True, residual=False,
                                   kq_dim_division=True), num_timesteps=10, weight_sharing=True, use_batch_norm=True,
                         residual=False)),
    }
    for name, (graph, hp) in workloads.items():
        enc = encoder.make_encoder(hp)
        plain = encoder.make_encoder(dict(hp, use_batch_norm=False))
        t = enc.num_timesteps
        ref = enc(graph, True).nodes.clone()                      # (creates the variables)
        plain(graph, True)
        plain.set_params({"nets": enc.get_params()["nets"]})
        for b in enc.bns:                                         # trained-looking variables, the same for both routes
            b.gamma.uniform_(0.5, 1.5), b.beta.normal_(0.0, 0.2)
        mm = [b.moving_mean.clone() for b in enc.bns]
        mv = [b.moving_variance.clone() for b in enc.bns]
        eps, omd = enc.bn_eps, 1.0 - enc.bn_decay_rate

        def torch_route():
            g = graph
            for i in range(t):
                h, b = g.nodes, enc.bns[i]
                mean = h.mean(0)
                var = h.var(0, unbiased=False)
                inv = torch.rsqrt(var + eps) * b.gamma
                h = h * inv + (b.beta - mean * inv)
                mm[i].sub_((mm[i] - mean) * omd)
                mv[i].sub_((mv[i] - var) * omd)
                g = enc.gnns[0 if enc.weight_sharing else i](g.replace(nodes=h))
            return g.nodes + graph.nodes if enc.residual else g.nodes

        ref = enc(graph, True).nodes.clone()
        alt = torch_route()
        sync()
        scale = float(ref.abs().max())
        row = {"workload": name, "graphs": int(graph.n_node.shape[0]), "nodes": int(graph.nodes.shape[0]),
               "edge_entries": int(graph.senders.shape[0]), "D": hp["node_dim"], "latent": hp["latent"], "K": hp["K"], "T": t,
               "weight_sharing": bool(enc.weight_sharing), "repeats": repeats, "out_max_abs": scale,
               "max_abs_diff_vs_torch_route": float((ref - alt).abs().max())}
        assert np.isfinite(scale) and row["max_abs_diff_vs_torch_route"] <= 1e-3 * max(1.0, scale), row
        row.update(timed({"device": (lambda: enc(graph, True), 20), "torch": (torch_route, 20),
                          "nonorm": (lambda: plain(graph, True), 20)}, repeats, sync))
        row["torch_over_device"] = round(row["torch_ms"]["median"] / row["device_ms"]["median"], 2)
        row["norm_fraction"] = round(1.0 - row["nonorm_ms"]["median"] / row["device_ms"]["median"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
