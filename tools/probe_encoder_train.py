#!/usr/bin/env python3
"""Developer probe: the encoder's training step (include/gnf_timestep_gnn_train.h, train.EncoderTrainer) on the device.
  fwd_plain     gnn.TimestepGNN(graph, is_training=True)   (gnf_timestep_gnn_f32)
  fwd_train     TimestepGNN.forward_train(graph): the same launches writing into the stash - fwd_train - fwd_plain is the stash's cost
  bwd           TimestepGNN.backward alone;  bwd_nonorm: the same nets without batch norm - bwd - bwd_nonorm is the norm stage's share
  step          EncoderTrainer.step, eager;  step_replay: loss_and_grads as a captured graph replayed + the Adam launch
  torch_step    the encoder restated in torch operations on the device (index_add aggregation, matmuls, batch moments), autograd,
                the library's binary_loss gradient fed to .backward(), torch.optim.Adam - what a user had without the backward pass
on
  config2   64 community_medium graphs at D = 64: avg_then_mlp (epsilon 2.0), latent 256, K = 5, T = 10, batch norm
  run_gnn   run_gnn.py's default shape on message-passing nets: D = 100, latent 2048 x 3, T = 10, batch norm, weight sharing, 8 small
            graphs - unpacked generic GEMMs, the baseline a packed route would have to beat (step only)
One process, after a warm-up, as alternated timed regions of 20 calls that end in a device synchronise; median, min and max over
the repeats go out as one JSON line per workload.  Before anything is timed the two routes' gradients are compared.
    python tools/probe_encoder_train.py [--repeats R]
    python tools/probe_encoder_train.py --overfit      (see overfit())"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, repeats, sync):
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


def torch_route(enc, graph, hp, trainer_kw, dtype=None):
    """(step callable, gradient callable) of the torch restatement on the encoder's current parameters (dtype: float32, or
    float64 for the yardstick both fp32 routes are held against before anything is timed)"""
    import torch
    from gnf_amd import adj_loss
    dtype = dtype or torch.float32
    p = enc.get_params()
    dev = graph.nodes.device
    leaf = lambda a: torch.tensor(a, device=dev, dtype=dtype, requires_grad=True)
    nets = [[(leaf(w), leaf(b)) for (w, b) in net] for net in p["nets"]]
    bns = [{"gamma": leaf(d["gamma"]), "beta": leaf(d["beta"])} for d in p.get("bn", [])]
    s, r = graph.senders.long(), graph.receivers.long()
    n = graph.nodes.shape[0]
    cnt = torch.zeros(n, device=dev, dtype=dtype).index_add_(0, r, torch.ones(r.shape[0], device=dev, dtype=dtype)).clamp(min=1.0).unsqueeze(1)
    alpha = 0.2
    variables = [t for net in nets for wb in net for t in wb] + [t for d in bns for t in d.values()]
    opt = torch.optim.Adam(variables, lr=trainer_kw["lr"], betas=(0.9, 0.999), eps=1e-8)

    def forward(x):
        nodes = x
        for i in range(hp["num_timesteps"]):
            if bns:
                mean = nodes.mean(0)
                var = ((nodes - mean) ** 2).mean(0)
                inv = torch.rsqrt(var + 1e-3) * bns[i]["gamma"]
                nodes = nodes * inv + (bns[i]["beta"] - mean * inv)
            agg = torch.zeros_like(nodes).index_add_(0, r, nodes.index_select(0, s)) / cnt
            h = hp["epsilon"] * nodes + agg
            net = nets[0 if hp.get("weight_sharing") else i]
            for j, (w, b) in enumerate(net):
                h = h @ w + b
                if j < len(net) - 1:
                    h = torch.maximum(h, alpha * h)
            nodes = h
        return nodes + x if hp.get("residual", True) else nodes

    def grads():
        opt.zero_grad(set_to_none=True)
        out = forward(graph.nodes.to(dtype))
        res = adj_loss.binary_loss(graph.replace(nodes=out.detach().float()), graph, grad="sum", max_nodes_per_graph=trainer_kw["cap"])
        out.backward(res["grad_nodes"].to(dtype))
        return variables

    def step():
        grads()
        opt.step()
    return step, grads


def overfit():
    """--overfit: does a step train?  300 steps on ONE fixed batch of 8 community_small graphs (D = 16, latent 64, K = 3, T = 3,
    batch norm, weight sharing, the net's last layer scaled by 0.1, constant lr 3e-3), once with features of scale 0.3 and once
    of scale 1.0 (where nearly every pair starts inside Keras' clip and gets no gradient): sum_loss, the largest gradient entry
    and the incorrect edges every 50 steps, one JSON line per scale"""
    import torch
    from gnf_amd import datasets, encoder, gnn
    from gnf_amd.train import EncoderTrainer
    dev = torch.device("cuda:0")
    hp = dict(node_dim=16, latent=64, K=3, activation="leaky_relu", agg="mean", combine="agg", epsilon=2.0, num_timesteps=3,
              use_batch_norm=True, weight_sharing=True, residual=True)
    for scale in (0.3, 1.0):
        gnn.set_random_seed(0)
        graph = datasets.GraphDataset("graph_rnn_community_small", 16, gaussian_scale=scale).get_next_train_batch(8, dev)
        enc = encoder.make_encoder(hp)
        enc._desc(16, dev, True)
        for b in enc.blocks():
            w, bias = b._mlp.params[-1]
            b._mlp.params[-1] = (w * 0.1, bias * 0.1)
        tr = EncoderTrainer(enc, lr=3e-3, lr_type="constant")
        rows = []
        for it in range(301):
            r = tr.step(graph)
            if it % 50 == 0:
                wrong = float(r["false_positive_pairs"].sum() + r["false_negative_pairs"].sum()) / 2
                rows.append({"step": it, "sum_loss": round(float(r["sum_loss"]), 3), "grad_max": round(float(tr.grad.abs().max()), 4),
                             "incorrect_edges": wrong})
        print(json.dumps({"workload": "overfit", "gaussian_scale": scale, "nodes": int(graph.nodes.shape[0]), "trace": rows}), flush=True)


def main():
    import numpy as np
    import torch
    from gnf_amd import datasets, encoder, gnn
    from gnf_amd.train import EncoderTrainer
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 7)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    gnn.set_random_seed(0)
    workloads = {
        "config2": (datasets.GraphDataset("graph_rnn_community_medium", 64).get_next_train_batch(64, dev),
                    dict(node_dim=64, latent=256, K=5, activation="leaky_relu", agg="mean", combine="agg", epsilon=2.0,
                         num_timesteps=10, use_batch_norm=True, residual=False), True),
        "run_gnn": (datasets.GraphDataset("graph_rnn_community_small", 100).get_next_train_batch(8, dev),
                    dict(node_dim=100, latent=2048, K=3, activation="leaky_relu", agg="mean", combine="agg", epsilon=2.0,
                         num_timesteps=10, use_batch_norm=True, weight_sharing=True, residual=True, bias_init_stddev=0.3), False),
    }
    for name, (graph, hp, full) in workloads.items():
        n, d = graph.nodes.shape
        cap = int(graph.n_node.max())
        enc = encoder.make_encoder(hp)
        tr = EncoderTrainer(enc, lr=1e-4, max_nodes_per_graph=cap)
        tr.loss_and_grads(graph)                                  # variables, arena, CSRs
        sync()
        line = {"workload": name, "nodes": int(n), "edges": int(graph.senders.shape[0]), "D": int(d), "latent": hp["latent"],
                "K": hp["K"], "T": hp["num_timesteps"], "parameters": int(tr.theta.numel())}
        fns = {}
        if full:
            t_step, t_grads = torch_route(enc, graph, hp, dict(lr=1e-4, cap=cap))
            # both fp32 routes against the restatement in float64: max |difference| over the whole gradient / max |gradient|
            flat = lambda tv: torch.cat([v.grad.reshape(-1) for v in tv]).double()
            ref = flat(torch_route(enc, graph, hp, dict(lr=1e-4, cap=cap), torch.float64)[1]())
            dev_rel = float((tr.grad.double() - ref).abs().max() / ref.abs().max())
            torch_rel = float((flat(t_grads()) - ref).abs().max() / ref.abs().max())
            line["device_vs_float64_grad_max_rel"], line["torch_fp32_vs_float64_grad_max_rel"] = dev_rel, torch_rel
            assert dev_rel <= max(4.0 * torch_rel, 1e-3), (dev_rel, torch_rel)
            plain = encoder.make_encoder(hp).set_params(enc.get_params())
            nonorm = encoder.make_encoder(dict(hp, use_batch_norm=False)).set_params({"nets": enc.get_params()["nets"]})
            g_out = torch.randn(n, d, device=dev)
            _, stash = enc.forward_train(graph)
            grads = enc.make_grads(d, dev)
            _, stash_nn = nonorm.forward_train(graph)
            grads_nn = nonorm.make_grads(d, dev)
            fns.update(fwd_plain=(lambda: plain(graph, True), 20), fwd_train=(lambda: enc.forward_train(graph), 20),
                       bwd=(lambda: enc.backward(graph, stash, g_out, grads), 20),
                       bwd_nonorm=(lambda: nonorm.backward(graph, stash_nn, g_out, grads_nn), 20),
                       torch_step=(t_step, 20))
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                tr.loss_and_grads(graph)

            def replay():
                cg.replay()
                tr.apply_gradients()
            fns["step_replay"] = (replay, 20)
        fns["step"] = (lambda: tr.step(graph), 20)
        line.update(timed(fns, repeats, sync))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    overfit() if "--overfit" in sys.argv else main()
