#!/usr/bin/env python3
"""Developer probe: the adjacency reconstruction loss, the device route against the dense route a user has without it.
  device  adj_loss.binary_loss (gnf_adj_loss_dist_f32, as every token): loss, per-graph loss, pair counts and (second timing)
          dL/dnodes from the embeddings and the true batch's CSR; nothing reaches the host
  dense   flow.pred_adj for the per-graph probability blocks, put on one [N, N] matrix (torch.block_diag) and compared with the
          dense true adjacency in ONE masked comparison per count, summed per graph with index_add; and a torch restatement
          of loss.py's binary_loss on the device - dense [N, N] true adjacency, dense logits in the reference's matmul
          form, clip, softplus, masked sum - with autograd for the gradient.  The block-diagonal mask and the graph id of
          every row are built once outside the timed region (the reference rebuilds its mask per call: the dense side is
          flattered)
on
  config2      the config-2 batch: 64 community_medium graphs drawn as the trainer draws them, D = 64
  driver       the data driver's sampling batch at its default flags, as tools/probe_decode_graphs.py draws it: 8 graphs of
               8 .. 19 nodes, D = 200, against symmetric G(n, 0.3) graphs with a self loop per node - both routes are
               launch-bound here
Embeddings: N(0, 1) * 0.5 * D^-1/4 with one row in eight stretched by 4 (the tests' distribution: every branch sees pairs).
Beside the device route, the same call with adj_loss.TunedSigmoidL2(10, 1) (temp and shift read from device memory) without
a gradient, with dL/dnodes, and with dL/dnodes and dL/d(temp, shift) - its outputs are asserted bit-equal to the device
route's first.  Since the two library paths were merged the `device` and `dist` columns time the same kernels through the same
entry point: they differ by the run-time parameter load, and `dist_grad_params` adds the stores and sums of the two extra fp64
row sums.  The columns are kept so that figures stay comparable with earlier records.
Both routes run on one machine, after a warm-up, as repeated timed regions (20 calls each) that end in a device synchronise;
the routes are alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload,
with dense_over_device for the call without and with the gradient.  Before anything is timed the two routes are compared
(the dense logits come out of a matmul, so they are compared, not asserted equal).
    python tools/probe_adj_loss.py [--repeats R]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = math.log((1.0 - 1e-7) / 1e-7)


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
    import torch
    from gnf_amd.adj_loss import TunedSigmoidL2, binary_loss
    import numpy as np
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.flow import pred_adj
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 7)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    cm = GraphDataset("graph_rnn_community_medium", 8)
    gen = torch.Generator(device="cpu").manual_seed(0)

    def embed(g, d):
        n = int(g.nodes.shape[0])
        z = torch.randn(n, d, generator=gen) * 0.5 * d ** -0.25
        z[torch.rand(n, generator=gen) < 0.125] *= 4.0
        return g.replace(nodes=z.to(dev))

    def driver_batch():
        rng = np.random.default_rng(0)
        dicts = []
        for n in rng.integers(8, 20, size=8):
            m = np.triu(rng.random((n, n)) < 0.3, 1)
            s, r = np.nonzero(m | m.T | np.eye(n, dtype=bool))
            dicts.append({"nodes": np.zeros((n, 1), np.float32), "senders": s, "receivers": r})
        return data_dicts_to_graphs_tuple(dicts, dev)

    workloads = {"config2": (cm.get_next_train_batch(64, dev), 64), "driver": (driver_batch(), 200)}
    for name, (true, d) in workloads.items():
        emb = embed(true, d)
        sizes = true.n_node.cpu().tolist()
        n = sum(sizes)
        gid = torch.repeat_interleave(torch.arange(len(sizes), device=dev), true.n_node.to(torch.int64))
        mask = ((gid[:, None] == gid[None, :]) & ~torch.eye(n, dtype=torch.bool, device=dev)).to(torch.float32)
        snd, rcv = true.senders.to(torch.int64), true.receivers.to(torch.int64)

        def dense(grad):
            z = emb.nodes.detach().clone().requires_grad_(grad)
            true_adj = torch.zeros(n, n, device=dev)
            true_adj[snd, rcv] = 1.0
            r = (z * z).sum(1, keepdim=True)
            dist = (r - 2.0 * z @ z.T + r.T) / math.sqrt(d)
            uc = (10.0 * (1.0 - dist)).clamp(-U, U)
            loss = ((torch.nn.functional.softplus(uc) - true_adj * uc) * mask).sum()
            if grad:
                loss.backward()
            p = torch.block_diag(*pred_adj(emb))             # (zero diagonal, zero outside the blocks)
            a = true_adj * mask
            zero = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
            fp = zero.index_add(0, gid, (p - a > 0.5).sum(1))
            fn = zero.index_add(0, gid, (a - p > 0.5).sum(1))
            return loss, fp, fn, z.grad

        out = binary_loss(emb, true, grad="sum", n_node_host=sizes)
        loss, fp, fn, grad = dense(True)
        gmax = float(grad.abs().max())
        row = {"workload": name, "graphs": len(sizes), "nodes": n, "D": d, "edge_entries": int(snd.shape[0]),
               "largest_graph": max(sizes), "ordered_pairs": sum(s * s - s for s in sizes), "repeats": repeats,
               "sum_loss_device": float(out["sum_loss"]), "sum_loss_dense_fp32": float(loss.detach()),
               "fp_pairs": int(out["false_positive_pairs"].sum()), "fn_pairs": int(out["false_negative_pairs"].sum()),
               "count_mismatches_vs_pred_adj": int((out["false_positive_pairs"] != fp).sum() +
                                                   (out["false_negative_pairs"] != fn).sum()),
               "grad_max_abs": gmax, "grad_max_abs_diff_vs_autograd": float((out["grad_nodes"] - grad).abs().max())}
        assert row["count_mismatches_vs_pred_adj"] == 0, row     # the same arithmetic as pred_adj: equal
        assert abs(row["sum_loss_device"] - row["sum_loss_dense_fp32"]) <= 1e-3 * abs(row["sum_loss_device"]), row
        assert row["grad_max_abs_diff_vs_autograd"] <= 1e-2 * gmax, row
        tuned = TunedSigmoidL2(10.0, 1.0)
        via_dist = binary_loss(emb, true, tuned, grad="sum", grad_params=True, n_node_host=sizes)
        for k in ("sum_loss", "loss_per_graph", "false_positive_pairs", "false_negative_pairs", "grad_nodes"):
            assert torch.equal(via_dist[k], out[k]), k           # the same arithmetic: equal
        row["grad_params"] = [float(v) for v in via_dist["grad_params"].cpu()]
        row.update(timed({"device": (lambda: binary_loss(emb, true, n_node_host=sizes), 20),
                          "device_grad": (lambda: binary_loss(emb, true, grad="sum", n_node_host=sizes), 20),
                          "dist": (lambda: binary_loss(emb, true, tuned, n_node_host=sizes), 20),
                          "dist_grad": (lambda: binary_loss(emb, true, tuned, grad="sum", n_node_host=sizes), 20),
                          "dist_grad_params": (lambda: binary_loss(emb, true, tuned, grad="sum", grad_params=True,
                                                                   n_node_host=sizes), 20),
                          "dense": (lambda: dense(False), 20), "dense_grad": (lambda: dense(True), 20)}, repeats, sync))
        row["dense_over_device"] = round(row["dense_ms"]["median"] / row["device_ms"]["median"], 2)
        row["dense_over_device_grad"] = round(row["dense_grad_ms"]["median"] / row["device_grad_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
