#!/usr/bin/env python3
"""Developer probe: the sampled triplet loss, the device route against the dense route a user has without it.
  device  triplet_loss.triplet_loss (gnf_triplet_loss_f32): sampling, scores, loss and (second timing) dL/dnodes from the
          embeddings and the true batch's sender-grouped CSR, O(N * L) memory; nothing reaches the host
  dense   a torch restatement of loss.py:242-270 on the device - dense [N, N] true_adj (index_put with accumulate: the
          einsum's multiplicities), inv_true_adj and l2 `distances` in the reference's matmul form with a zeroed diagonal, L rounds
          of torch.multinomial on the two row-normalised matrices, gather, margin_loss, sum - with autograd for the gradient.
          Rows without a candidate are given a uniform row and masked out of the sum (multinomial refuses an all-zero row: the
          reference's Categorical is undefined there); the block mask is built once outside the timed region (the dense side
          is flattered).  Its samples are torch's, not the header's: the two routes are compared on the loss per kept term, not
          on bits.
on
  config2      the config-2 batch: 64 community_medium graphs drawn as the trainer draws them, D = 64
  driver       the data driver's sampling batch at its default flags, as tools/probe_adj_loss.py draws it: 8 graphs of
               8 .. 19 nodes, D = 200, symmetric G(n, 0.3) graphs with a self loop per node
with run_gnn.py's defaults: triplet_dist_fn l2, margin_loss(0.65), num_sampling_loops 8.  Embeddings: N(0, 1) * sqrt(0.5 / D).
Both routes run on one machine, after a warm-up, as repeated timed regions (20 calls each) that end in a device synchronise;
the routes are alternated inside every repeat and median, min and max over the repeats go out as one JSON line per workload,
with dense_over_device for the call without and with the gradient.
    python tools/probe_triplet_loss.py [--repeats R]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_adj_loss import timed   # noqa: E402

LOOPS, MARGIN = 8, 0.65


def main():
    import numpy as np
    import torch
    from gnf_amd import _abi
    from gnf_amd.datasets import GraphDataset
    from gnf_amd.graphs import data_dicts_to_graphs_tuple
    from gnf_amd.triplet_loss import triplet_loss
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats = arg("--repeats", 7)
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    cm = GraphDataset("graph_rnn_community_medium", 8)
    gen = torch.Generator(device="cpu").manual_seed(0)

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
        n = int(true.nodes.shape[0])
        emb = true.replace(nodes=(torch.randn(n, d, generator=gen) * (0.5 / d) ** 0.5).to(dev))
        sizes = true.n_node.cpu().tolist()
        gid = torch.repeat_interleave(torch.arange(len(sizes), device=dev), true.n_node.to(torch.int64))
        eye = torch.eye(n, device=dev)
        block = (gid[:, None] == gid[None, :]).to(torch.float32)
        snd, rcv = true.senders.to(torch.int64), true.receivers.to(torch.int64)
        one = torch.ones(snd.shape[0], device=dev)
        rows = torch.arange(n, device=dev)

        def dense(grad):
            z = emb.nodes.detach().clone().requires_grad_(grad)
            true_adj = torch.zeros(n, n, device=dev).index_put_((snd, rcv), one, accumulate=True)
            inv = block * ((1.0 - eye) * (1.0 - true_adj)).clamp_min(0.0)
            r = (z * z).sum(1, keepdim=True)
            dist = (1.0 - eye) * (r - 2.0 * z @ z.T + r.T)
            ok = (true_adj.sum(1) > 0) & (inv.sum(1) > 0)
            pa, pn = torch.where(ok[:, None], true_adj, block), torch.where(ok[:, None], inv, block)
            jp = torch.multinomial(pa, LOOPS, replacement=True)      # [N, L]: normalises the rows itself
            jn = torch.multinomial(pn, LOOPS, replacement=True)
            terms = (MARGIN - dist[rows[:, None], jp] + dist[rows[:, None], jn]).clamp_min(0.0) * ok[:, None]
            loss = terms.sum()
            if grad:
                loss.backward()
            return loss, ok.sum() * LOOPS, z.grad

        out = triplet_loss(emb, true, num_sampling_loops=LOOPS, grad="sum", n_node_host=sizes)
        loss, kept, grad = dense(True)
        kept_dev = n * LOOPS - int(out["skipped_terms"].sum())
        row = {"workload": name, "graphs": len(sizes), "nodes": n, "D": d, "edge_entries": int(snd.shape[0]),
               "largest_graph": max(sizes), "loops": LOOPS, "repeats": repeats, "kept_terms": kept_dev,
               "workspace_bytes": int(_abi.lib().gnf_triplet_loss_workspace_bytes(len(sizes), n, LOOPS)),
               "dense_matrix_bytes": 3 * 4 * n * n,
               "mean_loss_device": float(out["mean_loss"]), "mean_loss_dense": float(loss.detach()) / max(int(kept), 1),
               "grad_max_abs_device": float(out["grad_nodes"].abs().max()), "grad_max_abs_dense": float(grad.abs().max())}
        assert int(kept) == kept_dev, row                            # the same nodes have candidates
        assert abs(row["mean_loss_device"] - row["mean_loss_dense"]) <= 0.25 * row["mean_loss_device"], row   # other samples
        kw = dict(num_sampling_loops=LOOPS, n_node_host=sizes)
        row.update(timed({"device": (lambda: triplet_loss(emb, true, **kw), 20),
                          "device_grad": (lambda: triplet_loss(emb, true, grad="sum", **kw), 20),
                          "dense": (lambda: dense(False), 20), "dense_grad": (lambda: dense(True), 20)}, repeats, sync))
        row["dense_over_device"] = round(row["dense_ms"]["median"] / row["device_ms"]["median"], 2)
        row["dense_over_device_grad"] = round(row["dense_grad_ms"]["median"] / row["device_grad_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
