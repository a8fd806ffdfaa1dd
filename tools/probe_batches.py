#!/usr/bin/env python3
"""Developer probe: "batch ready for the trainer" - assembled, on the device, both CSRs available - by the parent route and by
the device route (include/gnf_batches.h), on the same graph ids.
  parent  edge lists:  graphs.graphs_tuple_from_edge_lists on the host (GraphDataset.get_next_train_batch's assembly), upload,
                       csr_of(g) and csr_of(g, by_sender=True) - two gnf_build_csr
          complete:    datasets.transform_example on host embeddings (the host chunk reader's), upload, the same two csr_of
  device  edge lists:  DeviceGraphDataset.batch_of(ids) - one gnf_batch_assemble, caches seeded
          complete:    datasets.complete_batch on a device tensor (the device chunk reader's view) - one gnf_complete_batch
Node features are each route's own: the edge-list parent draws them with numpy on the host and uploads them, the device route
draws them with torch.randn on the device; the complete routes get the chunk's embeddings where their reader leaves them.
Shapes
  cm64_d64          64 x community_medium, D = 64, the encoder's trainer (run_gnn.py's defaults at that width)
  run_gnn_default   run_gnn.py's default batch: 8 x community_small, D = 100, the encoder's trainer
  grid32_complete   32 x grid node counts, complete topology, D = 200, the data driver's default flow and trainer
  cm32_complete     32 x community_medium node counts, likewise
Per shape: each route alone, and wall time per iteration of (make the batch, trainer.step on it).  After a warm-up, 7 timed
regions per route, the routes alternated inside every repeat, every region ending in a device synchronise; median and
min .. max go out as one JSON line per shape.  Before anything is timed the two routes' index arrays and CSRs are compared
for equality.
    python tools/probe_batches.py [--repeats R] [--shapes a,b] > profiles/batches_probe.jsonl"""
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np   # noqa: E402

from probe_graph_components import timed   # noqa: E402


def main():
    import torch
    from gnf_amd import datasets as D, encoder as E, gnn
    from gnf_amd.graphs import csr_of, graphs_tuple_from_edge_lists
    from gnf_amd.train import EncoderTrainer, GRevNetTrainer
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    repeats = int(arg("--repeats", 7))
    shapes = arg("--shapes", "cm64_d64,run_gnn_default,grid32_complete,cm32_complete").split(",")
    assert torch.cuda.is_available(), "the probe measures the device route: it needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    gnn.set_random_seed(12345)

    def same(a, b):
        e = int(a.senders.shape[0])
        ok = all(torch.equal(getattr(a, k).to(torch.int32), getattr(b, k).to(torch.int32))
                 for k in ("senders", "receivers", "n_node", "n_edge"))
        for t in (False, True):
            ca, cb = csr_of(a, by_sender=t), csr_of(b, by_sender=t)
            ok = ok and torch.equal(ca.rowptr, cb.rowptr) and torch.equal(ca.col[:e], cb.col[:e])
        return bool(ok)

    def encoder_trainer(dim):
        hp = dict(node_dim=dim, latent=2048, K=3, activation="leaky_relu", bias_init_stddev=0.3, num_timesteps=10,
                  weight_sharing=True, use_batch_norm=True, use_layer_norm=False, residual=True, test_local_stats=True,
                  agg="mean", combine="agg", epsilon=2.0)
        return EncoderTrainer(E.make_encoder(hp), lr=1e-5, num_train_iters=100000)

    def flow_trainer(dim=200):
        mlp = partial(gnn.make_mlp_model, 2048, dim / 2, 3, activation=gnn.relu, l2_regularizer_weight=0.000001, bias_init_stddev=0.3)
        make_gnn = partial(gnn.dm_self_attn_gnn, kq_dim=64, v_dim=64, make_mlp_fn=mlp, num_heads=1, concat_heads_output_dim=64,
                           kq_dim_division=True, layer_norm=False)
        return GRevNetTrainer(gnn.GRevNet(make_gnn, 10, dim, use_batch_norm=True, weight_sharing=False), lr=1e-5, adam_beta2=0.999,
                              use_lr_decay=False, clip_gradient_by_norm=True, clip_gradient_norm=10.0)

    def edge_list_shape(name, count, dim):
        host = D.GraphDataset(name, dim)
        device = D.DeviceGraphDataset(name, dim, device=dev)
        ids = host.sample_ids(count)

        def parent():
            n = int(host.all.n_node[ids].sum())
            x = host.rng.normal(scale=host.scale, size=(n, dim)).astype(np.float32)
            g = graphs_tuple_from_edge_lists(host.all.n_node, host.all.n_edge, host.all.senders, host.all.receivers, ids, x, dev)
            csr_of(g), csr_of(g, by_sender=True)
            return g
        return parent, lambda: device.batch_of(ids), encoder_trainer(dim), 10

    def complete_shape(name, count, dim=200):
        sizes = D.GraphDataset(name, 1).all.n_node[:count].astype(np.int32)
        emb_host = np.random.default_rng(1).standard_normal((int(sizes.sum()), dim)).astype(np.float32) * 0.3
        emb_dev = torch.as_tensor(emb_host).to(dev)

        def parent():
            g = D.transform_example(emb_host, sizes, dev)
            csr_of(g), csr_of(g, by_sender=True)
            return g
        return parent, lambda: D.complete_batch(emb_dev, sizes, dev), flow_trainer(dim), 3

    table = {"cm64_d64": lambda: edge_list_shape("graph_rnn_community_medium", 64, 64),
             "run_gnn_default": lambda: edge_list_shape("graph_rnn_community_small", 8, 100),
             "grid32_complete": lambda: complete_shape("graph_rnn_grid", 32),
             "cm32_complete": lambda: complete_shape("graph_rnn_community_medium", 32)}
    for name in shapes:
        parent, device, trainer, calls = table[name]()
        a, b = parent(), device()
        row = {"shape": name, "graphs": int(a.n_node.shape[0]), "nodes": int(a.nodes.shape[0]), "edges": int(a.senders.shape[0]),
               "routes_agree": same(a, b), "repeats": repeats, "calls_per_region": calls}
        assert row["routes_agree"], name
        del a, b
        step = lambda make: trainer.step(make())
        row.update(timed({"ready_parent": (parent, calls), "ready_device": (device, calls),
                          "iteration_parent": (partial(step, parent), calls), "iteration_device": (partial(step, device), calls)},
                         repeats, sync))
        row["ready_parent_over_device"] = round(row["ready_parent_ms"]["median"] / row["ready_device_ms"]["median"], 2)
        row["iteration_parent_over_device"] = round(row["iteration_parent_ms"]["median"] / row["iteration_device_ms"]["median"], 2)
        print(json.dumps(row), flush=True)
        del parent, device, trainer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
