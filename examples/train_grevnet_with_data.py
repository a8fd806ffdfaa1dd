#!/usr/bin/env python3
"""The data-backed trainer's loop (/root/reference/train_grevnet_with_data.py:145-271, 336-416, 520-545) on the
MI355X kernels: node-embedding chunks on disk -> batches of complete graphs (transform_example) -> GRevNet with that
driver's default GNN (dm_attn: one head, kq = v = 64, C = 64, kq_dim_division; :40-46, 303-310) around its wide relu
MLPs (latent 2048 x 3 layers, D = 200, 10 coupling layers, batch norm) -> Adam (beta2 0.999, constant lr); then the
sampling pipeline z ~ N(0, I) -> grevnet(., inverse=False) -> pred_adj(scaled_hacky_sigmoid_l2) -> threshold 0.5
(flow.generate_graphs: the generated graphs come back as a GraphsTuple with its CSR).  --variable_dataset / --max_nodes are
the reference's (batches of consecutive graphs holding fewer than max_nodes nodes); --device_batches keeps the chunks'
embeddings on the device and writes every batch's topology and CSRs there (datasets.complete_batch).

Training the encoder (run_gnn.py) is out of scope, so by default --make_chunks writes embedding chunks whose
embeddings are synthetic (two well-separated clusters per graph, so that the decoder finds structure); point
--train_data_dir at real chunks written by generate_grevnet_training_data.py to use those instead.  With
--encoder_params FILE (an .npz written by gnf_amd.encoder.save_encoder: an encoder's hyper-parameters and
TimestepGNN.get_params()) --make_chunks runs that encoder's forward pass over --dataset instead
(encoder.write_embedding_chunks, the loop of generate_grevnet_training_data.py) and the flow trains on its outputs;
--node_embedding_dim is then the encoder's node width, and when the file names the distance function the encoder was
trained against (run_gnn.py --binary_dist_fn / --tune_sigmoid) the sampled embeddings are decoded with it.

    python examples/train_grevnet_with_data.py --make_chunks --num_train_iters 200 --clip_gradient_by_norm

(With these synthetic, nearly degenerate embeddings the un-clipped defaults diverge after ~50 iterations - the
gradients themselves are verified against the oracle at this width, tools/wide_grad_check.py - which is what the
driver's clip_gradient_by_norm / clip_gradient_by_value flags are for.)
"""
import argparse
import os
import random
import sys
import tempfile
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnf_amd import datasets as D, gnn                                # noqa: E402
from gnf_amd.flow import generate_graphs                             # noqa: E402
from gnf_amd.train import GRevNetTrainer                              # noqa: E402


def make_chunks(path, files, graphs_per_file, dim, rng):
    for k in range(files):
        n_node = rng.integers(8, 20, size=graphs_per_file).astype(np.int32)
        rows = []
        for n in n_node:
            centres = rng.standard_normal((2, dim)) * 0.6
            lab = rng.integers(0, 2, size=n)
            rows.append(centres[lab] + 0.1 * rng.standard_normal((n, dim)))
        D.write_embedding_chunk(os.path.join(path, f"grevnet_train_{k}.pkl"), np.concatenate(rows), n_node)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train_data_dir", default=None)
    ap.add_argument("--make_chunks", action="store_true")
    ap.add_argument("--encoder_params", default=None)             # with --make_chunks: chunks from this encoder's forward pass
    ap.add_argument("--dataset", default="graph_rnn_community_small")
    ap.add_argument("--node_embedding_dim", type=int, default=200)
    ap.add_argument("--latent_dim", type=int, default=2048)
    ap.add_argument("--num_layers", type=int, default=3)
    ap.add_argument("--num_coupling_layers", type=int, default=10)
    ap.add_argument("--bias_init_stddev", type=float, default=0.3)
    ap.add_argument("--no_batch_norm", action="store_true")
    ap.add_argument("--weight_sharing", action="store_true")
    # the reference's defaults (train_grevnet_with_data.py:40-46): dm_attn, one head, kq = v = 64, C = 64
    # ("avg_then_mlp" is not a choice of the reference's ATTN_MAP; kept here as the message-passing alternative)
    ap.add_argument("--attn_type", default="dm_attn", choices=["dm_attn", "singlehead_my_attn", "multihead_my_attn", "avg_then_mlp"])
    ap.add_argument("--use_layer_norm", action="store_true")
    ap.add_argument("--attn_kq_dim", type=int, default=64)
    ap.add_argument("--attn_v_dim", type=int, default=64)
    ap.add_argument("--attn_num_heads", type=int, default=1)
    ap.add_argument("--attn_concat_heads_output_dim", type=int, default=64)
    ap.add_argument("--train_batch_size", type=int, default=32)
    ap.add_argument("--train_epochs", type=int, default=20)
    ap.add_argument("--num_train_iters", type=int, default=60)
    ap.add_argument("--log_every_n_steps", type=int, default=10)
    ap.add_argument("--sample_size", type=int, default=8)
    ap.add_argument("--lr", type=float, default=1e-4)          # lr_type 'constant' (train_grevnet_with_data.py:75-78)
    ap.add_argument("--adam_beta1", type=float, default=0.9)
    ap.add_argument("--adam_beta2", type=float, default=0.999)  # (:86; run_grevnet.py's default is 0.9)
    ap.add_argument("--adam_epsilon", type=float, default=1e-8)
    ap.add_argument("--clip_gradient_by_value", action="store_true")
    ap.add_argument("--clip_gradient_by_norm", action="store_true")
    ap.add_argument("--clip_gradient_norm", type=float, default=10.0)
    ap.add_argument("--random_seed", type=int, default=12345)
    ap.add_argument("--sample_log_prob_xs", action="store_true")   # also log the flow's own density of each generated graph
    # reduce every generated graph to its largest connected component / its nodes with a neighbour (graph_stats.keep_subgraphs)
    ap.add_argument("--keep_generated", default="all", choices=["all", "largest_component", "non_isolated"])
    # uniqueness and novelty of the sampled graphs against the training graphs of --dataset (graph_stats.uniqueness_novelty)
    ap.add_argument("--report_novelty", action="store_true")
    # degree / clustering MMD^2 of the sampled graphs against the test graphs of --dataset, beside the same scores of Erdos-Renyi
    # and Barabasi-Albert graphs fitted to its training graphs (random_graphs.evaluate_baselines)
    ap.add_argument("--report_baselines", action="store_true")
    # train_grevnet_with_data.py:60-61, 471-473: batches of consecutive graphs holding fewer than --max_nodes nodes
    ap.add_argument("--variable_dataset", action="store_true")
    ap.add_argument("--max_nodes", type=int, default=1500)
    # keep the chunks' embeddings on the device and build every batch's topology there (datasets.complete_batch)
    ap.add_argument("--device_batches", action="store_true")
    F = ap.parse_args()
    random.seed(F.random_seed)
    np.random.seed(F.random_seed)
    torch.manual_seed(F.random_seed)
    gnn.set_random_seed(F.random_seed)
    rng = np.random.default_rng(F.random_seed)
    dev = torch.device("cuda", 0)
    tmp = None
    decode_with = {}   # generate_graphs' distance_fn: the one the encoder of --encoder_params was trained against, if it says
    if F.train_data_dir is None:
        if not F.make_chunks:
            raise SystemExit("give --train_data_dir or --make_chunks")
        tmp = tempfile.TemporaryDirectory()
        F.train_data_dir = tmp.name
        if F.encoder_params is None:
            make_chunks(F.train_data_dir, 3, 10 * F.train_batch_size, F.node_embedding_dim, rng)
        else:
            from gnf_amd import encoder as E
            enc, enc_hp = E.load_encoder(F.encoder_params)
            F.node_embedding_dim = int(enc_hp["node_dim"])
            if "distance" in enc_hp:
                decode_with = {"distance_fn": E.distance_of(enc_hp)}
                print(f"decoding with {enc_hp['distance']}")
            paths = E.write_embedding_chunks(enc, D.GraphDataset(F.dataset, F.node_embedding_dim, seed=F.random_seed),
                                             F.train_data_dir, 30 * F.train_batch_size, F.train_batch_size, device=dev,
                                             chunk_bytes=10 * F.train_batch_size * 16 * F.node_embedding_dim * 4)
            print(f"{len(paths)} embedding chunks from the encoder in {F.encoder_params} over {F.dataset}")
    # sort_files: the reference consumes the chunks in os.listdir order, which differs from one temporary directory
    # to the next (and with it the whole loss curve); sorted here so that a run of this demo is reproducible
    chunk_device = dev if F.device_batches else None
    if F.variable_dataset:
        data = D.GrevnetDatasetVariable(F.train_data_dir, F.max_nodes, sort_files=True, device=chunk_device)
    else:
        data = D.GrevnetDatasetFixed(F.train_data_dir, F.train_batch_size, F.train_epochs, sort_files=True, device=chunk_device)
    # a (node_embeddings, n_node) batch -> GraphsTuple with the complete topology: assembled on the host and uploaded, or
    # (--device_batches) written on the device next to both of its CSRs
    to_graph = D.complete_batch if F.device_batches else D.transform_example

    make_mlp_fn = partial(gnn.make_mlp_model, F.latent_dim, F.node_embedding_dim / 2, F.num_layers,
                          activation=gnn.relu, l2_regularizer_weight=0.000001, bias_init_stddev=F.bias_init_stddev)
    make_gnn_fn = {
        "avg_then_mlp": partial(gnn.avg_then_mlp_gnn, make_mlp_fn, 1.0),
        "dm_attn": partial(gnn.dm_self_attn_gnn, kq_dim=F.attn_kq_dim, v_dim=F.attn_v_dim, make_mlp_fn=make_mlp_fn,
                           num_heads=F.attn_num_heads, concat_heads_output_dim=F.attn_concat_heads_output_dim,
                           kq_dim_division=True, layer_norm=F.use_layer_norm),
        # train_grevnet_with_data.py:289-302: whole-graph attention
        "singlehead_my_attn": partial(gnn.self_attn_gnn, kq_dim=F.attn_kq_dim, v_dim=F.attn_v_dim, make_mlp_fn=make_mlp_fn,
                                      kq_dim_division=True),
        "multihead_my_attn": partial(gnn.multihead_self_attn_gnn, kq_dim=F.attn_kq_dim, v_dim=F.attn_v_dim,
                                     concat_heads_output_dim=F.attn_concat_heads_output_dim, make_mlp_fn=make_mlp_fn,
                                     num_heads=F.attn_num_heads, kq_dim_division=True, layer_norm=F.use_layer_norm),
    }[F.attn_type]
    grevnet = gnn.GRevNet(make_gnn_fn, F.num_coupling_layers, F.node_embedding_dim,
                          use_batch_norm=not F.no_batch_norm, weight_sharing=F.weight_sharing)
    trainer = GRevNetTrainer(grevnet, lr=F.lr, adam_beta1=F.adam_beta1, adam_beta2=F.adam_beta2, adam_epsilon=F.adam_epsilon,
                             use_lr_decay=False, clip_gradient_by_value=F.clip_gradient_by_value,
                             clip_gradient_by_norm=F.clip_gradient_by_norm, clip_gradient_norm=F.clip_gradient_norm)
    t0 = time.perf_counter()
    for iteration in range(F.num_train_iters + 1):
        z, n_node = data.train_batch()
        graph = to_graph(z, n_node, dev)
        v = trainer.step(graph)
        if iteration % F.log_every_n_steps == 0:
            print(f"iteration {iteration:5d} ({time.perf_counter() - t0:6.1f} s): total_loss {float(v['total_loss']):12.3f} "
                  f"per_node_loss {float(v['loss_per_node']):9.4f} log_det_jacobian {float(v['log_det_jacobian']):12.3f} "
                  f"batch nodes {graph.nodes.shape[0]}")
            if not np.isfinite(float(v["total_loss"])):
                raise SystemExit("loss is not finite")
    # held-out likelihood per GRAPH: one more batch, one forward pass (the moments of the batch-norm bijectors are the batch's)
    from gnf_amd.flow import log_prob_per_graph
    z, n_node = data.train_batch()
    nll = -log_prob_per_graph(grevnet, to_graph(z, n_node, dev))["log_prob_xs_per_node"]
    print(f"per-node NLL over the {nll.shape[0]} graphs of one batch: min {float(nll.min()):.4f} mean {float(nll.mean()):.4f} "
          f"max {float(nll.max()):.4f}")
    # ---- sampling pipeline (train_grevnet_with_data.py:397-416, 526-540) ---------------------------------------
    n_node = np.asarray(random.sample(list(data.n_node) * F.sample_size, F.sample_size), np.int32)
    shape = (int(n_node.sum()), F.node_embedding_dim)
    shell = to_graph(torch.zeros(shape, device=dev) if F.device_batches else np.zeros(shape, np.float32), n_node, dev)
    # sample -> flow in reverse -> edge lists + CSR, all on the device (--sample_log_prob_xs: log p(x) of each graph from the same pass)
    keep = None if F.keep_generated == "all" else F.keep_generated
    out = generate_graphs(grevnet, shell, log_prob=F.sample_log_prob_xs, keep=keep, **decode_with)
    rows = torch.stack([out["graph"].n_node.to(dev, torch.float64), out["graph"].n_edge.to(torch.float64),
                        out["sample_log_prob_per_graph"]]).cpu().numpy()          # the one device-to-host copy of the tail
    for i, (nodes, edges, mean_lp) in enumerate(rows.T):
        print(f"sampled graph {i}: {int(nodes)} nodes, {int(edges) // 2} edges, mean sample log-prob {mean_lp:.2f}")
    if keep is not None:
        from gnf_amd.graph_stats import graph_components
        parts = graph_components(out["graph"])["n_components"].to(torch.float64).mean()
        share = float(out["kept"]["total_nodes"]) / max(int(n_node.sum()), 1)
        print(f"generated graphs: mean n_components {float(parts):.2f}, --keep_generated {keep} keeps {share:.1%} of the nodes, "
              f"{int(out['kept']['total_edges']) // 2} edges")
    if F.report_novelty:
        from gnf_amd.graphs import data_dicts_to_graphs_tuple
        from gnf_amd.graph_stats import graph_hashes, uniqueness_novelty
        ds = D.GraphDataset(F.dataset, 1, seed=F.random_seed)
        train = graph_hashes(data_dicts_to_graphs_tuple(ds.all.data_dicts(ds.train_ids, ds._features), dev))   # hashed once
        classes = uniqueness_novelty(train, train)["counts"][1]
        sampled = out["kept"]["graph"] if keep is not None else out["graph"]
        u = uniqueness_novelty(sampled, train)
        print(f"sampled graphs: uniqueness {float(u['uniqueness']):.1%}, novelty {float(u['novelty']):.1%}, unique and novel "
              f"{float(u['unique_novel']):.1%} of {int(u['counts'][0])}; the {len(ds.train_ids)} training graphs of {F.dataset} "
              f"fall into {int(classes)} isomorphism classes (Weisfeiler-Lehman hash, 3 rounds)")
    if F.report_baselines:
        from gnf_amd.graphs import data_dicts_to_graphs_tuple
        from gnf_amd.graph_stats import evaluate_generated, graph_stats
        from gnf_amd.random_graphs import evaluate_baselines
        ds = D.GraphDataset(F.dataset, 1, seed=F.random_seed)
        train_graphs = data_dicts_to_graphs_tuple(ds.all.data_dicts(ds.train_ids, ds._features), dev)
        test_stats = graph_stats(data_dicts_to_graphs_tuple(ds.all.data_dicts(ds.test_ids, ds._features), dev))   # scored once
        sampled = out["kept"]["graph"] if keep is not None else out["graph"]
        rows = {"model": evaluate_generated(sampled, test_stats),
                **evaluate_baselines(train_graphs, test_stats, seed=F.random_seed)}
        print(f"scores against the {len(ds.test_ids)} test graphs of {F.dataset} (MMD^2; baselines fitted to the "
              f"{len(ds.train_ids)} training graphs):")
        for name, row in rows.items():
            print(f"  {name:16s} degree_mmd {float(row['degree_mmd']):.6f} clustering_mmd {float(row['clustering_mmd']):.6f}")
    if F.sample_log_prob_xs:
        for i, lp in enumerate(out["log_prob_xs_per_node"].cpu().numpy()):
            print(f"sampled graph {i}: log_prob_xs_per_node {lp:.4f}")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
