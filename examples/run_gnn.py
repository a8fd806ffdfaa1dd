"""Stage 1 of the pipeline on the device: train the graph auto-encoder (the reference driver run_gnn.py's loop with its flag
names, kept small) and save it where examples/train_grevnet_with_data.py --make_chunks --encoder_params FILE reads it.

    python examples/run_gnn.py --dataset graph_rnn_community_small --num_train_iters 200 --save_path encoder.npz
    python examples/train_grevnet_with_data.py --make_chunks --encoder_params encoder.npz --attn_type avg_then_mlp ...

Batches come from datasets.GraphDataset (random Gaussian node features on the dataset's topologies) or, with --device_batches,
from datasets.DeviceGraphDataset (the dataset stays on the device; a batch and both of its CSRs are one call); every iteration is
train.EncoderTrainer.step (train-forward, binary_loss, backward, Adam); every --eval_every_n_steps a random test batch goes
through encoder.evaluate, and the figures run_gnn.py:441-465 logs are printed.  --denoising trains the denoising auto-encoder:
the encoder reads the batch with edges deleted at random (--deletion_prob; datasets.NoisyGraphDataset, on the device with
--device_batches) and is scored against the batch as it was; the log line then reads NUM_NODES:NUM_REMOVED:NUM_INCORRECT.
--binary_dist_fn picks the decoder's distance
function and --tune_sigmoid (with sigmoid_l2) trains its temp and shift from 10 and 1 (run_gnn.py:146-165); the function, with
the trained values, is saved with the encoder.  --loss_type triplet trains on the sampled triplet loss instead (run_gnn.py:82-91,
249-252: --triplet_dist_fn scores the pairs, --triplet_loss_fn margin | relative forms the terms, --num_sampling_loops rounds per
node; the loss is summed over the nodes, the samples of iteration k are those of --random_seed + k); the edge-error figures and
the evaluation then use --triplet_adj_dist_fn, which is also what is saved.  The message-passing --attn_type values train;
the attention ones exit with the library's GNF_EUNSUPPORTED text (their encoder backward is not built).

As in the reference, a pair whose logit lies inside Keras' clip gets no gradient: unit-scale random
features put nearly every pair of a fresh encoder's embeddings that far apart, and the loss then hardly moves.  A smaller
--gaussian_scale (0.3) starts the pairs inside the clip's range."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnf_amd import _abi, adj_loss, datasets as D, encoder as E, gnn   # noqa: E402
from gnf_amd.flow import scaled_hacky_sigmoid_l2                        # noqa: E402
from gnf_amd.train import EncoderTrainer                                # noqa: E402
from gnf_amd.triplet_loss import (dot, exp_l2, hacky_cauchy_l2, l2, margin_loss, relative_loss,   # noqa: E402
                                  sigmoid_dot)

# DIST_FN_MAP / TRIPLET_LOSS_FN_MAP of run_gnn.py:155-166 (sigmoid_l2 at run_gnn.py:146-147's temp 10, shift 1)
DIST_FNS = {"scaled_hacky_sigmoid_l2": scaled_hacky_sigmoid_l2, "hacky_sigmoid_l2": adj_loss.hacky_sigmoid_l2,
            "sigmoid_l2": adj_loss.sigmoid_l2(10.0, 1.0)}
TRIPLET_DIST_FNS = dict(DIST_FNS, l2=l2, dot=dot, exp_l2=exp_l2, hacky_cauchy_l2=hacky_cauchy_l2, sigmoid_dot=sigmoid_dot)
TRIPLET_LOSS_FNS = {"margin": margin_loss(), "relative": relative_loss}
MESSAGE_PASSING = {"avg_then_mlp": ("mean", "agg"), "sum_then_mlp": ("sum", "agg"), "sum_concat_then_mlp": ("sum", "concat"),
                   "avg_concat_then_mlp": ("mean", "concat")}


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="graph_rnn_community_small")
    ap.add_argument("--attn_type", default="avg_then_mlp", choices=list(MESSAGE_PASSING) + ["dm_attn"])
    ap.add_argument("--node_embedding_dim", type=int, default=100)
    ap.add_argument("--gaussian_scale", type=float, default=1.0)
    ap.add_argument("--latent_dim", type=int, default=2048)
    ap.add_argument("--num_layers", type=int, default=3)
    ap.add_argument("--num_processing_steps", type=int, default=10)
    ap.add_argument("--bias_init_stddev", type=float, default=0.3)
    ap.add_argument("--node_weighting_epsilon", type=float, default=2.0)
    ap.add_argument("--no_weight_sharing", action="store_true")
    ap.add_argument("--no_batch_norm", action="store_true")
    ap.add_argument("--use_layer_norm", action="store_true")
    ap.add_argument("--no_residual", action="store_true")
    ap.add_argument("--no_bn_test_local_stats", action="store_true")
    ap.add_argument("--use_soft_labels", action="store_true")
    ap.add_argument("--binary_dist_fn", default="scaled_hacky_sigmoid_l2",
                    choices=["scaled_hacky_sigmoid_l2", "hacky_sigmoid_l2", "sigmoid_l2"])
    ap.add_argument("--tune_sigmoid", action="store_true")
    ap.add_argument("--loss_type", default="binary", choices=list(EncoderTrainer.LOSS_TYPES))
    ap.add_argument("--triplet_dist_fn", default="l2", choices=list(TRIPLET_DIST_FNS))
    ap.add_argument("--triplet_adj_dist_fn", default="hacky_sigmoid_l2", choices=list(DIST_FNS))
    ap.add_argument("--triplet_loss_fn", default="margin", choices=list(TRIPLET_LOSS_FNS))
    ap.add_argument("--num_sampling_loops", type=int, default=8)
    ap.add_argument("--train_batch_size", type=int, default=8)
    ap.add_argument("--num_train_iters", type=int, default=200000)
    ap.add_argument("--log_every_n_steps", type=int, default=100)
    ap.add_argument("--eval_every_n_steps", type=int, default=100)
    ap.add_argument("--no_run_eval", action="store_true")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--lr_type", default="polynomial_decay", choices=list(EncoderTrainer.LR_TYPES))
    ap.add_argument("--lr_fixed_decay_steps", type=int, default=1000)
    ap.add_argument("--lr_fixed_decay_rate", type=float, default=0.99)
    ap.add_argument("--lr_fixed_decay_staircase", action="store_true")
    ap.add_argument("--adam_beta1", type=float, default=0.9)
    ap.add_argument("--adam_beta2", type=float, default=0.999)
    ap.add_argument("--adam_epsilon", type=float, default=1e-8)
    ap.add_argument("--random_seed", type=int, default=12345)
    ap.add_argument("--save_path", default="encoder.npz")
    # keep the dataset on the device and assemble every batch, with both of its CSRs, there (datasets.DeviceGraphDataset);
    # the node features then come from a device generator: same distribution, other numbers than the host route's
    ap.add_argument("--device_batches", action="store_true")
    # the denoising auto-encoder (run_gnn.py:40-41, 238): the encoder reads the batch with edges deleted at random
    # (datasets.NoisyGraphDataset / perturb_batch: every node pair's edges go with probability --deletion_prob, self loops stay)
    # and is scored against the batch as it was
    ap.add_argument("--denoising", action="store_true")
    ap.add_argument("--deletion_prob", type=float, default=0.3)
    return ap


def main():
    ap = make_parser()
    F = ap.parse_args()
    if F.tune_sigmoid and F.binary_dist_fn != "sigmoid_l2":
        ap.error("--tune_sigmoid trains the parameters of --binary_dist_fn sigmoid_l2")
    if F.tune_sigmoid and F.loss_type == "triplet":
        ap.error("--tune_sigmoid belongs to --loss_type binary")
    triplet = F.loss_type == "triplet"
    random.seed(F.random_seed)
    np.random.seed(F.random_seed)
    torch.manual_seed(F.random_seed)
    gnn.set_random_seed(F.random_seed)
    dev = torch.device("cuda", 0)

    hp = dict(node_dim=F.node_embedding_dim, latent=F.latent_dim, K=F.num_layers, activation="leaky_relu",
              bias_init_stddev=F.bias_init_stddev, num_timesteps=F.num_processing_steps, weight_sharing=not F.no_weight_sharing,
              use_batch_norm=not F.no_batch_norm, use_layer_norm=F.use_layer_norm, residual=not F.no_residual,
              test_local_stats=not F.no_bn_test_local_stats)
    if F.attn_type in MESSAGE_PASSING:
        agg, combine = MESSAGE_PASSING[F.attn_type]
        hp.update(agg=agg, combine=combine, epsilon=F.node_weighting_epsilon if combine == "agg" else 0.0)
    else:   # run_gnn.py's dm_attn defaults; the library refuses its backward pass below
        hp.update(agg="sum", combine="agg", epsilon=0.0,
                  attn=dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80, concat=True, kq_dim_division=False, residual=False))
    enc = E.make_encoder(hp)
    dist_fn = DIST_FNS[F.binary_dist_fn]
    trainer = EncoderTrainer(enc, lr=F.lr, adam_beta1=F.adam_beta1, adam_beta2=F.adam_beta2, adam_epsilon=F.adam_epsilon,
                             lr_type=F.lr_type, num_train_iters=F.num_train_iters, lr_fixed_decay_steps=F.lr_fixed_decay_steps,
                             lr_fixed_decay_rate=F.lr_fixed_decay_rate, lr_fixed_decay_staircase=F.lr_fixed_decay_staircase,
                             use_soft_labels=F.use_soft_labels, distance_fn=dist_fn, tune_sigmoid=F.tune_sigmoid,
                             loss_type=F.loss_type, triplet_dist_fn=TRIPLET_DIST_FNS[F.triplet_dist_fn],
                             triplet_adj_dist_fn=DIST_FNS[F.triplet_adj_dist_fn], triplet_loss_fn=TRIPLET_LOSS_FNS[F.triplet_loss_fn],
                             num_sampling_loops=F.num_sampling_loops, seed=F.random_seed)
    # the decoder's distance function: with --tune_sigmoid the token whose parameters the trainer moves, under the triplet
    # loss the one its edge-error figures are counted with (pred_adj of loss.py:268)
    dist_fn = trainer.triplet_adj_dist_fn if triplet else trainer.distance_fn
    if F.denoising:
        dataset = D.NoisyGraphDataset(F.dataset, F.node_embedding_dim, F.deletion_prob, F.gaussian_scale, seed=F.random_seed,
                                      device=dev if F.device_batches else None)
    elif F.device_batches:
        dataset = D.DeviceGraphDataset(F.dataset, F.node_embedding_dim, F.gaussian_scale, seed=F.random_seed, device=dev)
    else:
        dataset = D.GraphDataset(F.dataset, F.node_embedding_dim, F.gaussian_scale, seed=F.random_seed)

    def log(prefix, it, n_node, res, out_nodes=None, num_removed=None):
        per_graph = adj_loss.incorrect_edges_per_graph(res).cpu().numpy()
        total = float(adj_loss.total_incorrect_edges(res))
        print("*" * 100)
        print(f"iteration num: {it}")
        if num_removed is not None:      # run_gnn.py:405-413
            print("NUM_NODES:NUM_REMOVED:NUM_INCORRECT")
            print(", ".join(f"{a}:{b}:{c}" for a, b, c in zip(n_node.cpu().numpy(), num_removed.cpu().numpy(), per_graph)))
        else:
            print("NUM_NODES:NUM_INCORRECT")
            print(", ".join(f"{a}:{b}" for a, b in zip(n_node.cpu().numpy(), per_graph)))
        print(f"{prefix}sum loss: {float(res['sum_loss'])}")
        print(f"{prefix}mean loss: {float(res['mean_loss'])}")
        if "skipped_terms" in res:
            print(f"{prefix}triplet terms without a candidate: {int(res['skipped_terms'].sum())}")
        print(f"{prefix}total incorrect edges: {total}")
        print(f"{prefix}incorrect edges per node: {total / max(int(n_node.sum()), 1)}")
        print(f"{prefix}false positive edges: {float(adj_loss.false_positive_edges(res))}")
        print(f"{prefix}false negative edges: {float(adj_loss.false_negative_edges(res))}")
        if out_nodes is not None:
            print(f"gnn output norm:{float(out_nodes.norm(dim=1).mean())}")

    for iteration in range(F.num_train_iters):
        num_removed = None
        if F.denoising:
            graph, noisy, num_removed = dataset.get_next_train_batch(F.train_batch_size, dev)
        else:
            graph = dataset.get_next_train_batch(F.train_batch_size, dev)
        try:
            res = trainer.step(noisy, true_graph=graph) if F.denoising else trainer.step(graph)
        except _abi.GnfError as e:
            raise SystemExit(str(e))
        if iteration % F.log_every_n_steps == 0:
            log("", iteration, graph.n_node, res, res["gnn_output"].nodes, num_removed)
            print(f"learning rate: {trainer.current_learning_rate()}")
            if F.tune_sigmoid:
                temp, shift = dist_fn.values()
                print(f"temp: {temp!r} shift: {shift!r}")
            if not np.isfinite(float(res["sum_loss"])):
                raise SystemExit("loss is not finite")
        if not F.no_run_eval and iteration % F.eval_every_n_steps == 0:
            test = dataset.get_random_test_batch(F.train_batch_size, dev)
            log("eval ", iteration, test.n_node, E.evaluate(enc, test, distance_fn=dist_fn, use_soft_labels=F.use_soft_labels)["loss"])
    E.save_encoder(F.save_path, hp, enc, distance_fn=dist_fn)
    print(f"encoder saved to {F.save_path} after {trainer.global_step} steps")
    if F.tune_sigmoid:
        temp, shift = dist_fn.values()
        print(f"final temp: {temp!r} shift: {shift!r}")


if __name__ == "__main__":
    main()
