"""What consumes the encoder's forward pass (gnn.TimestepGNN, gnf_timestep_gnn_f32): the evaluation figures run_gnn.py logs
and the embedding chunks the GRevNet flow is trained on.  Both run the encoder with is_training=False; training the encoder is
train.EncoderTrainer (gnn.TimestepGNN.forward_train / backward), whose result save_encoder stores.

  evaluate                 run_gnn.py:441-465: encoder -> adj_loss.binary_loss and its counts
  write_embedding_chunks   generate_grevnet_training_data.py:78-120: encoder outputs cut into chunk files
  save_encoder / load_encoder   an encoder's hyper-parameters and TimestepGNN.get_params() in one .npz, with the distance
                           function it was trained against (distance_of)
"""
import json
import os

import numpy as np
import torch

from . import adj_loss, datasets
from .flow import scaled_hacky_sigmoid_l2
from .gnn import TimestepGNN

CHUNK_BYTES = 100e6   # generate_grevnet_training_data.py:80,90: a chunk is closed once it holds more than 100 MB of fp32


def evaluate(encoder, graphs, distance_fn=scaled_hacky_sigmoid_l2, use_soft_labels=False, report=False, **loss_kw):
    """The quantities run_gnn.py:441-465 logs for a batch, from encoder(graphs, is_training=False) and binary_loss of its
    output against the batch's own topology.  Returns a dict of device tensors (nothing is read back):
      "gnn_output"                  the encoder's GraphsTuple
      "sum_loss", "mean_loss"       0-d float64 (loss.py:186-187)
      "total_incorrect_edges", "false_positive_edges", "false_negative_edges"   0-d float64 (loss.py:104-116)
      "incorrect_edges_per_graph"   int32 [B] (loss.py:88-95)
      "incorrect_edges_per_node"    0-d float64: total_incorrect_edges / N
      "loss"                        binary_loss' own result dict
    loss_kw goes to binary_loss (max_nodes_per_graph or n_node_host make the call free of host synchronisation).
    report=True adds "report": adj_loss.reconstruction_report of the same output against the batch at threshold 0.5 (which
    pairs are wrong and with what score, run_gnn_inference.py:107-163), with binary_loss' node bound; a dict is passed on as
    that call's options (threshold, quantiles, per_graph, edge_capacity).  Without it the launches are those of before."""
    out = encoder(graphs, False)
    res = adj_loss.binary_loss(out, graphs, distance_fn=distance_fn, use_soft_labels=use_soft_labels, **loss_kw)
    total = adj_loss.total_incorrect_edges(res)
    n = int(graphs.nodes.shape[0])
    result = {"gnn_output": out, "sum_loss": res["sum_loss"], "mean_loss": res["mean_loss"], "total_incorrect_edges": total,
              "incorrect_edges_per_node": total / float(max(n, 1)),
              "incorrect_edges_per_graph": adj_loss.incorrect_edges_per_graph(res),
              "false_positive_edges": adj_loss.false_positive_edges(res),
              "false_negative_edges": adj_loss.false_negative_edges(res), "loss": res}
    if report:
        bound = {k: loss_kw[k] for k in ("max_nodes_per_graph", "n_node_host") if k in loss_kw}
        options = dict(report) if isinstance(report, dict) else {}
        result["report"] = adj_loss.reconstruction_report(out, graphs, distance_fn=distance_fn, **{**bound, **options})
    return result


def write_embedding_chunks(encoder, dataset, directory, num_examples, batch_size, device=None, prefix="grevnet_train",
                           chunk_bytes=CHUNK_BYTES):
    """generate_grevnet_training_data.py:78-120 (its pickled output): draw dataset.get_next_train_batch(batch_size), run the
    encoder with is_training=False, append its rows and the batch's n_node; whenever the pending rows exceed chunk_bytes of
    fp32 they are written as one chunk (datasets.write_embedding_chunk) and a new one starts.  Stops once num_examples
    graphs have gone through and writes what is pending - the reference goes on until its last chunk is full as well, and
    leaves an empty file behind; here the last chunk is short and every file holds graphs.  Returns the chunk paths, which
    GrevnetDatasetFixed / GrevnetDatasetVariable read back (sort_files=True: in this order)."""
    if batch_size < 1 or num_examples < 1:
        raise ValueError("batch_size and num_examples must be >= 1")
    os.makedirs(directory, exist_ok=True)
    device = torch.device("cuda", 0) if device is None else device
    paths, rows, sizes, pending, seen = [], [], [], 0, 0

    def flush():
        nonlocal rows, sizes, pending
        path = os.path.join(directory, f"{prefix}_{len(paths):05d}.pkl")
        datasets.write_embedding_chunk(path, np.concatenate(rows), np.concatenate(sizes))
        paths.append(path)
        rows, sizes, pending = [], [], 0

    while seen < num_examples:
        graphs = dataset.get_next_train_batch(batch_size, device)
        emb = encoder(graphs, False).nodes
        rows.append(emb.cpu().numpy())
        sizes.append(graphs.n_node.cpu().numpy().astype(np.int32))
        pending += rows[-1].size * 4
        seen += int(sizes[-1].shape[0])
        if pending > chunk_bytes:
            flush()
    if rows:
        flush()
    return paths


# ---- an encoder in one file --------------------------------------------------------------------------------------------------
_ENCODER_KEYS = ("num_timesteps", "weight_sharing", "use_batch_norm", "residual", "test_local_stats", "use_layer_norm")


def make_encoder(hp):
    """hp: factories.make_gnn_fn's keys for a GNN on nodes of width hp["node_dim"] (latent, K, activation and agg / combine /
    epsilon or attn), plus num_timesteps and optionally weight_sharing, use_batch_norm, residual, test_local_stats,
    use_layer_norm (TimestepGNN's defaults)."""
    from .factories import make_gnn_fn
    return TimestepGNN(make_gnn_fn(hp), **{k: hp[k] for k in _ENCODER_KEYS if k in hp})


def _flatten(params):
    flat = {}
    for q, net in enumerate(params["nets"]):
        mlp = net["mlp"] if isinstance(net, dict) else net
        for j, (w, b) in enumerate(mlp):
            flat[f"net{q}.W{j}"], flat[f"net{q}.b{j}"] = w, b
        if isinstance(net, dict):
            for k, v in net["attn"].items():
                flat[f"net{q}.attn.{k}"] = v
    for key in ("bn", "ln"):
        for q, d in enumerate(params.get(key) or []):
            for k, v in d.items():
                flat[f"{key}{q}.{k}"] = v
    return flat


_DISTANCE_KINDS = ("scaled_hacky_sigmoid_l2", "hacky_sigmoid_l2", "sigmoid_l2")


def distance_entry(distance_fn):
    """{"kind", "temp", "shift"} of a distance token: what save_encoder stores.  A TunedSigmoidL2's values are read back from
    the device here, once; it is stored as the sigmoid_l2 it has become (with "scale_by_sqrt_dim": false if it is unscaled)."""
    if isinstance(distance_fn, adj_loss.TunedSigmoidL2):
        temp, shift = distance_fn.values()
        entry = {"kind": "sigmoid_l2", "temp": temp, "shift": shift}
        if not distance_fn.scale_by_sqrt_dim:
            entry["scale_by_sqrt_dim"] = False
        return entry
    temp, shift, by_sqrt = adj_loss._distance_params(distance_fn)
    kind = "sigmoid_l2" if isinstance(distance_fn, adj_loss.sigmoid_l2) else _DISTANCE_KINDS[0 if by_sqrt else 1]
    return {"kind": kind, "temp": temp, "shift": shift}


def distance_of(hp):
    """The distance token of a loaded encoder's hyper-parameters: what to hand pred_adj, decode_graphs, generate_graphs and
    evaluate.  Files written without a "distance" entry give the default, scaled_hacky_sigmoid_l2."""
    entry = hp.get("distance")
    if entry is None or entry["kind"] == "scaled_hacky_sigmoid_l2":
        return scaled_hacky_sigmoid_l2
    if entry["kind"] == "hacky_sigmoid_l2":
        return adj_loss.hacky_sigmoid_l2
    if entry["kind"] == "sigmoid_l2":
        if not entry.get("scale_by_sqrt_dim", True):
            return adj_loss.TunedSigmoidL2(entry["temp"], entry["shift"], scale_by_sqrt_dim=False)
        return adj_loss.sigmoid_l2(entry["temp"], entry["shift"])
    raise ValueError(f"distance kind {entry['kind']!r}: one of {_DISTANCE_KINDS}")


def save_encoder(path, hp, encoder, distance_fn=None):
    """hp (make_encoder's) and encoder.get_params() as one .npz; with distance_fn, hp gains "distance" (distance_entry)"""
    if distance_fn is not None:
        hp = dict(hp, distance=distance_entry(distance_fn))
    np.savez(path, hp_json=np.array(json.dumps(hp)), **_flatten(encoder.get_params()))


def load_encoder(path):
    """make_encoder(hp).set_params(...) of a file written by save_encoder"""
    d = np.load(path)
    hp = json.loads(str(d["hp_json"]))
    enc = make_encoder(hp)
    nets = []
    for q in range(len(enc.gnns)):
        mlp, j = [], 0
        while f"net{q}.W{j}" in d.files:
            mlp.append((d[f"net{q}.W{j}"], d[f"net{q}.b{j}"]))
            j += 1
        attn = {k[len(f"net{q}.attn."):]: d[k] for k in d.files if k.startswith(f"net{q}.attn.")}
        nets.append({"attn": attn, "mlp": mlp} if attn else mlp)
    params = {"nets": nets}
    for key, keys in (("bn", ("gamma", "beta", "moving_mean", "moving_variance")), ("ln", ("gamma", "beta"))):
        if f"{key}0.gamma" in d.files:
            params[key] = [{k: d[f"{key}{q}.{k}"] for k in keys} for q in range(enc.num_timesteps)]
    return enc.set_params(params), hp
