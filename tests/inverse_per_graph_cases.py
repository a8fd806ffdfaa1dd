"""The batches, nets and latent rows of tests/test_inverse_per_graph_gpu.py, in a module of their own so that
tests/test_inverse_per_graph_cpu.py can check, without a device, that the seeds chosen here leave the float32 CPU
restatement inside half of the device tests' bounds: a failure on the device is then the device's.

Widths and head geometries are those of tests/test_per_graph_gpu.py (MP_CASES, ATTN_CASES, the graph-scope pair), the
batches are dataset graphs behind a one-node graph (boundaries inside the 16-row tiles) or ring + chord graphs of chosen
sizes."""
import os

import numpy as np

import graph_attn_ref as R
import inverse_per_graph_ref as IP
from oracle import gnf_oracle as O
from timestep_gnn_ref import ring_chord_batch

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
TOL = 1e-4      # per node of each graph: log_det_jacobian, log_prob_zs, log_prob_xs
X_TOL = 3e-4    # x against the fp64 g (atol and rtol)

MP_CASES = [
    # D, latent, K, T, agg, combine, weight_sharing, topology
    (2, 16, 3, 2, "mean", "agg", False, "sparse"),
    (64, 64, 3, 2, "sum", "concat", True, "sparse"),
    (100, 48, 2, 2, "sum", "agg", False, "complete"),
    (64, 256, 5, 2, "mean", "concat", False, "complete"),
]
ATTN_CASES = [
    # D, latent, K, T, heads, kq, v, C, concat, kq_div, residual, ws
    (64, 256, 5, 2, 8, 10, 10, 80, True, False, False, False),     # the drivers' defaults: the fused kernel's attention instance
    (20, 48, 2, 1, 3, 7, 5, 20, False, True, False, True),         # no concat, scaled logits, shared nets
]
# the data driver's head geometry (train_grevnet_with_data.py's defaults: dm_attn, one head, kq = v = 64, C = 64, scaled logits)
# at a small width, on the complete graphs that driver builds
ATTN_DATA_DRIVER = (40, 48, 2, 2, 1, 64, 64, 64, True, True, False, False)
# heads of 10 / 10 at H = 16: the attention prologue of the fused kernel in its any-geometry instance (the drivers' default,
# ATTN_CASES[0], runs the instance compiled for H = 32, 8 heads, C = 80)
ATTN_FRONT_GENERIC = (32, 64, 3, 2, 4, 10, 10, 48, True, False, False, False)
ATTN_RESIDUAL = (20, 48, 2, 1, 3, 7, 5, 20, False, True, True, True)
EDGE_SIZES = [1, 17, 16, 33, 2]   # a boundary inside a tile, a tile with one live row, a graph over three tiles, an edgeless graph


def dataset(name):
    d = np.load(os.path.join(DATA, name + ".npz"))
    return d["n_node"], d["n_edge"], d["senders"], d["receivers"]


def dataset_batch(name, ids, topology="sparse"):
    """dataset graphs (+ a one-node graph with its self loop in front: every later boundary moves by one row)"""
    nn, ne, s, r = O.batch_graphs(*dataset(name), ids)
    nn, ne = np.asarray(nn, np.int64), np.asarray(ne, np.int64)
    if topology == "complete":
        s, r = R.complete_edges(nn)
        ne = nn ** 2
    return (np.concatenate([[1], nn]), np.concatenate([[1], ne]), np.concatenate([[0], np.asarray(s) + 1]).astype(np.int32),
            np.concatenate([[0], np.asarray(r) + 1]).astype(np.int32))


def mp_case(case, bn, batch=None):
    d, latent, k, t, agg, combine, ws, topology = case
    hp = dict(D=d, latent=latent, K=k, T=t, agg=agg, combine=combine, epsilon=0.5 if combine == "agg" else 0.0,
              activation="leaky_relu", weight_sharing=ws, use_batch_norm=bn)
    nn, ne, s, r = batch if batch is not None else dataset_batch("grid_small", list(range(12)), topology)
    rng = np.random.default_rng(d * 1000 + latent + (7 if bn else 0))
    z = rng.standard_normal((int(np.sum(nn)), d)).astype(np.float32)
    dense = topology == "complete" or agg == "sum"
    p = O.make_grevnet_params(d + k, d // 2, latent, k, t, combine=combine, weight_sharing=ws,
                              final_scale=(0.02 if topology == "complete" else 0.1) if dense and agg == "sum" else 0.3)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    return hp, nn, ne, s, r, z, p


def attn_case(shape, bn, layer_norm, batch=None):
    d, latent, k, t, nh, kq, vd, c, concat, div, res, ws = shape
    akw = dict(num_heads=nh, kq_dim=kq, v_dim=vd, out_dim=c, concat=concat, kq_dim_division=div, residual=res)
    if layer_norm:
        akw["layer_norm"] = True
    hp = dict(D=d, latent=latent, K=k, T=t, agg="mean", combine="agg", epsilon=0.0, activation="relu", weight_sharing=ws,
              attn=akw, use_batch_norm=bn)
    if batch is None and shape == ATTN_DATA_DRIVER:
        batch = dataset_batch("grid_small", list(range(12)), "complete")
    if batch is None:
        batch = dataset_batch("grid_small", list(range(12))) if d != 64 else dataset_batch("community_medium", [3, 77, 150, 9])
    nn, ne, s, r = batch
    rng = np.random.default_rng(d * 100 + nh)
    z = (rng.standard_normal((int(np.sum(nn)), d)) * (0.3 if res else 1.0)).astype(np.float32)
    p = O.make_attn_grevnet_params(d + nh, d // 2, latent, k, t, weight_sharing=ws, final_scale=0.3, **akw)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    return hp, nn, ne, s, r, z, p


def graph_attn_case(kind, bn, d=8, sizes=(1, 15, 17, 63, 5, 30)):
    nn = np.asarray(sizes, np.int64)
    rng = np.random.default_rng(41 + d)
    ss, rr, ne, off = [], [], [], 0
    for m in nn:   # a random sparse edge list: the graph scope ignores it
        e = int(rng.integers(0, 3 * m + 1))
        ss.append(rng.integers(0, m, e) + off), rr.append(rng.integers(0, m, e) + off), ne.append(e)
        off += m
    s, r = np.concatenate(ss).astype(np.int32), np.concatenate(rr).astype(np.int32)
    kw = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80) if kind == "multihead" else dict(num_heads=1, kq_dim=16, v_dim=16)
    k, t, latent = 3, 2, 64
    p = R.make_graph_attn_grevnet_params(17, d // 2, latent, k, t, final_scale=0.3, **kw)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    z = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    return R.hp_of(p, d, latent, k, t), nn, np.asarray(ne, np.int64), s, r, z, p


def edge_batch(sizes=EDGE_SIZES):
    return ring_chord_batch(sizes)


def width_case(h, bn):
    """coupling halves of H = 1, 3, 50 columns (padded fragments) on the ring + chord batch"""
    return mp_case((2 * h, 32, 3, 2, "mean", "agg", False, "sparse"), bn, batch=edge_batch())


# ---- references ----------------------------------------------------------------------------------------------------------
def gnn_kw(hp):
    return dict(agg=hp["agg"], combine=hp["combine"], epsilon=hp["epsilon"], activation=hp["activation"])


def dense_ref(hp, nn, s, r, z, p):
    o = IP.InversePerGraphDense(s, r, int(np.sum(nn)), **gnn_kw(hp))
    return o.per_graph_terms(z, p, hp["T"], nn, hp["weight_sharing"])


def gather_ref(hp, nn, s, r, z, p, dtype=None):
    """the gather formulation: float64 by default (the graph scope's reference), float32 = what fp32 arithmetic costs"""
    o = IP.InversePerGraphGather(s, r, nn, dtype=dtype, **gnn_kw(hp))
    return o.per_graph_terms(z, p, hp["T"], hp["weight_sharing"])


def per_node_errors(got, ref, nn):
    """max over the graphs of |got - ref| / max(n_g, 1) for the three per-graph sums"""
    num = np.maximum(np.asarray(nn, np.float64), 1.0)
    return {k: float((np.abs(np.asarray(got[k], np.float64) - ref[k]) / num).max())
            for k in ("log_det_jacobian", "log_prob_zs", "log_prob_xs")}


def ln_tol(hp, nn, s, r, z, p, ref):
    """blocks that end in LayerNorm: the bound is the error the CPU fp32 restatement makes on the same inputs (x 6) next to
    the usual 1e-4, per node of each graph - the widened bound of tests/test_per_graph_gpu.py, restated"""
    import torch
    r32 = gather_ref(hp, nn, s, r, z, p, dtype=torch.float32)
    return TOL + 6.0 * max(per_node_errors(r32, ref, nn).values())


def all_cases():
    """(id, builder, reference kind) of every parity / shape case: what the CPU seed check walks"""
    out = []
    for c in MP_CASES:
        for bn in (False, True):
            out.append((f"mp_D{c[0]}_L{c[1]}_{c[4]}_{c[5]}_{c[7]}_{'bn' if bn else 'plain'}", lambda c=c, bn=bn: mp_case(c, bn), "dense"))
    for c in ATTN_CASES + [ATTN_DATA_DRIVER, ATTN_FRONT_GENERIC]:
        for bn in (False, True):
            out.append((f"attn_D{c[0]}_h{c[4]}_{'bn' if bn else 'plain'}", lambda c=c, bn=bn: attn_case(c, bn, False), "dense"))
    out.append(("attn_residual_layer_norm", lambda: attn_case(ATTN_RESIDUAL, False, True), "ln"))
    for kind in ("self_attn", "multihead"):
        for bn in (False, True):
            out.append((f"graph_{kind}_{'bn' if bn else 'plain'}", lambda kind=kind, bn=bn: graph_attn_case(kind, bn), "gather"))
    for h in (1, 3, 50):
        out.append((f"width_H{h}", lambda h=h: width_case(h, True), "dense"))
    out.append(("edge_batch_D64", lambda: mp_case(MP_CASES[1], True, batch=edge_batch()), "dense"))
    return out
