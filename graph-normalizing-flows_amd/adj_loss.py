"""How well do embeddings reconstruct the graph they belong to: loss.py's binary_loss, its edge-error counts and the gradient
of the loss with respect to the embeddings, on the device (gnf_adj_loss_dist_f32, include/gnf_distance.h and
include/gnf_adj_loss.h) - and, for a sigmoid_l2 whose temp and shift are trained with the encoder (run_gnn.py --tune_sigmoid),
the gradient with respect to those two as well (TunedSigmoidL2).

The reference builds a dense [N, N] true adjacency, a dense distance_fn(nodes) and their element-wise cross-entropy
(loss.py:162-188), counts wrong entries on those matrices (loss.py:88-116) and lets tf.gradients differentiate through
them.  Here the embeddings meet the true graph's receiver-sorted CSR pair by pair inside each graph; the arithmetic of a pair
is flow.pred_adj's, so the verdict on an edge agrees with `pred_adj > 0.5` and flow.decode_graphs bit for bit.
reconstruction_report (include/gnf_adj_report.h) says WHICH pairs are wrong and with what score: run_gnn_inference.py:107-163.
HIP only: CPU tensors raise GnfError.

Unpinned upstream facts this relies on: tf.keras.backend.binary_crossentropy of TF 1.x clips the probability to
[1e-7, 1 - 1e-7] (Keras' epsilon, K.epsilon() = 1e-7), converts it to a logit and applies sigmoid cross-entropy with logits;
tf.clip_by_value passes no gradient where it clips.
"""
import ctypes as C

import torch

from . import _abi
from .flow import scaled_hacky_sigmoid_l2
from .graph_stats import _node_bound

MAX_NODES_PER_GRAPH = 65536
RESULT_KEYS = ("sum_loss", "mean_loss", "loss_per_graph", "false_positive_pairs", "false_negative_pairs")


def hacky_sigmoid_l2(*_a, **_k):
    """Token for the distance function of loss.py:36-42, sigmoid(10 * (1 - ||z_i - z_j||^2)); the arithmetic runs inside
    the library."""
    raise NotImplementedError("token only: pass it as distance_fn to binary_loss")


class sigmoid_l2:
    """Token for loss.py:56-62 with its two parameters bound, sigmoid(temp * (shift - ||z_i - z_j||^2 / sqrt(D))):
    binary_loss(..., distance_fn=sigmoid_l2(3.0, 2.0))."""

    def __init__(self, temp, shift):
        self.temp, self.shift = float(temp), float(shift)

    def __repr__(self):
        return f"sigmoid_l2(temp={self.temp}, shift={self.shift})"


class TunedSigmoidL2:
    """Token for sigmoid_l2 with trainable parameters (run_gnn.py:146-165, --tune_sigmoid): temp and shift live in a device
    fp32 [2] tensor, `.params`, which the kernels read at run time - an optimiser step on the device changes what the next
    launch computes.  The tensor is created with (temp, shift) on first use, on the embeddings'
    device, or adopted with bind(); values() reads the two floats back and is the only call here that synchronises.
    scale_by_sqrt_dim=False drops the 1 / sqrt(D) on the squared distance (hacky_sigmoid_l2's form, loss.py:36-42)."""

    def __init__(self, temp=10.0, shift=1.0, scale_by_sqrt_dim=True):
        self._initial = (float(temp), float(shift))
        self.scale_by_sqrt_dim = bool(scale_by_sqrt_dim)
        self.params = None

    def bind(self, tensor):
        """adopt a device fp32 [2] tensor {temp, shift} (a view of a trainer's theta, say) as it is, values included"""
        if tensor.device.type != "cuda":
            raise _abi.GnfError("TunedSigmoidL2.params lives on a HIP device (no CPU path)")
        if tensor.dtype != torch.float32 or tuple(tensor.shape) != (2,) or not tensor.is_contiguous():
            raise ValueError(f"bind takes a contiguous float32 [2] tensor, got {tensor.dtype} {tuple(tensor.shape)}")
        self.params = tensor
        return self

    def on(self, device):
        """`.params`, created on `device` at first use"""
        if self.params is None:
            self.params = torch.tensor(self._initial, dtype=torch.float32, device=device)
        elif self.params.device != torch.device(device):
            raise _abi.GnfError(f"TunedSigmoidL2.params is on {self.params.device}, the embeddings on {device}")
        return self.params

    def values(self):
        """(temp, shift) as host floats: one 8-byte copy from the device once `.params` exists"""
        if self.params is None:
            return self._initial
        t, s = self.params.detach().cpu().tolist()
        return float(t), float(s)

    def __repr__(self):
        return "TunedSigmoidL2(temp={}, shift={}{})".format(*self.values(), "" if self.scale_by_sqrt_dim else ", unscaled")


def check_token(distance_fn, what):
    """NotImplementedError unless distance_fn is one of the four tokens; a fixed token's _distance_params, None for a
    TunedSigmoidL2"""
    if isinstance(distance_fn, TunedSigmoidL2):
        return None
    try:
        return _distance_params(distance_fn)
    except NotImplementedError:
        raise NotImplementedError(f"{what} supports distance_fn = scaled_hacky_sigmoid_l2 (loss.py:45-53), hacky_sigmoid_l2 "
                                  "(loss.py:36-42), sigmoid_l2(temp, shift) (loss.py:56-62) or TunedSigmoidL2(temp, shift)") \
            from None


def distance_desc(distance_fn, device, what="this call"):
    """_abi.GnfDistance of any of the four tokens (include/gnf_distance.h); the struct keeps no reference to a
    TunedSigmoidL2's tensor: hold the token while a launch may be pending"""
    fixed = check_token(distance_fn, what)
    if fixed is None:
        return _abi.GnfDistance(10.0, 1.0, int(distance_fn.scale_by_sqrt_dim), distance_fn.on(device).data_ptr())
    return _abi.GnfDistance(*fixed, None)


def _distance_params(distance_fn):
    """(temp, shift, scale_by_sqrt_dim) of a distance-function token"""
    if distance_fn is scaled_hacky_sigmoid_l2:
        return 10.0, 1.0, 1
    if distance_fn is hacky_sigmoid_l2:
        return 10.0, 1.0, 0
    if isinstance(distance_fn, sigmoid_l2):
        return distance_fn.temp, distance_fn.shift, 1
    raise NotImplementedError("binary_loss supports distance_fn = scaled_hacky_sigmoid_l2 (loss.py:45-53), hacky_sigmoid_l2 "
                              "(loss.py:36-42) or sigmoid_l2(temp, shift) (loss.py:56-62)")


def binary_loss(gnn_output, graph_phs, distance_fn=scaled_hacky_sigmoid_l2, use_soft_labels=False, epsilon=0.1, grad=None,
                abs_tol=0.5, max_nodes_per_graph=None, n_node_host=None, grad_params=False):
    """loss.py:162-188 with the counts of loss.py:88-116 and, on request, dL/dnodes: gnn_output.nodes are the embeddings,
    graph_phs gives the true topology and n_node.  Returns a dict of device tensors:
      "sum_loss", "mean_loss"     0-d float64: the masked cross-entropy summed over the ordered pairs (i, j), i != j, inside each
                                  graph, and that sum / (N^2 - N) with N the batch's node total (0 for N < 2)
      "loss_per_graph"            float64 [B]: the terms of sum_loss by graph
      "false_positive_pairs", "false_negative_pairs"  int64 [B]: ordered pairs with p - a > abs_tol / a - p > abs_tol against the
                                  hard label a (the helpers below halve them as loss.py does)
      "grad_nodes"                float32 [N, D], with grad="sum" (d sum_loss / d nodes) or grad="mean" (d mean_loss / d nodes)
      "grad_params"               float32 [2], with grad_params and a TunedSigmoidL2 token: d loss / d (temp, shift) of the
                                  loss `grad` names (sum_loss without grad).  grad_params=True allocates it; a device float32
                                  [2] tensor is written in place (a trainer's view of its gradient vector).  Any other token:
                                  ValueError.
    Every token goes through gnf_adj_loss_dist_f32 (a fixed token's bits are gnf_adj_loss_f32's: one kernel).
    The dense true_adj, pred_adj and ce_loss the reference also returns are NOT produced.  Per pair: p = sigmoid(u),
    ce = softplus(u_c) - t u_c with u_c = u clipped to +-log((1 - 1e-7) / 1e-7) - Keras' binary_crossentropy - and no gradient
    where the clip is active: a true edge whose endpoints lie far apart gets none, as in the reference.  t is the hard label,
    or with use_soft_labels 1 - epsilon / epsilon.  Duplicate edges count once (the reference counts their multiplicity; the
    datasets hold none); self loops and edges into another graph are ignored.
    The CSR comes from graphs.csr_of(graph_phs): on the result of decode_graphs no gnf_build_csr runs.  With
    max_nodes_per_graph (any upper bound on n_node, at most 65536) or n_node_host (the sizes as a host sequence) nothing is
    copied to the host and nothing synchronises, so the call can be captured; otherwise n_node is read once."""
    from .graphs import csr_desc, csr_of
    check_token(distance_fn, "binary_loss")    # (anything else raises before the device is looked at)
    want_gp = grad_params is not None and grad_params is not False
    if want_gp and not isinstance(distance_fn, TunedSigmoidL2):
        raise ValueError("grad_params needs distance_fn=TunedSigmoidL2(...): the other tokens' parameters are constants")
    if grad not in (None, "sum", "mean"):
        raise ValueError(f"grad={grad!r}: None, 'sum' or 'mean'")
    if not 0.0 <= float(epsilon) <= 0.5:
        raise ValueError(f"epsilon={epsilon}: a soft label lies in [0, 0.5]")
    if not float(abs_tol) >= 0.0:
        raise ValueError(f"abs_tol={abs_tol}")
    z = gnn_output.nodes
    n = int(z.shape[0])
    if int(graph_phs.nodes.shape[0]) != n:
        raise ValueError(f"gnn_output has {n} nodes, graph_phs {int(graph_phs.nodes.shape[0])}")
    lib = _abi.lib()
    dev = z.device
    if dev.type != "cuda" or graph_phs.senders.device.type != "cuda" or graph_phs.n_node.device.type != "cuda":
        raise _abi.GnfError("binary_loss runs on a HIP device only (no CPU path)")
    b = int(graph_phs.n_node.shape[0])
    cap = _node_bound(graph_phs, max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    z, _, d, ld = _abi.embeddings(z, "binary_loss")
    csr = csr_of(graph_phs)
    desc = csr_desc(graph_phs, csr, node_offsets=True)
    dist = distance_desc(distance_fn, dev, "binary_loss")
    # (the spec's own temp / shift / scale are gnf_adj_loss_f32's; this entry point reads the distance from `dist`)
    spec = _abi.GnfAdjLossSpec(dist.temp, dist.shift, dist.scale_by_sqrt_dim, int(bool(use_soft_labels)), float(epsilon),
                               float(abs_tol))
    sums2 = torch.empty(2, dtype=torch.float64, device=dev)
    out = {"loss_per_graph": torch.empty(b, dtype=torch.float64, device=dev),
           "false_positive_pairs": torch.empty(b, dtype=torch.int64, device=dev),
           "false_negative_pairs": torch.empty(b, dtype=torch.int64, device=dev)}
    g = torch.empty((n, d), dtype=torch.float32, device=dev) if grad else None
    pairs = float(n) * float(n) - float(n)
    grad_scale = 1.0 if grad != "mean" else (1.0 / pairs if n >= 2 else 0.0)
    gp = None
    if want_gp:
        gp = torch.empty(2, dtype=torch.float32, device=dev) if grad_params is True else grad_params
        if gp.device != dev or gp.dtype != torch.float32 or tuple(gp.shape) != (2,) or not gp.is_contiguous():
            raise ValueError("grad_params: True or a contiguous float32 [2] tensor on the embeddings' device")
    ws_bytes = lib.gnf_adj_loss_dist_workspace_bytes(b, n, cap)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_adj_loss_dist_f32(C.byref(desc), _abi.ptr(z), ld, d, cap, C.byref(spec), C.byref(dist),
                                             _abi.ptr(out["loss_per_graph"]), _abi.ptr(sums2),
                                             _abi.ptr(out["false_positive_pairs"]), _abi.ptr(out["false_negative_pairs"]),
                                             _abi.ptr(g), d, grad_scale, _abi.ptr(gp), _abi.ptr(ws), ws_bytes,
                                             _abi.stream_ptr(dev)), "gnf_adj_loss_dist_f32")
    out["sum_loss"], out["mean_loss"] = sums2[0], sums2[1]
    if grad:
        out["grad_nodes"] = g
    if want_gp:
        out["grad_params"] = gp
    return out


# ---- run_gnn_inference.py:107-163: which pairs are wrong, and with what score ------------------------------------------------
REPORT_CLASSES = {"correct": 1, "false_positive": 2, "false_negative": 3}
MAX_QUANTILES = _abi.GNF_SELECT_MAX_Q


def _quantile_list(quantiles):
    qs = [float(q) for q in quantiles]
    if len(qs) > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} quantiles per call, got {len(qs)}")
    for q in qs:
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"quantile {q}: in [0, 1]")
    return qs


def score_quantiles(score, cls, rowptr, seg_nodes, quantiles, edge_capacity=None):
    """gnf_score_select_f32 and the host side of its rule: per segment of the edge list (seg_nodes: device int32 node offsets)
    and for the classes 2 and 3, np.quantile's linear interpolation x[lo] + (h - lo) (x[hi] - x[lo]), h = (n - 1) q, of the
    class's scores - the order statistics x[lo], x[hi] selected exactly on the device, the interpolation two float64 torch
    ops on them.  Returns {"quantiles": float64 [S, 2, nq] (NaN where the class is empty), "count": int64 [S, 2], "stat":
    float32 [S, 2, nq, 2]}; nothing is read on the host."""
    qs = _quantile_list(quantiles)
    dev = rowptr.device
    if dev.type != "cuda":
        raise _abi.GnfError("score_quantiles runs on a HIP device only (no CPU path)")
    lib = _abi.lib()
    n_seg, nq = int(seg_nodes.shape[0]) - 1, len(qs)
    cap = int(score.shape[0]) if edge_capacity is None else min(int(edge_capacity), int(score.shape[0]))
    stat = torch.empty((n_seg, 2, nq, 2), dtype=torch.float32, device=dev)
    count = torch.empty((n_seg, 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_score_select_f32(_abi.ptr(score), _abi.ptr(cls), _abi.ptr(rowptr), _abi.ptr(seg_nodes), n_seg,
                                            int(rowptr.shape[0]) - 1, cap, (C.c_double * max(nq, 1))(*qs), nq, _abi.ptr(stat),
                                            _abi.ptr(count), _abi.stream_ptr(dev)), "gnf_score_select_f32")
    qv = torch.empty(nq, dtype=torch.float64, device=dev)
    for i, q in enumerate(qs):   # (fills, not a copy from the host: the call stays capturable)
        qv[i].fill_(q)
    h = (count - 1).clamp(min=0).to(torch.float64).unsqueeze(-1) * qv   # one fp64 product, as the device forms it
    x = stat.to(torch.float64)
    values = x[..., 0] + (h - torch.floor(h)) * (x[..., 1] - x[..., 0])
    return {"quantiles": values, "count": count, "stat": stat}


def reconstruction_report(gnn_output, graph_phs, distance_fn=scaled_hacky_sigmoid_l2, threshold=0.5,
                          quantiles=(0, .25, .5, .75, 1), per_graph=False, edge_capacity=None, max_nodes_per_graph=None,
                          n_node_host=None):
    """run_gnn_inference.py:107-163 on the device (include/gnf_adj_report.h): every ordered pair (sender s, receiver r), s != r,
    inside a graph that is a true edge of graph_phs or a predicted edge of gnn_output.nodes (score > threshold) becomes one
    entry of an edge list - receivers ascending, senders ascending within a receiver - with its class (1 correct, 2 false
    positive, 3 false negative: the reference's complete_mat weights) and its score, which has the bits of
    flow.pred_adj(...)[g][r, s] under the same distance_fn.  Returns a dict of device tensors:
      "graph"         GraphsTuple on gnn_output.nodes: the "complete" graph, int32 senders / receivers, n_edge, edges = the
                      classes as float32
      "cls", "score"  int32 / float32 [E]
      "csr"           graphs.Csr over (rowptr, senders): the receiver-sorted CSR of the list
      "class_pairs"   int64 [B, 3]: ordered pairs of each graph in class 1, 2, 3 ([:, 1:] are binary_loss' counts at 0.5)
      "totals"        int64 [4]: entries, class 1, class 2, class 3
      "fp_quantiles", "fn_quantiles"  float64 [nq] (per_graph: [B, nq]): np.quantile(scores of the class, quantiles) with
                      linear interpolation, NaN for an empty class
      "fp_count", "fn_count"          int64 0-d (per_graph: [B])
    Two departures from the reference: the diagonal is excluded (there every node counts as a false-positive self loop of
    score sigmoid(temp * shift)), and false negatives whose score is exactly 0 stay in the quantiles (np.nonzero drops them).
    Without edge_capacity the call reads totals[0] once, as decode_graphs does, and allocates exactly that many entries.  With
    edge_capacity and max_nodes_per_graph or n_node_host nothing is read on the host and the call can be captured; the edge
    tensors then have edge_capacity entries of which the first min(totals[0], edge_capacity) are valid, rowptr / n_edge /
    class_pairs / totals describe the untruncated list and the quantiles see the valid entries only.
    distance_fn: binary_loss' tokens, TunedSigmoidL2 included.  HIP only."""
    from .graphs import Csr, GraphsTuple, csr_desc, csr_of, node_offsets_of, seed_csr_cache
    check_token(distance_fn, "reconstruction_report")    # (anything else raises before the device is looked at)
    qs = _quantile_list(quantiles)
    if edge_capacity is not None and int(edge_capacity) < 0:
        raise ValueError(f"edge_capacity={edge_capacity}")
    z = gnn_output.nodes
    n = int(z.shape[0])
    if int(graph_phs.nodes.shape[0]) != n:
        raise ValueError(f"gnn_output has {n} nodes, graph_phs {int(graph_phs.nodes.shape[0])}")
    lib = _abi.lib()
    dev = z.device
    if dev.type != "cuda" or graph_phs.senders.device.type != "cuda" or graph_phs.n_node.device.type != "cuda":
        raise _abi.GnfError("reconstruction_report runs on a HIP device only (no CPU path)")
    b = int(graph_phs.n_node.shape[0])
    cap = _node_bound(graph_phs, max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    z, _, d, ld = _abi.embeddings(z, "reconstruction_report")
    desc = csr_desc(graph_phs, csr_of(graph_phs), node_offsets=True)
    dist = distance_desc(distance_fn, dev, "reconstruction_report")
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    n_edge = torch.empty(b, dtype=torch.int32, device=dev)
    class_pairs = torch.empty((b, 3), dtype=torch.int64, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    ws_bytes = lib.gnf_adj_report_workspace_bytes(b, n, cap)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_adj_report_count_f32(C.byref(desc), C.byref(dist), _abi.ptr(z), ld, d, cap, float(threshold),
                                                _abi.ptr(rowptr), _abi.ptr(n_edge), _abi.ptr(class_pairs), _abi.ptr(totals),
                                                _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), "gnf_adj_report_count_f32")
        exact = edge_capacity is None
        e = int(totals[0].item()) if exact else int(edge_capacity)
        senders = torch.empty(e, dtype=torch.int32, device=dev)
        receivers = torch.empty(e, dtype=torch.int32, device=dev)
        cls = torch.empty(e, dtype=torch.int32, device=dev)
        score = torch.empty(e, dtype=torch.float32, device=dev)
        _abi.check(lib.gnf_adj_report_fill(C.byref(dist), _abi.ptr(z), ld, d, b, n, cap, _abi.ptr(rowptr), e,
                                           _abi.ptr(senders), _abi.ptr(receivers), _abi.ptr(cls), _abi.ptr(score), _abi.ptr(ws),
                                           ws_bytes, _abi.stream_ptr(dev)), "gnf_adj_report_fill")
    if per_graph:
        seg = node_offsets_of(graph_phs)
    else:
        seg = torch.zeros(2, dtype=torch.int32, device=dev)
        seg[1:].fill_(n)
    sel = score_quantiles(score, cls, rowptr, seg, qs, e)
    qv, cnt = sel["quantiles"], sel["count"]
    if not per_graph:
        qv, cnt = qv[0], cnt[0]
    graph = GraphsTuple(nodes=gnn_output.nodes, edges=cls.to(torch.float32), receivers=receivers, senders=senders,
                        globals=torch.zeros(b, dtype=torch.float32, device=dev), n_node=graph_phs.n_node, n_edge=n_edge)
    csr = Csr(rowptr, senders, n, e)
    if exact:
        seed_csr_cache(graph, csr, by_sender=False)
    return {"graph": graph, "cls": cls, "score": score, "csr": csr, "class_pairs": class_pairs, "totals": totals,
            "fp_quantiles": qv[..., 0, :], "fn_quantiles": qv[..., 1, :], "fp_count": cnt[..., 0], "fn_count": cnt[..., 1]}


def _report_subgraph(report, classes):
    g = report["graph"]
    cls = report["cls"]
    e = int(cls.shape[0])
    keep = torch.arange(e, device=cls.device) < report["totals"][0]   # (a capacity above the total: the tail is unspecified)
    pick = torch.zeros_like(keep)
    for c in classes:
        pick |= cls == c
    idx = torch.nonzero(keep & pick).squeeze(1)
    n_edge = sum(report["class_pairs"][:, c - 1] for c in classes).to(torch.int32)
    sub = g.replace(senders=g.senders[idx], receivers=g.receivers[idx], edges=g.edges[idx], n_edge=n_edge)
    return {"graph": sub, "cls": cls[idx], "score": report["score"][idx]}


def predicted_graph(report):
    """run_gnn_inference.py:141-146: the predicted graph of a reconstruction_report - its entries of class 1 or 2, in order:
    flow.decode_graphs(..., self_loops=False)'s edge list at the report's threshold.  Returns {"graph", "cls", "score"}; an
    index selection on the device (its size is the one number read back).  n_edge is that of the untruncated list."""
    return _report_subgraph(report, (1, 2))


def error_graph(report, cls):
    """the entries of one class (1, 2, 3 or a name of REPORT_CLASSES) as predicted_graph returns them"""
    c = REPORT_CLASSES.get(cls, cls)
    if c not in (1, 2, 3):
        raise ValueError(f"cls={cls!r}: 1, 2, 3 or one of {sorted(REPORT_CLASSES)}")
    return _report_subgraph(report, (c,))


# ---- loss.py:88-116 over the result dict: the reference's figures are the ordered-pair counts halved -------------------------
def incorrect_edges_per_graph(result):
    """loss.py:88-95: wrong entries of each graph's block, halved, int32 [B]"""
    return ((result["false_positive_pairs"] + result["false_negative_pairs"]) // 2).to(torch.int32)


def false_positive_edges(result):
    """loss.py:104-106: 0-d float64"""
    return result["false_positive_pairs"].sum().to(torch.float64) / 2.0


def false_negative_edges(result):
    """loss.py:109-111: 0-d float64"""
    return result["false_negative_pairs"].sum().to(torch.float64) / 2.0


def total_incorrect_edges(result):
    """loss.py:114-116: 0-d float64"""
    return (result["false_positive_pairs"].sum() + result["false_negative_pairs"].sum()).to(torch.float64) / 2.0
