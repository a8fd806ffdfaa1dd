"""The sampled triplet loss of the encoder: loss.py's triplet_loss (loss.py:221-270, run_gnn.py --loss_type triplet) and the
gradient of its sum with respect to the embeddings, on the device (gnf_triplet_loss_f32, include/gnf_triplet_loss.h).

For node i and each of L = num_sampling_loops rounds the reference draws a positive j+ from i's out-edges (by multiplicity, a
self loop included) and a negative j- uniformly from the other nodes of i's graph without an edge i -> j, scores both pairs
with distance_fn (the diagonal scores 0) and adds triplet_loss_fn(p, q) to unreduced_loss[i].  It does so on dense [N, N]
true_adj / inv_true_adj / distances matrices; here sampling, scoring, loss and gradient read the sender-grouped CSR of the
true batch and need O(N * L) memory.  HIP only: CPU tensors raise GnfError.

Departures from the reference (the header states them in full):
 1. the random stream: a 32-bit draw r picks candidate (r * cnt) >> 32 of cnt; r comes from `draws` (uint32 [L, 2, N] on the
    device, [l, 0, i] positive, [l, 1, i] negative; an int32 / int64 tensor of values in [0, 2^32) is accepted) or from the
    header's hash of (seed, l, which, i); positives in edge order of the row, negatives in ascending node order;
 2. edges that leave i's graph are ignored, as in binary_loss;
 3. a node without a positive or without a negative candidate has terms of 0 without gradient, counted in "skipped_terms";
    so is a relative_loss term whose p + q == 0;
 4. self_loops="keep" is the reference, "skip" makes self loops non-candidates;
 5. the trainer's total loss is the SUM of unreduced_loss over the nodes (run_gnn.py:270 adds a sum_loss its triplet branch
    never defines);
 6. no dense pred_adj is returned: flow.pred_adj provides it, and the edge-error figures come from one
    binary_loss(..., grad=None) call, counted inside graphs.
"""
import ctypes as C

import torch

from . import _abi
from .adj_loss import TunedSigmoidL2, _distance_params, hacky_sigmoid_l2, sigmoid_l2
from .flow import scaled_hacky_sigmoid_l2
from .graph_stats import _node_bound

MAX_NODES_PER_GRAPH = 65536
MAX_SAMPLING_LOOPS = 64
RESULT_KEYS = ("sum_loss", "mean_loss", "loss_per_node", "loss_per_graph", "skipped_terms")


def _token(name, doc):
    def fn(*_a, **_k):
        raise NotImplementedError("token only: pass it as distance_fn to triplet_loss")
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = doc
    return fn


l2 = _token("l2", "Token for loss.py:210-214, the squared distance ||z_i - z_j||^2.")
dot = _token("dot", "Token for loss.py:217-218, the dot product z_i . z_j.")
exp_l2 = _token("exp_l2", "Token for loss.py:13-18, exp(-||z_i - z_j||^2).")
hacky_cauchy_l2 = _token("hacky_cauchy_l2", "Token for loss.py:27-33, atan(-(||z_i - z_j||^2 - 4)) / pi + 0.5.")
sigmoid_dot = _token("sigmoid_dot", "Token for loss.py:21-24, sigmoid(z_i . z_j - 0.5).")

_PLAIN = {l2: _abi.GNF_TRIPLET_L2, dot: _abi.GNF_TRIPLET_DOT, exp_l2: _abi.GNF_TRIPLET_EXP_L2,
          hacky_cauchy_l2: _abi.GNF_TRIPLET_HACKY_CAUCHY_L2, sigmoid_dot: _abi.GNF_TRIPLET_SIGMOID_DOT}


class margin_loss:
    """Token for loss.py:221-222 with its margin bound: max(margin - p + q, 0)."""

    def __init__(self, margin=0.65):
        self.margin = float(margin)

    def __repr__(self):
        return f"margin_loss(margin={self.margin})"


def relative_loss(*_a, **_k):
    """Token for loss.py:225-226, p / (p + q); the arithmetic runs inside gnf_triplet_loss_f32."""
    raise NotImplementedError("token only: pass it as triplet_loss_fn to triplet_loss")


def score_params(distance_fn):
    """(score kind, temp, shift, scale_by_sqrt_dim) of a score token"""
    if isinstance(distance_fn, TunedSigmoidL2):
        raise NotImplementedError("triplet_loss takes no TunedSigmoidL2: no parameter gradient is built under this loss")
    try:
        if distance_fn in _PLAIN:
            return _PLAIN[distance_fn], 0.0, 0.0, 0
    except TypeError:   # (an unhashable object is no token)
        pass
    try:
        temp, shift, by_sqrt = _distance_params(distance_fn)
    except NotImplementedError:
        raise NotImplementedError("triplet_loss supports distance_fn = l2, dot, exp_l2, hacky_cauchy_l2, sigmoid_dot "
                                  "(loss.py:13-33, 210-218), scaled_hacky_sigmoid_l2, hacky_sigmoid_l2 or "
                                  "sigmoid_l2(temp, shift) (loss.py:36-62)") from None
    return _abi.GNF_TRIPLET_SIGMOID_L2, temp, shift, by_sqrt


def loss_params(triplet_loss_fn):
    """(loss kind, margin) of a loss token; the class margin_loss stands for margin_loss()"""
    if triplet_loss_fn is margin_loss:
        triplet_loss_fn = margin_loss()
    if isinstance(triplet_loss_fn, margin_loss):
        return _abi.GNF_TRIPLET_MARGIN, triplet_loss_fn.margin
    if triplet_loss_fn is relative_loss:
        return _abi.GNF_TRIPLET_RELATIVE, 0.0
    raise NotImplementedError("triplet_loss supports triplet_loss_fn = margin_loss(margin) (loss.py:221-222) or relative_loss "
                              "(loss.py:225-226)")


def triplet_loss(gnn_output, graph_phs, distance_fn=l2, triplet_loss_fn=None, num_sampling_loops=8, seed=0, draws=None,
                 grad=None, self_loops="keep", max_nodes_per_graph=None, n_node_host=None, return_indices=False):
    """loss.py:242-270 and, on request, d sum / d nodes: gnn_output.nodes are the embeddings, graph_phs gives the true topology
    and n_node.  triplet_loss_fn defaults to margin_loss().  Returns a dict of device tensors:
      "loss_per_node"    float32 [N]: unreduced_loss, the sum of the node's L terms
      "loss_per_graph"   float64 [B]; "sum_loss" 0-d float64, their sum; "mean_loss" 0-d float64, sum_loss / kept terms (0 when
                         no term is kept)
      "skipped_terms"    int64 [B]: terms of nodes without a candidate (and relative_loss terms with p + q == 0)
      "grad_nodes"       float32 [N, D], with grad="sum" (d sum_loss / d nodes) or grad="mean" (d sum_loss / d nodes / (N L))
      "pos_index", "neg_index"   int32 [L, N] with return_indices: the chosen nodes, batch-global, -1 where a term is skipped
    grad="mean" scales by a host constant, 1 / (N L); mean_loss divides by the kept terms, which only the device knows.
    With max_nodes_per_graph (any upper bound on n_node, at most 65536) or n_node_host nothing is copied to the host and
    nothing synchronises, so the call can be captured; `seed` is then fixed in the capture, `draws` is read at replay."""
    from .graphs import csr_desc, csr_of
    kind, temp, shift, by_sqrt = score_params(distance_fn)
    loss_kind, margin = loss_params(margin_loss() if triplet_loss_fn is None else triplet_loss_fn)
    if grad not in (None, "sum", "mean"):
        raise ValueError(f"grad={grad!r}: None, 'sum' or 'mean'")
    if self_loops not in ("keep", "skip"):
        raise ValueError(f"self_loops={self_loops!r}: 'keep' or 'skip'")
    loops = int(num_sampling_loops)
    if not 1 <= loops <= MAX_SAMPLING_LOOPS:
        raise ValueError(f"num_sampling_loops={num_sampling_loops}: 1 to {MAX_SAMPLING_LOOPS}")
    z = gnn_output.nodes
    n = int(z.shape[0])
    if int(graph_phs.nodes.shape[0]) != n:
        raise ValueError(f"gnn_output has {n} nodes, graph_phs {int(graph_phs.nodes.shape[0])}")
    dev = z.device
    if dev.type != "cuda" or graph_phs.senders.device.type != "cuda" or graph_phs.n_node.device.type != "cuda":
        raise _abi.GnfError("triplet_loss runs on a HIP device only (no CPU path)")
    lib = _abi.lib()
    if n * 2 * loops > 2 ** 31 - 1:
        raise ValueError(f"{n} nodes with num_sampling_loops={loops}: N * 2 L must fit int32")
    b = int(graph_phs.n_node.shape[0])
    cap = _node_bound(graph_phs, max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    z, _, d, ld = _abi.embeddings(z, "triplet_loss")
    if draws is not None:
        if draws.device != dev or tuple(draws.shape) != (loops, 2, n):
            raise ValueError(f"draws: a [{loops}, 2, {n}] tensor on the embeddings' device, got {tuple(draws.shape)} on {draws.device}")
        if draws.dtype in (torch.int64, torch.int32):
            draws = draws.to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.uint32)
        if draws.dtype != torch.uint32:
            raise ValueError(f"draws: uint32 (or int32 / int64 values in [0, 2^32)), got {draws.dtype}")
        draws = draws.contiguous()
    csr = csr_of(graph_phs, by_sender=True)
    desc = csr_desc(graph_phs, csr, node_offsets=True)
    spec = _abi.GnfTripletSpec(kind, temp, shift, by_sqrt, loss_kind, margin, loops, 1 if self_loops == "skip" else 0,
                               int(seed) & 0xFFFFFFFFFFFFFFFF)
    sums2 = torch.empty(2, dtype=torch.float64, device=dev)
    out = {"loss_per_node": torch.empty(n, dtype=torch.float32, device=dev),
           "loss_per_graph": torch.empty(b, dtype=torch.float64, device=dev),
           "skipped_terms": torch.empty(b, dtype=torch.int64, device=dev)}
    pos = torch.empty((loops, n), dtype=torch.int32, device=dev) if return_indices else None
    neg = torch.empty((loops, n), dtype=torch.int32, device=dev) if return_indices else None
    g = torch.empty((n, d), dtype=torch.float32, device=dev) if grad else None
    grad_scale = 1.0 if grad != "mean" else (1.0 / (float(n) * loops) if n else 0.0)
    ws_bytes = lib.gnf_triplet_loss_workspace_bytes(b, n, loops)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_triplet_loss_f32(C.byref(desc), _abi.ptr(z), ld, d, cap, C.byref(spec), _abi.ptr(draws),
                                            _abi.ptr(out["loss_per_node"]), _abi.ptr(out["loss_per_graph"]), _abi.ptr(sums2),
                                            _abi.ptr(out["skipped_terms"]), _abi.ptr(pos), _abi.ptr(neg), _abi.ptr(g), d,
                                            grad_scale, _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), "gnf_triplet_loss_f32")
    out["sum_loss"], out["mean_loss"] = sums2[0], sums2[1]
    if grad:
        out["grad_nodes"] = g
    if return_indices:
        out["pos_index"], out["neg_index"] = pos, neg
    return out


__all__ = ["triplet_loss", "l2", "dot", "exp_l2", "hacky_cauchy_l2", "sigmoid_dot", "scaled_hacky_sigmoid_l2",
           "hacky_sigmoid_l2", "sigmoid_l2", "margin_loss", "relative_loss", "score_params", "loss_params"]
