"""Log-prob assembly and sampling entry of the GRevNet drivers
(/root/reference/run_grevnet.py:290-311; same at train_grevnet_with_data.py:346-355, 397-414).

The two batch-wide reductions (sum(s) over all coupling half-steps, sum(z^2)) come out of
gnf_grevnet_f32 as device fp64 scalars; what is left here is scalar arithmetic, kept on the device
so that nothing synchronises until the caller reads a value.
"""
import ctypes as C
import math

import torch

from . import _abi
from .graph_stats import _node_bound

LN_2PI = math.log(2.0 * math.pi)


def gauss_sumsq(z):
    """sum_{n,j} z[n,j]^2 as a device fp64 0-d tensor (kernel D alone, gnf_gauss_sumsq_f32)."""
    lib = _abi.lib()
    if z.device.type != "cuda":
        raise _abi.GnfError("gauss_sumsq runs on a HIP device only (no CPU path)")
    z = z.to(torch.float32)
    if z.stride(1) != 1:
        z = z.contiguous()
    n, d = z.shape
    out = torch.empty(1, dtype=torch.float64, device=z.device)
    ws = torch.empty(8 * 1024, dtype=torch.uint8, device=z.device)
    with torch.cuda.device(z.device):
        _abi.check(lib.gnf_gauss_sumsq_f32(_abi.ptr(z), n, d, z.stride(0), _abi.ptr(out), _abi.ptr(ws),
                                           ws.numel(), _abi.stream_ptr(z.device)), "gnf_gauss_sumsq_f32")
    return out[0]


def forward_shard_sums(grevnet, graph, out=None):
    """Lean forward for throughput loops and multi-GPU shards: runs f and leaves
    [log_det_jacobian, sum(z^2), num_nodes] in a 3-element device fp64 tensor with NO further device
    work (that vector is exactly what one all-reduce sums over ranks; `log_prob_from_sums` finishes
    the arithmetic of run_grevnet.py:292-302 on the host).  Returns (z_nodes, sums3)."""
    n = graph.nodes.shape[0]
    if out is None:
        out = torch.zeros(3, dtype=torch.float64, device=graph.nodes.device)
        out[2] = float(n)
    z, _ = grevnet._run(graph, _abi.GNF_FORWARD, out)
    grevnet.last_sums = out
    return z, out


def log_prob_from_sums(sums3, d):
    """Host arithmetic of run_grevnet.py:292-302 on (all-reduced) [logdet, sum z^2, N] (python floats)."""
    logdet, sumsq, n = float(sums3[0]), float(sums3[1]), float(sums3[2])
    log_prob_zs = -0.5 * sumsq - 0.5 * d * LN_2PI * n
    log_prob_xs = log_prob_zs + logdet
    return {"log_prob_zs": log_prob_zs, "log_det_jacobian": logdet, "log_prob_xs": log_prob_xs,
            "total_loss": -log_prob_xs, "num_nodes": n, "loss_per_node": -log_prob_xs / n,
            "log_prob_xs_per_node": log_prob_xs / n, "log_prob_zs_per_node": log_prob_zs / n,
            "log_det_jacobian_per_node": logdet / n}


def log_prob_terms(grevnet, graph):
    """run_grevnet.py:290-302.  Returns a dict of 0-d device tensors (fp64 internally; the `*_f32`
    entries are the fp32 scalars the TF graph would log) plus the transformed graph:
      log_prob_zs = sum_n MVN(0,I).log_prob(z_n) = -0.5*sum(z^2) - D/2*ln(2pi)*N
      log_prob_xs = log_prob_zs + log_det_jacobian ; total_loss = -log_prob_xs ; *_per_node = * / sum(n_node)
    """
    z_graph, _ = grevnet(graph, inverse=True)
    sums = grevnet.last_sums                      # device fp64 [2]: logdet, sum z^2
    n, d = z_graph.nodes.shape
    logdet = sums[0]
    log_prob_zs = -0.5 * sums[1] - 0.5 * d * LN_2PI * n
    log_prob_xs = log_prob_zs + logdet
    num_nodes = float(n)                          # tf.cast(tf.reduce_sum(n_node), tf.float32)
    out = {
        "z_graph": z_graph,
        "log_det_jacobian": logdet,
        "log_prob_zs": log_prob_zs,
        "log_prob_xs": log_prob_xs,
        "total_loss": -log_prob_xs,
        "num_nodes": num_nodes,
        "loss_per_node": -log_prob_xs / num_nodes,
        "log_prob_xs_per_node": log_prob_xs / num_nodes,
        "log_prob_zs_per_node": log_prob_zs / num_nodes,
        "log_det_jacobian_per_node": logdet / num_nodes,
        # the three batch-wide sums a multi-GPU shard all-reduces
        "shard_sums": torch.stack([log_prob_zs, logdet, torch.tensor(num_nodes, dtype=torch.float64,
                                                                     device=sums.device)]),
    }
    return out


def log_prob_per_graph(grevnet, graph):
    """log p(G_g) for every graph of the batch from ONE forward pass (GRevNet.f_per_graph).  [B] device fp64 tensors:
      log_det_jacobian[g], log_prob_zs[g] = -0.5 * sum_{n in g} |z_n|^2 - n_g * D/2 * ln(2 pi), log_prob_xs = their sum,
      num_nodes[g], log_prob_xs_per_node[g] (an empty graph: 0, not NaN);
    plus z_graph and, under "batch", the scalars log_prob_terms returns - from the same call.  With batch norm the
    bijectors use the moments of the whole batch, so the values differ from those of single-graph calls: they are the
    terms of THIS batch's log-likelihood, and they add up to it."""
    z_graph, logdet = grevnet.f_per_graph(graph)
    gs = grevnet.last_graph_sums
    n, d = z_graph.nodes.shape
    dev = z_graph.nodes.device
    num = graph.n_node.to(device=dev, dtype=torch.float64)
    log_prob_zs = -0.5 * gs[:, 1] - 0.5 * d * LN_2PI * num
    log_prob_xs = log_prob_zs + logdet
    sums = grevnet.last_sums
    b_zs = -0.5 * sums[1] - 0.5 * d * LN_2PI * n
    b_xs = b_zs + sums[0]
    nn = float(n)
    batch = {"log_det_jacobian": sums[0], "log_prob_zs": b_zs, "log_prob_xs": b_xs, "total_loss": -b_xs, "num_nodes": nn,
             "loss_per_node": -b_xs / nn if n else b_xs * 0.0, "log_prob_xs_per_node": b_xs / nn if n else b_xs * 0.0,
             "log_prob_zs_per_node": b_zs / nn if n else b_zs * 0.0,
             "log_det_jacobian_per_node": sums[0] / nn if n else sums[0] * 0.0}
    return {"z_graph": z_graph, "log_det_jacobian": logdet, "log_prob_zs": log_prob_zs, "log_prob_xs": log_prob_xs,
            "num_nodes": num, "log_prob_xs_per_node": log_prob_xs / torch.clamp(num, min=1.0), "batch": batch}


def sample(grevnet, graph, generator=None):
    """run_grevnet.py:304-311: z ~ N(0, I) of shape [sum(n_node), D]; x = grevnet(graph.replace(nodes=z),
    inverse=False).nodes; also MVN.log_prob(z) per node.  torch.randn is the sampler."""
    n, d = graph.nodes.shape
    z = torch.randn(n, d, dtype=torch.float32, device=graph.nodes.device, generator=generator)
    sample_log_prob = -0.5 * (z.double() ** 2).sum(dim=1) - 0.5 * d * LN_2PI
    top = grevnet(graph.replace(nodes=z), inverse=False)
    return {"sample": z, "sample_log_prob": sample_log_prob, "grevnet_top": top, "grevnet_top_nodes": top.nodes}


def sample_per_graph(grevnet, graph, generator=None):
    """sample, with the flow's own density of every graph it generates from the same inverse pass (GRevNet.g_per_graph):
    what sample returns (same generator state: the same z, the same x bit for bit) plus [B] device fp64 tensors
      log_det_jacobian[g] = log|det dg/dz| of graph g's block, log_prob_zs[g] = -0.5 * sum_{n in g} |z_n|^2 - n_g * D/2 * ln(2 pi)
      (sum z^2 from the library call), log_prob_xs = log_prob_zs - log_det_jacobian, num_nodes[g],
      log_prob_xs_per_node[g] (an empty graph: 0, not NaN).
    The bijectors of g use the moving statistics: a graph's values do not depend on the rest of the batch."""
    n, d = graph.nodes.shape
    z = torch.randn(n, d, dtype=torch.float32, device=graph.nodes.device, generator=generator)
    sample_log_prob = -0.5 * (z.double() ** 2).sum(dim=1) - 0.5 * d * LN_2PI
    out = {"sample": z, "sample_log_prob": sample_log_prob}
    out.update(inverse_per_graph(grevnet, graph.replace(nodes=z)))
    return out


PER_GRAPH_KEYS = ("log_det_jacobian", "log_prob_zs", "log_prob_xs", "num_nodes", "log_prob_xs_per_node")


def inverse_per_graph(grevnet, z_graph):
    """x = g(z) of given latent rows with the five per-graph tensors of sample_per_graph (PER_GRAPH_KEYS) from the same
    pass, plus "grevnet_top" / "grevnet_top_nodes" as sample names them."""
    top, logdet = grevnet.g_per_graph(z_graph)
    gs = grevnet.last_graph_sums
    d = z_graph.nodes.shape[1]
    num = z_graph.n_node.to(device=gs.device, dtype=torch.float64)
    log_prob_zs = -0.5 * gs[:, 1] - 0.5 * d * LN_2PI * num
    log_prob_xs = log_prob_zs - logdet
    return {"grevnet_top": top, "grevnet_top_nodes": top.nodes, "log_det_jacobian": logdet, "log_prob_zs": log_prob_zs,
            "log_prob_xs": log_prob_xs, "num_nodes": num, "log_prob_xs_per_node": log_prob_xs / torch.clamp(num, min=1.0)}


def scaled_hacky_sigmoid_l2(*_a, **_k):
    """Token for the distance function of loss.py:45-53 (the only one pred_adj is used with on this
    path); the arithmetic runs inside gnf_pred_adj_dist_f32."""
    raise NotImplementedError("token only: pass it as distance_fn to pred_adj")


def pred_adj(gnn_output, distance_fn=scaled_hacky_sigmoid_l2, max_nodes_per_graph=None):
    """loss.py:154-159 for the sampling path (train_grevnet_with_data.py:415-416): edge probabilities
    sigmoid(10 * (1 - ||z_i - z_j||^2 / sqrt(D))) between the nodes of each graph, zero diagonal.  The
    reference returns a dense block-diagonal-masked [N, N] matrix; this returns the list of per-graph
    [n_g, n_g] blocks (views of one device buffer), which is what its consumer slices out
    (train_grevnet_with_data.py:538-540).  `adjacency = block > 0.5` gives the sampled graphs.
    distance_fn: the default, or one of adj_loss' tokens - hacky_sigmoid_l2, sigmoid_l2(temp, shift), TunedSigmoidL2 - whose
    probabilities have the bits binary_loss scores.  Every token goes through gnf_pred_adj_dist_f32 (the default's bits are
    gnf_pred_adj_f32's: one kernel)."""
    from .adj_loss import check_token, distance_desc
    check_token(distance_fn, "pred_adj")   # (anything else raises before the device is looked at)
    lib = _abi.lib()
    if gnn_output.nodes.device.type != "cuda":
        raise _abi.GnfError("pred_adj runs on a HIP device only (no CPU path)")
    z, _, d, ld = _abi.embeddings(gnn_output.nodes, "pred_adj")
    n_node_host = gnn_output.n_node.cpu().tolist()          # sizes the output (the reference syncs here too)
    b = len(n_node_host)
    total = sum(n * n for n in n_node_host)
    largest = max(n_node_host) if b else 0
    cap = int(max_nodes_per_graph) if max_nodes_per_graph is not None else largest
    if cap < largest:   # the launch covers `cap` rows per graph: a smaller bound would leave blocks unwritten
        raise ValueError(f"max_nodes_per_graph={cap} is below the largest graph of the batch ({largest} nodes)")
    dev = z.device
    out = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    off = torch.empty(b + 1, dtype=torch.int64, device=dev)
    ws_bytes = lib.gnf_pred_adj_workspace_bytes(b)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    nn = gnn_output.n_node.to(torch.int32).contiguous()
    dist = distance_desc(distance_fn, dev, "pred_adj")
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_pred_adj_dist_f32(C.byref(dist), _abi.ptr(z), ld, d, _abi.ptr(nn), b, cap, _abi.ptr(out),
                                             _abi.ptr(off), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)),
                   "gnf_pred_adj_dist_f32")
    blocks, o = [], 0
    for n in n_node_host:
        blocks.append(out[o:o + n * n].view(n, n))
        o += n * n
    return blocks


def decode_graphs(gnn_output, threshold=0.5, self_loops=False, edge_capacity=None, n_node_host=None,
                  distance_fn=scaled_hacky_sigmoid_l2, max_nodes_per_graph=None):
    """The graphs the sampling path generates (generate_graphs.py:68-78, train_grevnet_with_data.py:532-540: `pred_adj >
    0.5`, one graph per block), as device edge lists: edge (sender = j, receiver = i) of graph g exists iff
    pred_adj(gnn_output)[g][i, j] > threshold - the same fp32 arithmetic, bit for bit, without the dense blocks
    (gnf_adj_edges_count_dist_f32 / gnf_adj_edges_fill).  The diagonal is no edge unless self_loops=True; then every node
    has its self loop whatever the threshold (the convention of the flow's datasets).  Returns a dict:
      "graph"        GraphsTuple: the input's nodes and n_node, int32 senders / receivers (batch-wide node ids, receivers
                     ascending, senders ascending within a receiver) and n_edge, zero edges / globals as
                     data_dicts_to_graphs_tuple makes them
      "csr"          graphs.Csr over (rowptr, senders): the receiver-sorted CSR of that edge list and, the edge set being
                     exactly symmetric, its by-sender transpose as well
      "total_edges"  0-d device int64
    Without edge_capacity the call reads total_edges once (an 8-byte copy, its only synchronisation when n_node_host or
    max_nodes_per_graph says how large the graphs are; otherwise n_node is read from the device first, as pred_adj does),
    allocates exactly that many edges and seeds csr_of's cache for both orientations: a GRevNet call or a trainer step on
    result["graph"] launches no gnf_build_csr.
    With edge_capacity (and n_node_host, a host sequence of the graphs' sizes, or max_nodes_per_graph) nothing is copied to
    the host and nothing synchronises, so the call can be captured into a hipGraph.  The edge tensors (and "graph".edges)
    then have edge_capacity entries of which only the first min(total_edges, edge_capacity) are valid - the rest is
    unspecified - and rowptr / n_edge / "csr" describe the untruncated edge list: check total_edges <= edge_capacity before
    using them.  The CSR cache is not seeded in this mode.
    distance_fn: as for pred_adj."""
    from .adj_loss import check_token, distance_desc
    from .graphs import Csr, GraphsTuple, seed_csr_cache
    check_token(distance_fn, "decode_graphs")   # (anything else raises before the device is looked at)
    lib = _abi.lib()
    dev = gnn_output.nodes.device
    if dev.type != "cuda":
        raise _abi.GnfError("decode_graphs runs on a HIP device only (no CPU path)")
    z, n, d, ld = _abi.embeddings(gnn_output.nodes, "decode_graphs")
    b = int(gnn_output.n_node.shape[0])
    cap = _node_bound(gnn_output, max_nodes_per_graph, n_node_host, 2 ** 31 - 1)
    nn = gnn_output.n_node.to(device=dev, dtype=torch.int32).contiguous()
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    n_edge = torch.empty(b, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, cap)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    dist = distance_desc(distance_fn, dev, "decode_graphs")
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_adj_edges_count_dist_f32(C.byref(dist), _abi.ptr(z), ld, d, _abi.ptr(nn), b, n, cap,
                                                    float(threshold), int(bool(self_loops)), _abi.ptr(rowptr),
                                                    _abi.ptr(n_edge), _abi.ptr(total), _abi.ptr(ws), ws_bytes,
                                                    _abi.stream_ptr(dev)), "gnf_adj_edges_count_dist_f32")
        exact = edge_capacity is None
        e = int(total.item()) if exact else int(edge_capacity)
        senders = torch.empty(e, dtype=torch.int32, device=dev)
        receivers = torch.empty(e, dtype=torch.int32, device=dev)
        _abi.check(lib.gnf_adj_edges_fill(b, n, cap, _abi.ptr(rowptr), e, _abi.ptr(senders), _abi.ptr(receivers),
                                          _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), "gnf_adj_edges_fill")
    graph = GraphsTuple(nodes=gnn_output.nodes, edges=torch.zeros(e, dtype=torch.float32, device=dev), receivers=receivers,
                        senders=senders, globals=torch.zeros(b, dtype=torch.float32, device=dev), n_node=gnn_output.n_node,
                        n_edge=n_edge)
    csr = Csr(rowptr, senders, n, e)
    if exact:
        seed_csr_cache(graph, csr, by_sender=False)
        seed_csr_cache(graph, csr, by_sender=True)
    return {"graph": graph, "csr": csr, "total_edges": total[0]}


def generate_graphs(grevnet, shell_graph, generator=None, threshold=0.5, self_loops=False,
                    distance_fn=scaled_hacky_sigmoid_l2, log_prob=False, keep=None):
    """generate_graphs.py:57-84 / train_grevnet_with_data.py:526-540 in one call: sample z ~ N(0, I) on shell_graph's
    topology, run the flow in reverse, decode the embeddings to graphs (decode_graphs, exact-size mode).  Returns what
    decode_graphs returns, what sample returns, and "sample_log_prob_per_graph": the mean of sample_log_prob over each
    graph's nodes (generate_graphs.py:76; device fp64 [B], 0 for a graph without nodes).  distance_fn: the function the
    encoder whose embeddings the flow models was trained against (decode_graphs' argument).  log_prob=True samples
    through sample_per_graph instead - the same graphs, edge lists and sample_log_prob_per_graph for the same generator
    state - and adds its five [B] tensors (PER_GRAPH_KEYS): the flow's own density of each generated graph.
    keep ("largest_component", "non_isolated" or a mask: graph_stats.keep_subgraphs' argument) adds "kept", the result of
    keep_subgraphs(result["graph"], keep, self_loops=self_loops) - the generated batch reduced to the nodes to keep, all B
    graphs still in place; every other key is what a call without it returns.  None launches nothing more."""
    out = (sample_per_graph if log_prob else sample)(grevnet, shell_graph, generator=generator)
    top = out["grevnet_top"]
    res = decode_graphs(top, threshold=threshold, self_loops=self_loops, distance_fn=distance_fn)
    dev = top.nodes.device
    nn = shell_graph.n_node.to(device=dev, dtype=torch.int64)
    b = int(nn.shape[0])
    gid = torch.repeat_interleave(torch.arange(b, device=dev), nn, output_size=int(top.nodes.shape[0]))
    sums = torch.zeros(b, dtype=torch.float64, device=dev).index_add_(0, gid, out["sample_log_prob"])
    res.update(out)
    res["sample_log_prob_per_graph"] = sums / torch.clamp(nn, min=1).to(torch.float64)
    if keep is not None:
        from .graph_stats import keep_subgraphs
        res["kept"] = keep_subgraphs(res["graph"], keep, self_loops=self_loops)
    return res
