"""Scoring generated graphs on the device: the step after flow.generate_graphs.

GraphRNN-style evaluation compares generated graphs to held-out ones by the MMD of their degree and clustering-coefficient
histograms.  The reference stops at pickling the graphs (generate_graphs.py:68-84); here the edge lists never leave the
device: graph_stats (gnf_graph_stats) turns a batch into per-node degrees / triangle counts and per-graph histograms,
hist_mmd (gnf_hist_mmd_f64) reduces two histogram sets to one MMD^2, evaluate_generated does both for two batches.
The third statistic of that evaluation, orbit counts: graph_orbits (gnf_graph_orbits) counts the 15 node orbits of the
graphlets on 2, 3 and 4 nodes, orbit_mmd (gnf_vec_mmd_i64) is the MMD^2 of two sets of per-graph mean orbit vectors under a
Gaussian kernel; evaluate_generated(..., orbits=True) adds it.
The fourth statistic, the one reported since GRAN: graph_spectra (gnf_graph_spectra) computes the eigenvalues of every
graph's normalised Laplacian and their per-graph histogram, spectral_mmd is hist_mmd on those histograms under the
total-variation kernel; evaluate_generated(..., spectral=True) adds it.
Before any of them: graph_components (gnf_graph_components) says whether a generated graph is one graph at all - `pred_adj >
threshold` decides every pair of nodes on its own - and keep_subgraphs (gnf_graph_subgraph_count / _fill) reduces a batch to
its largest components, its non-isolated nodes or a mask, as a batch everything here and the flow accept as it is;
evaluate_generated(..., keep=...) does that to the generated batch first.
And what none of the four can see - a sampler that replays its training set scores a perfect MMD: graph_hashes
(gnf_graph_hashes) gives every graph a Weisfeiler-Lehman hash that does not depend on the node numbering, uniqueness_novelty
(gnf_graph_hash_match) turns two hash sets into the shares of generated graphs that repeat no earlier generated graph and no
training graph; evaluate_generated(..., train=...) adds them.
Every graph is read as undirected and simple (self loops ignored, duplicates once, one direction is enough).  HIP only:
CPU tensors raise GnfError.
"""
import ctypes as C

import torch

from . import _abi

_KERNELS = {"gaussian_emd": _abi.GNF_MMD_GAUSSIAN_EMD, "gaussian_tv": _abi.GNF_MMD_GAUSSIAN_TV}
MAX_NODES_PER_GRAPH = 65536   # a node's triangle count must fit int32
STATS_KEYS = ("degree", "triangles", "clustering", "degree_hist", "clustering_hist", "n_edges", "n_triangles")
ORBIT_MAX_NODES_PER_GRAPH = 8192   # gnf_graph_orbits: the cost per node grows with n_g + d_i d_mean
N_ORBITS = 15
ORBIT_KEYS = ("orbits", "orbit_sums", "orbit_mean", "n_node")
SPECTRA_MAX_NODES_PER_GRAPH = 2048   # gnf_graph_spectra: a dense eigenvalue solver, n^3 work per graph
SPECTRA_LDS_NODES = 139              # up to here a graph's matrix lives in LDS, above it in the workspace
SPECTRA_SLOTS = 256                  # matrix slots of the workspace route
SPECTRA_KEYS = ("eigenvalues", "spectral_hist", "n_node")
COMPONENT_KEYS = ("component", "component_size", "n_components", "largest_component_size", "largest_component_root", "n_isolated")
WL_MAX_ITERATIONS = 64    # gnf_graph_hashes: refinement rounds
WL_LDS_NODES = 4096       # up to here a graph's colours live in LDS (one launch), above it in the workspace (one per round)
HASH_KEYS = ("hash", "node_colour", "n_edges", "n_node")
NOVELTY_KEYS = ("uniqueness", "novelty", "unique_novel", "first_in_generated", "match_in_training", "counts")
_KEEP_RULES = {"largest_component": _abi.GNF_KEEP_LARGEST_COMPONENT, "non_isolated": _abi.GNF_KEEP_NON_ISOLATED}


def _node_bound(graph, max_nodes_per_graph, n_node_host, limit):
    """Columns of the adjacency bitmap: max_nodes_per_graph, else the largest graph (n_node_host, else n_node read once)."""
    n = int(graph.nodes.shape[0])
    b = int(graph.n_node.shape[0])
    if n_node_host is not None:
        sizes = [int(v) for v in n_node_host]
        if len(sizes) != b or sum(sizes) != n:
            raise ValueError(f"n_node_host describes {len(sizes)} graphs / {sum(sizes)} nodes, the batch has {b} / {n}")
    elif max_nodes_per_graph is None:
        sizes = graph.n_node.cpu().tolist()
    else:
        sizes = None
    largest = (max(sizes) if sizes else 0) if sizes is not None else None
    cap = int(max_nodes_per_graph) if max_nodes_per_graph is not None else largest
    if largest is not None and cap < largest:   # the bitmap holds `cap` columns per row: a smaller bound would drop edges
        raise ValueError(f"max_nodes_per_graph={cap} is below the largest graph of the batch ({largest} nodes)")
    if cap > limit:
        raise ValueError(f"max_nodes_per_graph={cap} exceeds {limit}")
    return cap


def _call(dev, entry, sizes, args, query=None, ws=None):
    """One library call on dev's current stream: entry(*args, workspace, workspace bytes, stream), the workspace as
    `query` (entry + "_workspace_bytes" unless given) sizes it for `sizes`.  Returns the workspace; ws= passes on the one an
    earlier call left (gnf_graph_subgraph_fill reads what gnf_graph_subgraph_count wrote)."""
    lib = _abi.lib()
    ws_bytes = getattr(lib, query or entry + "_workspace_bytes")(*sizes)
    if ws is None:
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _abi.check(getattr(lib, entry)(*args, _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), entry)
    return ws


class _Batch:
    """A GraphsTuple as the batch entry points on the adjacency bitmap take it.  Three steps, so that every caller keeps its
    own argument checks where they stand between them: the constructor refuses a batch that is not on a HIP device and reads
    the sizes; bound() is the first step that may copy n_node to the host; call() is the first that may launch (csr_of:
    gnf_build_csr, unless the batch came from decode_graphs or keep_subgraphs)."""

    def __init__(self, name, graph):
        self.graph, self.dev = graph, graph.senders.device
        if self.dev.type != "cuda" or graph.n_node.device.type != "cuda":
            raise _abi.GnfError(f"{name} runs on a HIP device only (no CPU path)")
        self.n = int(graph.nodes.shape[0])
        self.b = int(graph.n_node.shape[0])

    def bound(self, max_nodes_per_graph, n_node_host, limit):
        self.cap = _node_bound(self.graph, max_nodes_per_graph, n_node_host, limit)
        return self.cap

    def call(self, entry, *args, query=None):
        """entry(csr with node offsets, max_nodes_per_graph, *args, workspace, workspace bytes, stream)"""
        from .graphs import csr_desc, csr_of
        csr = csr_of(self.graph)
        desc = csr_desc(self.graph, csr, node_offsets=True)
        return _call(self.dev, entry, (self.b, self.n, self.cap), (C.byref(desc), self.cap) + args, query)


def _mmd2(name, out5, what):
    """The biased V-statistic sum_AA / cnt_a^2 + sum_BB / cnt_b^2 - 2 sum_AB / (cnt_a cnt_b) of out5 = {sum AA, sum BB, sum AB,
    cnt_a, cnt_b} as a 0-d device tensor; reading the two counts is the one copy to the host."""
    cnt_a, cnt_b = out5[3:5].tolist()
    if cnt_a < 1 or cnt_b < 1:
        raise ValueError(f"{name}: {int(cnt_a)} / {int(cnt_b)} non-empty {what} in the two sets; both need one")
    return out5[0] / (out5[3] * out5[3]) + out5[1] / (out5[4] * out5[4]) - 2.0 * out5[2] / (out5[3] * out5[4])


def graph_stats(graph, max_nodes_per_graph=None, n_node_host=None, clustering_bins=100):
    """Degree and clustering statistics of every graph of a GraphsTuple, as a dict of device tensors:
      "degree", "triangles"   int32 [N]: neighbours of each node, triangles through it
      "clustering"            float64 [N]: 2 T / (d (d - 1)), 0 for d < 2
      "degree_hist"           int32 [B, max_nodes_per_graph]: nodes of graph g with degree d
      "clustering_hist"       int32 [B, clustering_bins]: bin 0 for d < 2, else min(bins - 1, (2 T bins) // (d (d - 1))) in
                              exact integers (c = 1 lands in the last bin)
      "n_edges", "n_triangles" int64 [B]
    The CSR comes from graphs.csr_of: on the result of decode_graphs / generate_graphs no gnf_build_csr runs.
    With max_nodes_per_graph (any upper bound on n_node) or n_node_host (the sizes as a host sequence) nothing is copied to
    the host and nothing synchronises, so the call can be captured; otherwise n_node is read once, as pred_adj does."""
    batch = _Batch("graph_stats", graph)
    dev, n, b = batch.dev, batch.n, batch.b
    bins = int(clustering_bins)
    cap = batch.bound(max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    if bins < 1:
        raise ValueError(f"clustering_bins={bins}")
    out = {"degree": torch.empty(n, dtype=torch.int32, device=dev),
           "triangles": torch.empty(n, dtype=torch.int32, device=dev),
           "degree_hist": torch.empty((b, cap), dtype=torch.int32, device=dev),
           "clustering_hist": torch.empty((b, bins), dtype=torch.int32, device=dev),
           "n_edges": torch.empty(b, dtype=torch.int64, device=dev),
           "n_triangles": torch.empty(b, dtype=torch.int64, device=dev)}
    batch.call("gnf_graph_stats", bins, *(_abi.ptr(out[k]) for k in ("degree", "triangles", "degree_hist", "clustering_hist",
                                                                        "n_edges", "n_triangles")))
    d = out["degree"].to(torch.float64)
    pairs = d * (d - 1.0)
    out["clustering"] = torch.where(pairs > 0, 2.0 * out["triangles"].to(torch.float64) / pairs.clamp(min=1.0),
                                    torch.zeros_like(pairs))
    return out


def _hist_mmd_sums(hists_a, hists_b, kernel, sigma, distance_scaling):
    if kernel not in _KERNELS:
        raise ValueError(f"kernel={kernel!r}: one of {sorted(_KERNELS)}")
    for h in (hists_a, hists_b):
        if not isinstance(h, torch.Tensor) or h.device.type != "cuda":
            raise _abi.GnfError("hist_mmd runs on a HIP device only (no CPU path)")
        if h.dim() != 2:
            raise ValueError(f"hist_mmd takes [rows, bins] histograms, got shape {tuple(h.shape)}")
    dev = hists_a.device
    ha = hists_a.to(torch.int32).contiguous()
    hb = hists_b.to(device=dev, dtype=torch.int32).contiguous()
    a, la = int(ha.shape[0]), int(ha.shape[1])
    b, lb = int(hb.shape[0]), int(hb.shape[1])
    out5 = torch.empty(5, dtype=torch.float64, device=dev)
    _call(dev, "gnf_hist_mmd_f64", (a, b), (_abi.ptr(ha), a, la, la, _abi.ptr(hb), b, lb, lb, _KERNELS[kernel], float(sigma),
                                            float(distance_scaling), _abi.ptr(out5)), query="gnf_hist_mmd_workspace_bytes")
    return out5


def hist_mmd(hists_a, hists_b, kernel="gaussian_emd", sigma=1.0, distance_scaling=1.0):
    """MMD^2 of two sets of histograms (int32 [a, La] and [b, Lb] on the device; the narrower set reads as zero-padded), as a
    0-d float64 device tensor: sum_AA / cnt_a^2 + sum_BB / cnt_b^2 - 2 sum_AB / (cnt_a cnt_b) with the Gaussian kernel
    exp(-W^2 / (2 sigma^2)) over W = the 1-D earth mover's distance of the normalised rows divided by distance_scaling
    ("gaussian_emd") or their total variation ("gaussian_tv") - the biased V-statistic, diagonals in, as in GraphRNN's
    evaluation.  All-zero rows (graphs without nodes) are left out.  Raises ValueError when a set has no other row: reading
    the two counts is the call's only copy to the host."""
    return _mmd2("hist_mmd", _hist_mmd_sums(hists_a, hists_b, kernel, sigma, distance_scaling), "histograms")


def graph_orbits(graph, max_nodes_per_graph=None, n_node_host=None):
    """Orbit counts of every graph of a GraphsTuple, as a dict of device tensors:
      "orbits"      int64 [N, 15]: induced connected subgraphs on 2, 3 and 4 nodes through each node, by the node's orbit
                    (Przulj's numbering, as ORCA: 0 edge, 1-2 path, 3 triangle, 4-5 4-path, 6-7 star, 8 4-cycle, 9-11 tailed
                    triangle, 12-13 chorded 4-cycle, 14 complete graph); column 0 is the degree, column 3 the triangles
      "orbit_sums"  int64 [B, 15]: the columns summed over each graph
      "orbit_mean"  float64 [B, 15]: orbit_sums / n_node, the graph's orbit vector; 0 for a graph without nodes
      "n_node"      int32 [B]: the batch's sizes (what orbit_mmd divides by)
    The CSR comes from graphs.csr_of: on the result of decode_graphs / generate_graphs no gnf_build_csr runs.  As for
    graph_stats, with max_nodes_per_graph (any upper bound on n_node, at most 8192) or n_node_host nothing is copied to the
    host and nothing synchronises, so the call can be captured; otherwise n_node is read once."""
    batch = _Batch("graph_orbits", graph)
    batch.bound(max_nodes_per_graph, n_node_host, ORBIT_MAX_NODES_PER_GRAPH)
    out = {"orbits": torch.empty((batch.n, N_ORBITS), dtype=torch.int64, device=batch.dev),
           "orbit_sums": torch.empty((batch.b, N_ORBITS), dtype=torch.int64, device=batch.dev)}
    batch.call("gnf_graph_orbits", _abi.ptr(out["orbits"]), N_ORBITS, _abi.ptr(out["orbit_sums"]))
    out["n_node"] = graph.n_node.to(torch.int32)
    out["orbit_mean"] = out["orbit_sums"].to(torch.float64) / out["n_node"].clamp(min=1).to(torch.float64).unsqueeze(1)
    return out


def _orbit_set(x, dev=None):
    """(orbit_sums int64 [rows, L] contiguous, n_node int32 [rows]) of a graph_orbits result or an (orbit_sums, n_node) pair"""
    sums, cnt = (x["orbit_sums"], x["n_node"]) if isinstance(x, dict) else x
    for v in (sums, cnt):
        if not isinstance(v, torch.Tensor) or v.device.type != "cuda":
            raise _abi.GnfError("orbit_mmd runs on a HIP device only (no CPU path)")
    if sums.dim() != 2 or cnt.dim() != 1 or int(cnt.shape[0]) != int(sums.shape[0]):
        raise ValueError(f"orbit_mmd takes [rows, L] sums with [rows] sizes, got {tuple(sums.shape)} and {tuple(cnt.shape)}")
    dev = sums.device if dev is None else dev
    return sums.to(device=dev, dtype=torch.int64).contiguous(), cnt.to(device=dev, dtype=torch.int32).contiguous()


def _orbit_mmd_sums(orbits_a, orbits_b, sigma):
    xa, ca = _orbit_set(orbits_a)
    dev = xa.device
    xb, cb = _orbit_set(orbits_b, dev)
    a, b, width = int(xa.shape[0]), int(xb.shape[0]), int(xa.shape[1])
    if int(xb.shape[1]) != width:
        raise ValueError(f"orbit_mmd: vectors of {width} and {int(xb.shape[1])} entries")
    out5 = torch.empty(5, dtype=torch.float64, device=dev)
    _call(dev, "gnf_vec_mmd_i64", (a, b), (_abi.ptr(xa), _abi.ptr(ca), a, width, _abi.ptr(xb), _abi.ptr(cb), b, width, width,
                                           float(sigma), _abi.ptr(out5)), query="gnf_vec_mmd_workspace_bytes")
    return out5


def orbit_mmd(orbits_a, orbits_b, sigma=30.0):
    """MMD^2 of the orbit vectors (orbit_sums / n_node, not normalised further) of two sets of graphs - two results of
    graph_orbits, or two (orbit_sums int64 [rows, L], n_node int32 [rows]) pairs on the device - under the Gaussian kernel
    exp(-|x - y|^2 / (2 sigma^2)), sigma = 30 as in GraphRNN's orbit evaluation: the same biased V-statistic as hist_mmd, as
    a 0-d float64 device tensor.  Graphs without nodes are left out.  Two identical sets give exactly 0.  Raises ValueError
    when a set has no other graph: reading the two counts is the call's only copy to the host."""
    return _mmd2("orbit_mmd", _orbit_mmd_sums(orbits_a, orbits_b, sigma), "graphs")


def graph_spectra(graph, max_nodes_per_graph=None, n_node_host=None, bins=200, lo=-1e-5, hi=2.0):
    """Normalised-Laplacian spectrum of every graph of a GraphsTuple, as a dict of device tensors:
      "eigenvalues"    float64 [N]: the eigenvalues of graph g, ascending, in the rows of its nodes.  L_ii = 1 (0 for an isolated
                       node), L_ij = -1 / sqrt(d_i d_j) for an edge: an isolated node contributes an eigenvalue 0
      "spectral_hist"  int32 [B, bins]: eigenvalue x counts in bin clamp(floor((x - lo) * bins / (hi - lo)), 0, bins - 1) - values
                       outside [lo, hi) land in the first / last bin, none is dropped; a row sums to n_node
      "n_node"         int32 [B]
    The defaults (200 bins over [-1e-5, 2]) are GRAN's setting.  The CSR comes from graphs.csr_of: on the result of
    decode_graphs / generate_graphs no gnf_build_csr runs.  As for graph_stats, with max_nodes_per_graph (any upper bound on
    n_node, at most 2048) or n_node_host nothing is copied to the host and nothing synchronises, so the call can be captured;
    otherwise n_node is read once.  Up to 139 nodes per graph the matrices live in LDS, above that in a workspace of
    min(B, 256) * max_nodes_per_graph^2 doubles."""
    batch = _Batch("graph_spectra", graph)
    bins = int(bins)
    batch.bound(max_nodes_per_graph, n_node_host, SPECTRA_MAX_NODES_PER_GRAPH)
    if bins < 1 or not float(hi) > float(lo):
        raise ValueError(f"bins={bins} lo={lo} hi={hi}")
    out = {"eigenvalues": torch.empty(batch.n, dtype=torch.float64, device=batch.dev),
           "spectral_hist": torch.empty((batch.b, bins), dtype=torch.int32, device=batch.dev)}
    batch.call("gnf_graph_spectra", _abi.ptr(out["eigenvalues"]), _abi.ptr(out["spectral_hist"]), bins, float(lo), float(hi))
    out["n_node"] = graph.n_node.to(torch.int32)
    return out


def spectral_mmd(a, b, sigma=1.0):
    """MMD^2 of the eigenvalue histograms of two sets of graphs - two results of graph_spectra, or two int32 [rows, bins]
    histogram tensors on the device - under the Gaussian kernel on the total variation of the normalised rows, sigma = 1 as
    in GRAN's evaluation: the estimator of hist_mmd(..., "gaussian_tv", sigma, 1.0) on the same entry point
    (gnf_hist_mmd_f64), a 0-d float64 device tensor.  Graphs without nodes are left out.  Two identical sets give exactly 0:
    gnf_hist_mmd_f64 adds a same-set block up from its upper triangle and the cross block row by row, so its three sums of
    two identical sets agree only to rounding; here every block is read off as the CROSS block of a call of its own - (a, a),
    (b, b), (a, b) - three sums formed in one order, equal bit for bit when the sets are.  Raises ValueError when a set has
    no other row: reading the two counts is the call's only copy to the host."""
    ha, hb = (x["spectral_hist"] if isinstance(x, dict) else x for x in (a, b))
    ab = _hist_mmd_sums(ha, hb, "gaussian_tv", sigma, 1.0)
    cnt_a, cnt_b = ab[3:5].tolist()
    if cnt_a < 1 or cnt_b < 1:
        raise ValueError(f"spectral_mmd: {int(cnt_a)} / {int(cnt_b)} non-empty histograms in the two sets; both need one")
    aa = _hist_mmd_sums(ha, ha, "gaussian_tv", sigma, 1.0)
    hb = hb.to(ha.device)
    bb = _hist_mmd_sums(hb, hb, "gaussian_tv", sigma, 1.0)
    return aa[2] / (ab[3] * ab[3]) + bb[2] / (ab[4] * ab[4]) - 2.0 * ab[2] / (ab[3] * ab[4])


def graph_components(graph, max_nodes_per_graph=None, n_node_host=None):
    """Connected components of every graph of a GraphsTuple (gnf_graph_components), as a dict of int32 device tensors:
      "component"               [N]: the batch-wide row of the smallest node of each node's component - canonical, whatever
                                the search order; a root is its own label
      "component_size"          [N]: the number of nodes of that component
      "n_components"            [B]: an isolated node is a component of size 1, a graph without nodes has 0
      "largest_component_size"  [B]
      "largest_component_root"  [B]: among the largest components the one with the smallest root; -1 for a graph without nodes
      "n_isolated"              [B]: nodes of degree 0
    The CSR comes from graphs.csr_of: on the result of decode_graphs / generate_graphs no gnf_build_csr runs.  As for
    graph_stats, with max_nodes_per_graph (any upper bound on n_node, at most 65536) or n_node_host nothing is copied to the
    host and nothing synchronises, so the call can be captured; otherwise n_node is read once.  A level-synchronous search:
    one pair of workgroup barriers per level, a path on n nodes costs up to n levels."""
    batch = _Batch("graph_components", graph)
    batch.bound(max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    out = {k: torch.empty(batch.n if k in COMPONENT_KEYS[:2] else batch.b, dtype=torch.int32, device=batch.dev)
           for k in COMPONENT_KEYS}
    batch.call("gnf_graph_components", *(_abi.ptr(out[k]) for k in COMPONENT_KEYS))
    return out


def keep_subgraphs(graph, keep="largest_component", self_loops=False, max_nodes_per_graph=None, n_node_host=None):
    """The batch that is left when only some nodes of every graph are kept (gnf_graph_subgraph_count / _fill): the subgraph of
    the simple undirected graph that the kept nodes induce, in decode_graphs' convention.
      keep   "largest_component" (ties: the component with the smallest node), "non_isolated" (degree > 0), or a bool /
             uint8 tensor [N], nonzero = keep
    Returns a dict:
      "graph"        GraphsTuple with all B graphs (one with nothing kept has n_node = 0, so per-graph tensors of the input
                     still line up): nodes = the input's rows in their old order (index_select), int32 senders / receivers
                     (both directions of every edge, receivers ascending, senders ascending within a receiver; the diagonal
                     only with self_loops=True, and then on every kept node), zero edges, the input's globals, new n_node /
                     n_edge
      "csr"          graphs.Csr over (rowptr, senders): the receiver-sorted CSR and, the edge set being symmetric, its
                     by-sender transpose; csr_of's cache is seeded for both, so a GRevNet call, a trainer step or one of the
                     scores on result["graph"] launches no gnf_build_csr
      "node_index"   int32 [N']: the old row of each new node      "new_id"  int32 [N]: the new row of each old node, or -1
      "total_nodes", "total_edges"   0-d device int64
    Exact-size mode only: the call reads N' and E' once (one 16-byte copy, its only synchronisation when max_nodes_per_graph
    or n_node_host says how large the graphs are) and allocates exactly that.  A capacity / capture mode, as decode_graphs
    has one, is out of scope here (the two entry points take capacities; this wrapper does not)."""
    from .graphs import Csr, GraphsTuple, seed_csr_cache
    batch = _Batch("keep_subgraphs", graph)
    dev, n, b = batch.dev, batch.n, batch.b
    mask = None
    if isinstance(keep, torch.Tensor):
        if keep.dim() != 1 or int(keep.shape[0]) != n or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"keep: a bool / uint8 tensor [{n}], got {keep.dtype} {tuple(keep.shape)}")
        if keep.device.type != "cuda":
            raise _abi.GnfError("keep_subgraphs runs on a HIP device only (no CPU path)")
        rule, mask = _abi.GNF_KEEP_MASK, keep.to(device=dev, dtype=torch.uint8).contiguous()
    elif keep in _KEEP_RULES:
        rule = _KEEP_RULES[keep]
    else:
        raise ValueError(f"keep={keep!r}: one of {sorted(_KEEP_RULES)} or a bool / uint8 tensor [N]")
    cap = batch.bound(max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    if n * (cap + 1) > 2 ** 31 - 1:
        raise ValueError(f"{n} nodes x (max_nodes_per_graph={cap} + 1) exceeds the int32 edge ids")
    new_id = torch.empty(n, dtype=torch.int32, device=dev)
    new_n_node = torch.zeros(b, dtype=torch.int32, device=dev)
    n_edge = torch.zeros(b, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)     # (an empty batch: the call writes nothing)
    ws = batch.call("gnf_graph_subgraph_count", rule, _abi.ptr(mask), int(bool(self_loops)), _abi.ptr(new_id), _abi.ptr(new_n_node),
                    _abi.ptr(rowptr), _abi.ptr(n_edge), _abi.ptr(totals), query="gnf_graph_subgraph_workspace_bytes")
    n_new, e_new = totals.tolist()
    node_index = torch.empty(n_new, dtype=torch.int32, device=dev)
    senders = torch.empty(e_new, dtype=torch.int32, device=dev)
    receivers = torch.empty(e_new, dtype=torch.int32, device=dev)
    _call(dev, "gnf_graph_subgraph_fill", (b, n, cap), (b, n, cap, _abi.ptr(rowptr), n_new, e_new, _abi.ptr(node_index),
                                                        _abi.ptr(senders), _abi.ptr(receivers)),
          query="gnf_graph_subgraph_workspace_bytes", ws=ws)
    rowptr = rowptr[:n_new + 1]
    kept = GraphsTuple(nodes=graph.nodes.index_select(0, node_index.to(graph.nodes.device)),
                       edges=torch.zeros(e_new, dtype=torch.float32, device=dev), receivers=receivers, senders=senders,
                       globals=graph.globals, n_node=new_n_node, n_edge=n_edge)
    sub = Csr(rowptr, senders, n_new, e_new)
    seed_csr_cache(kept, sub, by_sender=False)
    seed_csr_cache(kept, sub, by_sender=True)
    return {"graph": kept, "csr": sub, "node_index": node_index, "new_id": new_id, "total_nodes": totals[0],
            "total_edges": totals[1]}


def graph_hashes(graph, iterations=3, labels=None, max_nodes_per_graph=None, n_node_host=None):
    """Weisfeiler-Lehman hash of every graph of a GraphsTuple (gnf_graph_hashes; the definition is in
    include/gnf_graph_hashes.h), as a dict of device tensors:
      "hash"         int64 [B]: the 64-bit hash as its bit pattern - compare for equality only
      "node_colour"  int64 [N]: every node's colour after the last round, likewise
      "n_edges"      int64 [B]: simple undirected edges
      "n_node"       int32 [B]: the batch's sizes (the second half of the key uniqueness_novelty compares)
    Isomorphic graphs get equal hashes, whatever their node numbering.  The converse holds only as far as 1-dimensional
    colour refinement sees: a 6-cycle and two triangles, or two regular graphs of equal size and degree, collide by
    definition.  labels (int64 [N] on the device, permuted with the nodes) replaces the degree as the initial colour and is the
    way out - the triangle column of graph_orbits separates that pair.
    The CSR comes from graphs.csr_of: on the result of decode_graphs / generate_graphs no gnf_build_csr runs.  As for
    graph_stats, with max_nodes_per_graph (any upper bound on n_node, at most 65536) or n_node_host nothing is copied to the
    host and nothing synchronises, so the call can be captured; otherwise n_node is read once.  Up to WL_LDS_NODES columns
    one launch does all rounds; above, one launch per round.  Both give the same bits."""
    batch = _Batch("graph_hashes", graph)
    dev, n, b = batch.dev, batch.n, batch.b
    iterations = int(iterations)
    if not 0 <= iterations <= WL_MAX_ITERATIONS:
        raise ValueError(f"iterations={iterations}: 0 .. {WL_MAX_ITERATIONS}")
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
            raise ValueError(f"labels: an int64 tensor [{n}]")
        if labels.device.type != "cuda":
            raise _abi.GnfError("graph_hashes runs on a HIP device only (no CPU path)")
        labels = labels.to(dev).contiguous()
    batch.bound(max_nodes_per_graph, n_node_host, MAX_NODES_PER_GRAPH)
    out = {"hash": torch.empty(b, dtype=torch.int64, device=dev),
           "node_colour": torch.empty(n, dtype=torch.int64, device=dev),
           "n_edges": torch.empty(b, dtype=torch.int64, device=dev)}
    batch.call("gnf_graph_hashes", iterations, _abi.ptr(labels), _abi.ptr(out["hash"]), _abi.ptr(out["node_colour"]),
               _abi.ptr(out["n_edges"]))
    out["n_node"] = graph.n_node.to(torch.int32)
    return out


def _hash_set(x, iterations, dev=None):
    """(hash int64 [rows], n_node int32 [rows]), contiguous on one device, of a GraphsTuple or a graph_hashes result"""
    if not isinstance(x, dict):
        x = graph_hashes(x, iterations)
    elif not ("hash" in x and "n_node" in x):
        raise ValueError("uniqueness_novelty on a dict needs the result of graph_hashes in it")
    h, cnt = x["hash"], x["n_node"]
    for v in (h, cnt):
        if not isinstance(v, torch.Tensor) or v.device.type != "cuda":
            raise _abi.GnfError("uniqueness_novelty runs on a HIP device only (no CPU path)")
    if h.dim() != 1 or cnt.shape != h.shape or h.dtype != torch.int64:
        raise ValueError(f"uniqueness_novelty takes int64 [rows] hashes with [rows] sizes, got {h.dtype} {tuple(h.shape)} and "
                         f"{tuple(cnt.shape)}")
    dev = h.device if dev is None else dev
    return h.to(dev).contiguous(), cnt.to(device=dev, dtype=torch.int32).contiguous()


def uniqueness_novelty(generated, training, iterations=3):
    """Whether the generated graphs repeat each other or the training set (gnf_graph_hash_match).  Each argument is a
    GraphsTuple (hashed here with graph_hashes(g, iterations)) or a result of graph_hashes - hash the training set once and
    pass the result.  Two graphs count as the same when their hash and their n_node are equal: isomorphic graphs always do,
    and so do the pairs colour refinement cannot separate (see graph_hashes).  Graphs without nodes are left out.  Returns
      "uniqueness"          distinct / valid: the share of generated graphs that repeat no EARLIER generated graph
      "novelty"             novel / valid: the share that match no training graph
      "unique_novel"        the share that do neither                    (all three 0-d float64 device tensors)
      "first_in_generated"  int32 [A]: the first generated graph with this graph's key - itself for the first of its kind
      "match_in_training"   int32 [A]: the first matching training graph, else -1   (both -1 for a graph without nodes)
      "counts"              int64 [4]: valid, distinct, novel, distinct and novel
    An empty training set is allowed: everything is novel.  Raises ValueError when no generated graph has a node: reading the
    counts for that check is the call's only copy to the host when both arguments are graph_hashes results."""
    ha, ca = _hash_set(generated, iterations)
    dev = ha.device
    hb, cb = _hash_set(training, iterations, dev)
    a, b = int(ha.shape[0]), int(hb.shape[0])
    first = torch.empty(a, dtype=torch.int32, device=dev)
    match = torch.empty(a, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    _call(dev, "gnf_graph_hash_match", (a, b), (_abi.ptr(ha), _abi.ptr(ca), a, _abi.ptr(hb), _abi.ptr(cb), b, _abi.ptr(first),
                                                _abi.ptr(match), _abi.ptr(counts)))
    if counts[0].item() < 1:
        raise ValueError("uniqueness_novelty: no generated graph has a node")
    valid = counts[0].to(torch.float64)
    return {"uniqueness": counts[1].to(torch.float64) / valid, "novelty": counts[2].to(torch.float64) / valid,
            "unique_novel": counts[3].to(torch.float64) / valid, "first_in_generated": first, "match_in_training": match,
            "counts": counts}


def evaluate_generated(generated, reference, orbits=False, spectral=False, keep=None, train=None):
    """Degree and clustering MMD^2 of a generated batch against a reference batch: two GraphsTuples, or two results of
    graph_stats (clustering_hist with 100 bins).  Degree: EMD kernel, sigma 1, distance_scaling 1.  Clustering: 100 bins,
    EMD kernel, sigma 0.1, distance_scaling 100.  Returns {"degree_mmd", "clustering_mmd"}, 0-d float64 device tensors.
    orbits=True adds "orbit_mmd" (orbit_mmd, sigma 30); dicts passed instead of GraphsTuples must then also hold the
    result of graph_orbits ({**graph_stats(g), **graph_orbits(g)}).  spectral=True adds "spectral_mmd" (spectral_mmd on
    graph_spectra's default histograms, sigma 1); dicts must then also hold "spectral_hist".
    keep (keep_subgraphs' argument: "largest_component", "non_isolated" or a mask) reduces the GENERATED batch, a
    GraphsTuple, before it is scored - the usual post-processing of generated graphs; the reference batch is scored as
    given.  With a dict for `generated` there is no graph to reduce: ValueError.
    train (the TRAINING batch as a GraphsTuple, or its graph_hashes result - hash it once) adds "uniqueness", "novelty" and
    "unique_novel" (uniqueness_novelty, 3 rounds) of the generated batch, after keep= is applied - what the MMDs cannot see:
    a sampler that replays its training set.  A dict for `generated` must then hold the result of graph_hashes."""
    if keep is not None:
        if isinstance(generated, dict):
            raise ValueError("evaluate_generated(keep=...) needs the generated batch as a GraphsTuple, not its statistics")
        generated = keep_subgraphs(generated, keep)["graph"]
    if train is not None and isinstance(generated, dict) and not ("hash" in generated and "n_node" in generated):
        raise ValueError("evaluate_generated(train=...) on a dict needs the result of graph_hashes in it")
    inputs = (generated, reference)
    stats = [s if isinstance(s, dict) else graph_stats(s, clustering_bins=100) for s in inputs]
    for s in stats:
        if int(s["clustering_hist"].shape[1]) != 100:
            raise ValueError(f"evaluate_generated needs 100 clustering bins, got {int(s['clustering_hist'].shape[1])}")
    out = {"degree_mmd": hist_mmd(stats[0]["degree_hist"], stats[1]["degree_hist"], "gaussian_emd", 1.0, 1.0),
           "clustering_mmd": hist_mmd(stats[0]["clustering_hist"], stats[1]["clustering_hist"], "gaussian_emd", 0.1, 100.0)}
    if orbits:
        for s in inputs:
            if isinstance(s, dict) and not ("orbit_sums" in s and "n_node" in s):
                raise ValueError("evaluate_generated(orbits=True) on a dict needs the result of graph_orbits in it")
        sets = [s if isinstance(s, dict) else graph_orbits(s) for s in inputs]
        out["orbit_mmd"] = orbit_mmd(sets[0], sets[1], 30.0)
    if spectral:
        for s in inputs:
            if isinstance(s, dict) and "spectral_hist" not in s:
                raise ValueError("evaluate_generated(spectral=True) on a dict needs the result of graph_spectra in it")
        sets = [s if isinstance(s, dict) else graph_spectra(s) for s in inputs]
        out["spectral_mmd"] = spectral_mmd(sets[0], sets[1], 1.0)
    if train is not None:
        shares = uniqueness_novelty(generated, train, 3)
        out.update({k: shares[k] for k in NOVELTY_KEYS[:3]})
    return out
