"""Random graph models on the device (include/gnf_random_graphs.h): Erdos-Renyi G(n, p), the planted partition model and
Barabasi-Albert preferential attachment, as batches in the shape flow.decode_graphs returns - edge list in the decoder's order,
its CSR (which is both orientations), the edge total.  They are the baseline rows of graph_stats.evaluate_generated (fit_baseline,
baselines, evaluate_baselines) and a source of graph batches of chosen size and density that needs no data file.
random_graphs_host is the numpy twin: the same arrays, integer for integer, and the route of the generators on the CPU."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from .grevnet_synthetic_data import synthetic_draw

MODELS = ("erdos_renyi", "planted_partition", "barabasi_albert")
_M64 = (1 << 64) - 1
_TWO32 = 4294967296.0


def thresholds(p, n_graphs):
    """thr = (uint64)(p * 2^32) per graph (the product is exact): p a scalar or a sequence of n_graphs probabilities."""
    p = np.broadcast_to(np.asarray(p, np.float64).reshape(-1) if np.ndim(p) else np.float64(p), (n_graphs,))
    if p.size and not ((p >= 0.0) & (p <= 1.0)).all():
        raise ValueError("probabilities must lie in [0, 1]")
    return (p * _TWO32).astype(np.uint64)


def default_blocks(n, n_blocks):
    """block(i) = (i * n_blocks) // n for i in [0, n): int64"""
    return (np.arange(n, dtype=np.int64) * int(n_blocks)) // max(int(n), 1)


def _planted_host(n, g, thr_in, thr_out, block, seed, self_loops):
    i = np.arange(n, dtype=np.uint64)
    lo, hi = np.minimum(i[:, None], i[None, :]), np.maximum(i[:, None], i[None, :])
    d = synthetic_draw(seed, g, lo, hi).astype(np.uint64)
    thr = np.where(block[:, None] == block[None, :], np.uint64(thr_in), np.uint64(thr_out))
    adj = d < thr
    np.fill_diagonal(adj, bool(self_loops))
    return adj


def ba_targets_host(n, m, g, seed):
    """(targets int64 [n - m, m], fallback nodes) of include/gnf_random_graphs.h's Barabasi-Albert rule for n > m: row t - m
    holds targets(t).  First occurrences through np.unique - the restatement in tests/ walks the draws one by one instead."""
    table = np.zeros((n - m, m), np.int64)
    table[0] = np.arange(m)
    j = np.arange(_abi.GNF_RG_BA_DRAWS, dtype=np.uint64)
    fallbacks = 0
    for t in range(m + 1, n):
        size = 2 * m * (t - m)
        k = ((synthetic_draw((seed ^ _abi.GNF_RG_BA_SEED_XOR) & _M64, g, t, j).astype(np.uint64) * np.uint64(size))
             >> np.uint64(32)).astype(np.int64)
        tp, c = k // (2 * m), k % (2 * m)
        cand = np.where(c < m, table[tp, np.minimum(c, m - 1)], m + tp)
        _, first = np.unique(cand, return_index=True)
        acc = cand[np.sort(first)][:m]
        if len(acc) < m:
            fallbacks += 1
            rest = np.setdiff1d(np.arange(t), acc)[:m - len(acc)]      # ascending
            acc = np.concatenate([acc, rest])
        table[t - m] = acc
    return table, fallbacks


def _ba_host(n, m, g, seed, self_loops):
    adj = np.zeros((n, n), bool)
    fallbacks = 0
    if n > m:
        table, fallbacks = ba_targets_host(n, m, g, seed)
        t = np.repeat(np.arange(m, n), m)
        adj[t, table.ravel()] = True
        adj[table.ravel(), t] = True
    np.fill_diagonal(adj, bool(self_loops))
    return adj, fallbacks


def random_graphs_host(model, n_node, thresholds_or_m, thr_out=None, n_blocks=1, blocks=None, seed=0, first_graph=0,
                       self_loops=False, max_m=_abi.GNF_RG_MAX_M):
    """The arrays of include/gnf_random_graphs.h in numpy, integer for integer what the device writes:
      "senders", "receivers" int32 [E] (batch-wide ids, receivers ascending, senders ascending within a receiver),
      "rowptr" int32 [N + 1], "n_edge" int32 [B], "total" int, "n_node" int32 [B], "fallbacks" (nodes that took the Barabasi-
      Albert fallback, per graph).
    model "planted_partition" (or "erdos_renyi": thr_out, n_blocks and blocks are then not looked at): thresholds_or_m is the
    uint64 in-block threshold per graph (thresholds(p, B)), thr_out the out-of-block one (None: the same), blocks an int [N]
    label array or None for n_blocks contiguous blocks.  model "barabasi_albert": thresholds_or_m is m per graph, clamped into
    [1, max_m]."""
    if model not in MODELS:
        raise ValueError(f"model={model!r}: one of {MODELS}")
    n_node = np.maximum(np.asarray(n_node, np.int64).reshape(-1), 0)
    b = len(n_node)
    offs = np.concatenate([[0], np.cumsum(n_node)])
    par = np.broadcast_to(np.asarray(thresholds_or_m).reshape(-1), (b,)) if b else np.zeros(0, np.int64)
    if model == "erdos_renyi":
        thr_out, n_blocks, blocks = None, 1, None
    out_par = par if thr_out is None else np.broadcast_to(np.asarray(thr_out).reshape(-1), (b,))
    snd, rcv, n_edge, rowcnt, fallbacks = [], [], [], [], []
    for q, n in enumerate(n_node.tolist()):
        g = int(first_graph) + q
        if model == "barabasi_albert":
            adj, fb = _ba_host(n, int(min(max(int(par[q]), 1), max_m)), g, int(seed), self_loops)
        else:
            block = default_blocks(n, n_blocks) if blocks is None else np.asarray(blocks, np.int64)[offs[q]:offs[q + 1]]
            adj, fb = _planted_host(n, g, int(par[q]), int(out_par[q]), block, int(seed) & _M64, self_loops), 0
        r, s = np.nonzero(adj)            # row-major: receivers ascend, senders ascend within a receiver
        snd.append(s + offs[q])
        rcv.append(r + offs[q])
        n_edge.append(len(r))
        rowcnt.append(adj.sum(axis=1))
        fallbacks.append(fb)
    cat = lambda xs: np.concatenate(xs + [np.zeros(0, np.int64)])
    rowptr = np.concatenate([[0], np.cumsum(cat(rowcnt))])
    return {"senders": cat(snd).astype(np.int32), "receivers": cat(rcv).astype(np.int32), "rowptr": rowptr.astype(np.int32),
            "n_edge": np.asarray(n_edge, np.int32), "total": int(rowptr[-1]), "n_node": n_node.astype(np.int32),
            "fallbacks": fallbacks}


# ---- generators -------------------------------------------------------------------------------------------------------------------
def _resolve_device(device, *tensors):
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((t.device for t in tensors if torch.is_tensor(t)), None)
        if dev is None:
            dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _per_graph(x, b, dev, dtype):
    """a scalar, sequence or tensor as a [b] tensor of dtype on dev (a tensor already there is not copied to the host)"""
    if torch.is_tensor(x):
        t = x.to(device=dev, dtype=dtype).reshape(-1)
    else:
        t = torch.as_tensor(np.asarray(x).reshape(-1)).to(device=dev, dtype=dtype)
    return (t.expand(b) if t.numel() == 1 else t).contiguous()


def _thr_tensor(p, b, dev):
    """(uint64)(p * 2^32) as int64 (the same bits: the value is at most 2^32) [b] on dev"""
    if not torch.is_tensor(p):
        return torch.from_numpy(thresholds(p, b).astype(np.int64)).to(dev)
    return (_per_graph(p, b, dev, torch.float64).clamp(0.0, 1.0) * _TWO32).to(torch.int64)


def _generate(model, n_node, param, param_out=None, n_blocks=1, blocks=None, max_m=None, seed=0, first_graph=0, self_loops=False,
              nodes=None, device=None, edge_capacity=None, seed_dev=None, max_nodes_per_graph=None):
    from .graphs import Csr, GraphsTuple, seed_csr_cache
    dev = _resolve_device(device, nodes, n_node, param)
    exact = edge_capacity is None
    if torch.is_tensor(n_node):
        nn = n_node.to(device=dev, dtype=torch.int32).contiguous()
        sizes = None if (nodes is not None and max_nodes_per_graph is not None) else n_node.cpu().tolist()
    else:
        sizes = [int(v) for v in np.asarray(n_node).reshape(-1)]
        nn = torch.as_tensor(np.asarray(sizes, np.int32)).to(dev)
    b = int(nn.shape[0])
    n = int(nodes.shape[0]) if nodes is not None else sum(sizes)
    if sizes is not None and sum(sizes) != n:
        raise ValueError(f"nodes has {n} rows, n_node counts {sum(sizes)}")
    largest = max(sizes) if sizes else 0
    cap = int(max_nodes_per_graph) if max_nodes_per_graph is not None else largest
    if sizes is not None and cap < largest:
        raise ValueError(f"max_nodes_per_graph={cap} is below the largest graph of the batch ({largest} nodes)")
    if nodes is None:
        nodes = torch.zeros(n, 1, dtype=torch.float32, device=dev)
    ba = model == "barabasi_albert"
    if ba:
        m = _per_graph(param, b, dev, torch.int32)
        if max_m is None and torch.is_tensor(param) and not exact:
            max_m = _abi.GNF_RG_MAX_M          # (reading the largest m would synchronise)
        elif max_m is None:
            largest_m = (int(m.max()) if torch.is_tensor(param) else int(np.max(param))) if b else 1
            max_m = min(max(largest_m, 1), _abi.GNF_RG_MAX_M)
    else:
        thr_in = _thr_tensor(param, b, dev)
        thr_out = None if param_out is None else _thr_tensor(param_out, b, dev)
        if blocks is not None:
            blocks = blocks.to(device=dev, dtype=torch.int32).contiguous() if torch.is_tensor(blocks) else \
                torch.as_tensor(np.asarray(blocks, np.int32).reshape(-1)).to(dev)
            if int(blocks.shape[0]) != n:
                raise ValueError(f"blocks has {int(blocks.shape[0])} labels for {n} nodes")
    if dev.type != "cuda":     # the numpy twin
        if seed_dev is not None:
            seed = int(seed_dev.reshape(-1)[0])
        sizes = nn.tolist() if sizes is None else sizes
        h = random_graphs_host(model, sizes, (m if ba else thr_in).numpy().view(np.int32 if ba else np.uint64),
                               None if ba or thr_out is None else thr_out.numpy().view(np.uint64), n_blocks,
                               None if blocks is None else blocks.numpy(), int(seed) & _M64, first_graph, self_loops,
                               max_m if ba else _abi.GNF_RG_MAX_M)
        e = h["total"] if exact else int(edge_capacity)
        senders, receivers = torch.zeros(e, dtype=torch.int32), torch.zeros(e, dtype=torch.int32)
        k = min(e, h["total"])
        senders[:k], receivers[:k] = torch.from_numpy(h["senders"][:k]), torch.from_numpy(h["receivers"][:k])
        rowptr, n_edge = torch.from_numpy(h["rowptr"]), torch.from_numpy(h["n_edge"])
        total = torch.tensor([h["total"]], dtype=torch.int64)
    else:
        lib = _abi.lib()
        spec = _abi.GnfRandomGraphSpec()
        spec.seed, spec.first_graph = int(seed) & _M64, int(first_graph) & _M64
        spec.seed_dev = None if seed_dev is None else seed_dev.data_ptr()
        spec.model = _abi.GNF_RG_BARABASI_ALBERT if ba else _abi.GNF_RG_PLANTED
        spec.self_loops = int(bool(self_loops))
        if ba:
            spec.m_dev, spec.max_m = m.data_ptr(), int(max_m)
        else:
            spec.thr_in, spec.thr_out = thr_in.data_ptr(), None if thr_out is None else thr_out.data_ptr()
            spec.block, spec.n_blocks = None if blocks is None else blocks.data_ptr(), int(n_blocks)
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        n_edge = torch.empty(b, dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        ws_bytes = lib.gnf_adj_edges_workspace_bytes(b, n, cap)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _abi.check(lib.gnf_random_graph_edges_count(C.byref(spec), _abi.ptr(nn), b, n, cap, _abi.ptr(rowptr), _abi.ptr(n_edge),
                                                        _abi.ptr(total), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)),
                       "gnf_random_graph_edges_count")
            e = int(total.item()) if exact else int(edge_capacity)
            senders = torch.empty(e, dtype=torch.int32, device=dev)
            receivers = torch.empty(e, dtype=torch.int32, device=dev)
            _abi.check(lib.gnf_adj_edges_fill(b, n, cap, _abi.ptr(rowptr), e, _abi.ptr(senders), _abi.ptr(receivers),
                                              _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), "gnf_adj_edges_fill")
    graph = GraphsTuple(nodes=nodes, edges=torch.zeros(e, dtype=torch.float32, device=dev), receivers=receivers, senders=senders,
                        globals=torch.zeros(b, dtype=torch.float32, device=dev), n_node=nn, n_edge=n_edge)
    csr = Csr(rowptr, senders, n, e)
    if exact and dev.type == "cuda":
        seed_csr_cache(graph, csr, by_sender=False)
        seed_csr_cache(graph, csr, by_sender=True)
    return {"graph": graph, "csr": csr, "total_edges": total[0]}


_COMMON = """n_node: the graphs' sizes, a sequence or an int tensor.  Common options: seed (the host word) or seed_dev (a one-word int64
    device tensor read when the kernels run - a captured call replayed after the word was changed draws other graphs);
    first_graph (graph b of the call is draw index first_graph + b: two calls of B / 2 give the graphs of one call of B);
    self_loops (one loop per node); nodes ([N, F] features to carry; zeros [N, 1] otherwise); device (default: that of the
    tensors given, else the current HIP device, else the CPU - there the numpy twin random_graphs_host computes the same arrays).
    Returns the dict flow.decode_graphs returns: "graph" (GraphsTuple; receivers ascending, senders ascending within a receiver),
    "csr" (graphs.Csr over (rowptr, senders): by receiver and, the edge set being symmetric, by sender), "total_edges".
    Without edge_capacity the call reads total_edges once, allocates exactly that many edges and seeds csr_of's cache for both
    orientations: a GRevNet call or graph_stats on result["graph"] launches no gnf_build_csr.  With edge_capacity - and n_node
    and the parameters as device tensors, `nodes` and max_nodes_per_graph given - nothing is copied to the host, so the call
    can be captured into a hipGraph; only the first min(total_edges, edge_capacity) edges are valid and the cache is not seeded."""


def erdos_renyi(n_node, p, **options):
    """G(n, p): every pair of a graph is an edge with probability p (a scalar, or one per graph as a sequence or tensor), decided
    by gnf_syn_draw(seed, graph, lo, hi) < (uint64)(p * 2^32) - p = 1 gives every pair, p = 0 none.
    """
    return _generate("erdos_renyi", n_node, p, **options)


def planted_partition(n_node, p_in, p_out, n_blocks=2, blocks=None, **options):
    """The planted partition model: a pair is an edge with probability p_in inside a block and p_out across blocks.  blocks: an
    int [N] label per node; None means n_blocks contiguous blocks of near-equal size, block(i) = (i * n_blocks) // n.
    """
    return _generate("planted_partition", n_node, p_in, p_out, n_blocks=n_blocks, blocks=blocks, **options)


def barabasi_albert(n_node, m, max_m=None, **options):
    """Barabasi-Albert preferential attachment: nodes m .. n - 1 each attach to m distinct earlier nodes drawn by degree (m a
    scalar or one per graph, clamped into [1, max_m]; max_m <= 64 defaults to the largest m given).  n > m nodes give exactly
    m (n - m) undirected edges and a connected graph; n <= m gives no edges.  One workgroup per graph with the targets table in
    LDS: max_nodes_per_graph * max_m <= 32768, else GnfError.
    """
    return _generate("barabasi_albert", n_node, m, max_m=max_m, **options)


for _f in (erdos_renyi, planted_partition, barabasi_albert):
    _f.__doc__ += "    " + _COMMON


# ---- baselines --------------------------------------------------------------------------------------------------------------------
def fit_params(n_edges, n_node, model):
    """The fitted parameter per graph from its undirected edge count E_b and size n_b (tensors on one device):
    erdos_renyi: p_b = E_b / C(n_b, 2), 0 when n_b < 2 (float64); barabasi_albert: m_b = clamp(round(E_b / n_b), 1,
    min(64, n_b - 1)) with round = floor(x + 1/2) in exact integers, and 1 where n_b < 2 (int32)."""
    e, n = n_edges.to(torch.int64), n_node.to(device=n_edges.device, dtype=torch.int64)
    if model == "erdos_renyi":
        pairs = n * (n - 1) // 2
        return torch.where(pairs > 0, e.to(torch.float64) / pairs.clamp(min=1).to(torch.float64),
                           torch.zeros_like(e, dtype=torch.float64)).clamp(max=1.0)
    if model == "barabasi_albert":
        rounded = (2 * e + n) // (2 * n.clamp(min=1))
        return torch.minimum(rounded, (n - 1).clamp(max=_abi.GNF_RG_MAX_M)).clamp(min=1).to(torch.int32)
    raise ValueError(f"fit_params: model={model!r} (erdos_renyi or barabasi_albert)")


def fit_baseline(reference, model):
    """fit_params from graph_stats(reference)["n_edges"]: one parameter per graph of the reference batch (a GraphsTuple on a HIP
    device, or its graph_stats result together with n_node as reference = (stats, n_node))."""
    from .graph_stats import graph_stats
    pair = type(reference) is tuple          # (a GraphsTuple is a namedtuple: not this)
    stats, n_node = reference if pair else (graph_stats(reference), reference.n_node)
    return fit_params(stats["n_edges"], n_node, model)


def baselines(reference, models=("erdos_renyi", "barabasi_albert"), seed=0):
    """One baseline graph per graph of `reference`, of the same size, with the parameter fitted to that graph (fit_baseline):
    {model: the generator's result dict}.  The reference's statistics are computed once."""
    from .graph_stats import graph_stats
    stats = graph_stats(reference)
    sizes = reference.n_node.cpu().tolist()
    nn = reference.n_node.to(device=stats["n_edges"].device, dtype=torch.int32)
    out = {}
    for model in models:
        par = fit_baseline((stats, nn), model)
        make = {"erdos_renyi": erdos_renyi, "barabasi_albert": barabasi_albert}[model]
        out[model] = make(sizes, par, seed=seed, device=par.device)
    return out


def evaluate_baselines(train, test, models=("erdos_renyi", "barabasi_albert"), seed=0, **evaluate_options):
    """The rows a table of generated-graph scores puts beside the model's: {model: graph_stats.evaluate_generated(the baseline
    fitted to `train` graph by graph, test, **evaluate_options)}."""
    from .graph_stats import evaluate_generated
    made = baselines(train, models, seed)
    return {model: evaluate_generated(made[model]["graph"], test, **evaluate_options) for model in models}
