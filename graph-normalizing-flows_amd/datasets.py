"""Harness-side data for the hot path (no arithmetic of the path itself):

  * GraphDataset       - the reference's GraphRNN-pickle datasets after graph_data.py:33-50 preprocessing
                         (to_directed + one self loop per node first), read from the committed
                         data/*.npz edge lists (tools/convert_datasets.py), with the reference's batch
                         semantics (graph_data.py:61-122): train split = first int(0.8*G) graphs,
                         graphs drawn uniformly WITH replacement (the `self.index` quirk at
                         graph_data.py:119 leaves train_index at 0), fresh N(0, scale^2) node features
                         per batch (graph_data.py:24-27).
  * fully_connected_edges / senders_receivers - the complete-graph + self-loop topology of
                         grevnet_synthetic_data.py:17-21 and utils.py:164-183 (sender-major order).
  * DeviceGraphDataset / complete_batch - the same batches assembled on the device (include/gnf_batches.h): the dataset is
                         uploaded once, a batch and both of its CSRs come out of one gnf_batch_assemble / gnf_complete_batch.
  * perturb_batch / NoisyGraphDataset - the denoising encoder's noisy batches (include/gnf_perturb.h; graph_data.py:206-280,
                         which deletes nothing): edges deleted per unordered node pair by a defined integer hash, the noisy
                         edge list and both of its CSRs from one gnf_perturb_edges on the device, numpy on the host.
  * synthetic stand-ins - protein / citeseer(ego) datasets are absent from the reference
                         (.MISSING_LARGE_BLOBS); BASELINE.md section 4 fixes the generators used instead.
"""
import os

import numpy as np

from .graphs import data_dicts_to_graphs_tuple

DATA_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")

# reference name (graph_data.py:283-300 FILENAME_MAP key) -> committed edge-list file
FILENAME_MAP = {
    "graph_rnn_grid": "grid.npz",
    "graph_rnn_ego_small": "citeseer_small.npz",
    "graph_rnn_community_small": "caveman_small.npz",
    "graph_rnn_community_medium": "community_medium.npz",
    "graph_rnn_grid_small": "grid_small.npz",   # no key in the reference map; BASELINE config 1
}


class EdgeListDataset:
    """A list of graphs as concatenated local edge lists."""

    def __init__(self, n_node, n_edge, senders, receivers):
        self.n_node = np.asarray(n_node, np.int32)
        self.n_edge = np.asarray(n_edge, np.int32)
        self.senders = np.asarray(senders, np.int32)
        self.receivers = np.asarray(receivers, np.int32)
        self.eoff = np.concatenate([[0], np.cumsum(self.n_edge)]).astype(np.int64)

    def __len__(self):
        return len(self.n_node)

    def graph(self, gid):
        lo, hi = self.eoff[gid], self.eoff[gid + 1]
        return int(self.n_node[gid]), self.senders[lo:hi], self.receivers[lo:hi]

    def data_dicts(self, graph_ids, nodes_fn):
        out = []
        for gid in graph_ids:
            n, s, r = self.graph(gid)
            out.append({"nodes": nodes_fn(n), "senders": s, "receivers": r, "n_node": n})
        return out

    @staticmethod
    def load(path):
        d = np.load(path)
        return EdgeListDataset(d["n_node"], d["n_edge"], d["senders"], d["receivers"])


class GraphDataset:
    def __init__(self, dataset_name, node_embedding_dim, gaussian_scale=1.0, seed=12345):
        self.all = EdgeListDataset.load(os.path.join(DATA_DIR, FILENAME_MAP[dataset_name]))
        g = len(self.all)
        self.train_ids = np.arange(0, int(0.8 * g))        # graph_data.py:77-78
        self.test_ids = np.arange(int(0.8 * g), g)
        self.dim = int(node_embedding_dim)
        self.scale = float(gaussian_scale)
        self.rng = np.random.default_rng(seed)              # run_grevnet.py:108 default seed

    def _features(self, n):
        return self.rng.normal(scale=self.scale, size=(n, self.dim)).astype(np.float32)

    def sample_ids(self, batch_size, split="train"):
        ids = self.train_ids if split == "train" else self.test_ids
        return self.rng.choice(ids, size=batch_size, replace=True)

    def get_next_train_batch(self, batch_size, device=None):
        return data_dicts_to_graphs_tuple(self.all.data_dicts(self.sample_ids(batch_size), self._features), device)

    def get_next_test_batch(self, batch_size, device=None):
        return data_dicts_to_graphs_tuple(self.all.data_dicts(self.sample_ids(batch_size, "test"), self._features),
                                          device)

    def get_random_test_batch(self, batch_size, device=None):            # graph_data.py:109-111
        return self.get_next_test_batch(batch_size, device)

    def full_n_nodes(self):                                              # graph_data.py:89-96
        return [int(n) for n in self.all.n_node]

    def train_n_nodes(self):
        return [int(self.all.n_node[i]) for i in self.train_ids]

    def test_n_nodes(self):
        return [int(self.all.n_node[i]) for i in self.test_ids]


class OverfitGraphDataset(GraphDataset):
    """graph_data.py:125-203: train on a handful of graphs.  The train split is sorted by node count; either
    the `num_graphs` smallest graphs, or the first graph of every size listed in `graph_sizes`, repeated
    cyclically up to max(num_graphs, train_batch_size) entries (subset_graphs, graph_data.py:157-177); batches are
    then drawn from that list exactly like GraphDataset's (uniformly with replacement, graph_data.py:194-203).
    full / train / test_n_nodes all describe the subset, as in the reference (graph_data.py:147-154)."""

    def __init__(self, dataset_name, num_graphs, train_batch_size, node_embedding_dim, graph_sizes=None,
                 gaussian_scale=1.0, seed=12345):
        super().__init__(dataset_name, node_embedding_dim, gaussian_scale, seed)
        order = sorted(self.train_ids.tolist(), key=lambda i: int(self.all.n_node[i]))   # stable, like list.sort
        if graph_sizes:
            first = {}
            for i in order:
                first.setdefault(int(self.all.n_node[i]), i)
            subset = [first[int(sz)] for sz in graph_sizes]                              # KeyError like the reference
        else:
            subset = order[:int(num_graphs)]
        want = max(int(num_graphs), int(train_batch_size))
        self.train_ids = np.array([subset[k % len(subset)] for k in range(want)], dtype=np.int64)

    def full_n_nodes(self):
        return self.train_n_nodes()

    def test_n_nodes(self):
        return self.train_n_nodes()


def _int32_arena(sizes, device, zero=False):
    """One int32 allocation cut into len(sizes) tensors, each starting on a 256-byte boundary."""
    import torch
    starts, total = [], 0
    for n in sizes:
        starts.append(total)
        total += (int(n) + 63) // 64 * 64
    buf = (torch.zeros if zero else torch.empty)(max(total, 1), dtype=torch.int32, device=device)
    return [buf[a:a + int(n)] for a, n in zip(starts, sizes)]


class DeviceGraphDataset:
    """GraphDataset with the dataset resident on the device: the edge lists are uploaded once (dataset-wide node ids), the two
    dataset-wide CSRs are built once by gnf_build_csr (graphs.build_csr_device), and every batch - n_node, n_edge, node
    offsets, senders, receivers and BOTH CSRs - comes out of one gnf_batch_assemble (include/gnf_batches.h): no host loop over
    the graphs, no index upload beyond the B graph ids, no sort.  n_node / n_edge stay on the host to size the outputs, so
    nothing is read back.  Same split rule (train = the first int(0.8 G) graphs) and method names as GraphDataset; the ids are
    drawn on the host from the same numpy stream as GraphDataset.sample_ids.
    The node FEATURES are a different stream from GraphDataset's: torch.randn on the device from a torch.Generator seeded with
    `seed`, times gaussian_scale (GraphDataset draws them with numpy on the host, interleaved with the ids) - same
    distribution, other numbers.
    `dataset`: a FILENAME_MAP name or an EdgeListDataset.  There is no CPU path: the device must be a HIP device."""

    def __init__(self, dataset, node_embedding_dim, gaussian_scale=1.0, seed=12345, device=None):
        import torch
        from . import _abi
        from .graphs import GraphsTuple, build_csr_device
        self.all = EdgeListDataset.load(os.path.join(DATA_DIR, FILENAME_MAP[dataset])) if isinstance(dataset, str) else dataset
        g = len(self.all)
        self.train_ids = np.arange(0, int(0.8 * g))
        self.test_ids = np.arange(int(0.8 * g), g)
        self.dim = int(node_embedding_dim)
        self.scale = float(gaussian_scale)
        self.rng = np.random.default_rng(seed)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise _abi.GnfError("DeviceGraphDataset needs a HIP device; there is no CPU path (GraphDataset is the host route)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.gen = torch.Generator(device=self.device).manual_seed(int(seed))
        n_node = self.all.n_node.astype(np.int64)
        n_edge = self.all.n_edge.astype(np.int64)
        self._n_node, self._n_edge = n_node, n_edge
        node_off = np.concatenate([[0], np.cumsum(n_node)])
        if node_off[-1] >= 2 ** 31 - 1 or self.all.eoff[-1] > 2 ** 31 - 1:
            raise ValueError("DeviceGraphDataset: the dataset-wide CSR is int32")
        shift = np.repeat(node_off[:-1], n_edge)
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(self.device)
        self._node_off, self._edge_off = up(node_off, np.int32), up(self.all.eoff, np.int64)
        big = GraphsTuple(nodes=torch.empty(int(node_off[-1]), 0, device=self.device), edges=None,
                          receivers=up(self.all.receivers + shift, np.int32), senders=up(self.all.senders + shift, np.int32),
                          globals=None, n_node=up(n_node, np.int32), n_edge=up(n_edge, np.int32))
        self._big, self._csr, self._csr_t = big, build_csr_device(big), build_csr_device(big, by_sender=True)
        e_all = int(self.all.eoff[-1])
        edge_ptr = lambda t: t.data_ptr() if e_all else 0
        self._store = _abi.GnfBatchStore(self._node_off.data_ptr(), self._edge_off.data_ptr(), edge_ptr(big.senders),
                                         edge_ptr(big.receivers), self._csr.rowptr.data_ptr(), edge_ptr(self._csr.col),
                                         self._csr_t.rowptr.data_ptr(), edge_ptr(self._csr_t.col), g, int(node_off[-1]), e_all)

    def sample_ids(self, batch_size, split="train"):
        ids = self.train_ids if split == "train" else self.test_ids
        return self.rng.choice(ids, size=batch_size, replace=True)

    def batch_of(self, graph_ids, nodes=None, split=None):
        """The batch of the graphs `graph_ids` (host integers; repeats allowed, any order) as a GraphsTuple on the device whose
        CSR cache is seeded for both orientations and whose node-offset cache is seeded: csr_of / node_offsets_of return what
        this call made, no gnf_build_csr runs afterwards.  Deterministic in graph_ids.  nodes: [sum n_node, D] features to use
        (a device tensor is used as it is); None draws them from the dataset's device generator.  split = "train" / "test":
        the ids must lie in that split; None: anywhere in the dataset.  Ids outside raise ValueError."""
        import ctypes as C
        import torch
        from . import _abi
        from .graphs import Csr, GraphsTuple, seed_csr_cache, seed_node_offsets_cache
        ids = np.asarray(graph_ids, np.int64).reshape(-1)
        allowed = {None: (0, len(self.all)), "train": (0, len(self.train_ids)),
                   "test": (len(self.train_ids), len(self.all))}[split]
        if len(ids) and (ids.min() < allowed[0] or ids.max() >= allowed[1]):
            raise ValueError(f"DeviceGraphDataset.batch_of: graph ids outside [{allowed[0]}, {allowed[1]})"
                             + (f", the {split} split" if split else ""))
        b, n, e = len(ids), int(self._n_node[ids].sum()), int(self._n_edge[ids].sum())
        dev = self.device
        lib = _abi.lib()
        ws_bytes = lib.gnf_batch_assemble_workspace_bytes(b)
        live = b > 0 and n > 0     # otherwise the call writes rowptr[0] only: the sizes and offsets are zeros
        n_node, n_edge, offsets, snd, rcv, rowptr, col, rowptr_t, col_t, ws = _int32_arena(
            [b, b, b + 1, e, e, n + 1, e, n + 1, e, (ws_bytes + 3) // 4 + 1], dev, zero=not live)
        gid = torch.as_tensor(ids.astype(np.int32)).to(dev)
        with torch.cuda.device(dev):
            _abi.check(lib.gnf_batch_assemble(C.byref(self._store), _abi.ptr(gid), b, n, e, _abi.ptr(n_node), _abi.ptr(n_edge),
                                              _abi.ptr(offsets), _abi.ptr(snd), _abi.ptr(rcv), _abi.ptr(rowptr), _abi.ptr(col),
                                              _abi.ptr(rowptr_t), _abi.ptr(col_t), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)),
                       "gnf_batch_assemble")
        if nodes is None:
            nodes = torch.randn((n, self.dim), generator=self.gen, device=dev, dtype=torch.float32) * self.scale
        elif not isinstance(nodes, torch.Tensor):
            nodes = torch.as_tensor(np.asarray(nodes, np.float32)).to(dev)
        elif nodes.device != dev:
            nodes = nodes.to(dev)
        if nodes.shape[0] != n:
            raise ValueError(f"DeviceGraphDataset.batch_of: {nodes.shape[0]} feature rows for {n} nodes")
        graph = GraphsTuple(nodes=nodes, edges=torch.zeros(e, dtype=torch.float32, device=dev), receivers=rcv, senders=snd,
                            globals=torch.zeros(b, dtype=torch.float32, device=dev), n_node=n_node, n_edge=n_edge)
        seed_csr_cache(graph, Csr(rowptr, col, n, e))
        seed_csr_cache(graph, Csr(rowptr_t, col_t, n, e), by_sender=True)
        seed_node_offsets_cache(graph, offsets)
        return graph

    def get_next_train_batch(self, batch_size, device=None):
        return self.batch_of(self.sample_ids(batch_size), split="train")

    def get_next_test_batch(self, batch_size, device=None):
        return self.batch_of(self.sample_ids(batch_size, "test"), split="test")

    def get_random_test_batch(self, batch_size, device=None):
        return self.get_next_test_batch(batch_size)

    def full_n_nodes(self):
        return [int(n) for n in self.all.n_node]

    def train_n_nodes(self):
        return [int(self.all.n_node[i]) for i in self.train_ids]

    def test_n_nodes(self):
        return [int(self.all.n_node[i]) for i in self.test_ids]


# ----------------------------------------------------------------------------------------------
# Edge-deletion noise for the denoising encoder (include/gnf_perturb.h; run_gnn.py --denoising, graph_data.py:206-280)
# ----------------------------------------------------------------------------------------------
PERTURB_LOOPS = {"keep": 0, "draw": 1}       # GNF_PERTURB_LOOPS_KEEP / GNF_PERTURB_LOOPS_DRAW
PERTURB_KEYS = ("senders", "receivers", "rowptr", "col", "rowptr_t", "col_t", "n_edge", "num_removed", "totals")
_M64 = (1 << 64) - 1


def perturb_threshold(deletion_prob):
    """(uint64_t)(deletion_prob * 2^32) of include/gnf_perturb.h: a pair is deleted iff its draw is below it."""
    p = float(deletion_prob)
    if not 0.0 <= p <= 1.0:      # NaN included
        raise ValueError(f"deletion_prob={deletion_prob!r} is not in [0, 1]")
    return int(p * 4294967296.0)


def perturb_draw(seed, lo, hi):
    """The pair's 32-bit draw of include/gnf_perturb.h in numpy uint64 arithmetic (wrapping); lo <= hi are node ids."""
    u = np.uint64
    lo = np.atleast_1d(np.asarray(lo)).astype(u)
    hi = np.atleast_1d(np.asarray(hi)).astype(u)
    with np.errstate(over="ignore"):
        x = np.full(1, int(seed) & _M64, u) ^ (u(0x9E3779B97F4A7C15) * (lo + u(1))) ^ (u(0xBF58476D1CE4E5B9) * (hi + u(1)))
        x = x ^ (x >> u(30))
        x = x * u(0xBF58476D1CE4E5B9)
        x = x ^ (x >> u(27))
        x = x * u(0x94D049BB133111EB)
        x = x ^ (x >> u(31))
    return (x >> u(32)).astype(np.int64)


def perturb_keep_mask(senders, receivers, deletion_prob, seed, self_loops="keep"):
    """bool [E]: which directed edges (batch-global ids) survive - the definition of include/gnf_perturb.h."""
    s = np.asarray(senders, np.int64)
    r = np.asarray(receivers, np.int64)
    keep = perturb_draw(seed, np.minimum(s, r), np.maximum(s, r)) >= perturb_threshold(deletion_prob)
    if PERTURB_LOOPS[self_loops] == 0:
        keep |= s == r
    return keep


def perturb_arrays_host(senders, receivers, n_nodes, n_edge, deletion_prob, seed, self_loops="keep"):
    """The host route gnf_perturb_edges is held to: filter the edge list with perturb_keep_mask, then graphs.build_csr_host by
    receiver and by sender on what is left.  Returns the PERTURB_KEYS arrays (int32; totals int64 [2] = {E', E - E'})."""
    from .graphs import build_csr_host
    s = np.asarray(senders, np.int64)
    r = np.asarray(receivers, np.int64)
    n_edge = np.asarray(n_edge, np.int64)
    keep = perturb_keep_mask(s, r, deletion_prob, seed, self_loops)
    s2, r2 = s[keep], r[keep]
    rowptr, col = build_csr_host(s2, r2, int(n_nodes))
    rowptr_t, col_t = build_csr_host(r2, s2, int(n_nodes))
    kept = np.bincount(np.repeat(np.arange(len(n_edge)), n_edge)[keep], minlength=len(n_edge)).astype(np.int64)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return dict(senders=i32(s2), receivers=i32(r2), rowptr=i32(rowptr), col=i32(col), rowptr_t=i32(rowptr_t), col_t=i32(col_t),
                n_edge=i32(kept), num_removed=i32(n_edge - kept), totals=np.array([len(s2), len(s) - len(s2)], np.int64))


def perturb_batch(graph, deletion_prob, seed, self_loops="keep", seed_tensor=None, exact=True):
    """The noisy batch of the denoising encoder: `graph` with every unordered node pair's edges deleted with probability
    deletion_prob (the definition, the self_loops modes "keep" / "draw" and the random stream: include/gnf_perturb.h).
    Returns (noisy, num_removed): noisy shares nodes, n_node and globals with `graph` and has edge arrays of its own, with
    edges = zeros(E'); num_removed is int32 [B] on the batch's device, deleted directed entries per graph.
    On a HIP device one gnf_perturb_edges call makes the edge list and BOTH CSRs of the noisy batch from csr_of(graph) in both
    orientations (cache hits on a DeviceGraphDataset batch).
      exact=True   reads E' once (an 8-byte copy, the call's only synchronisation), narrows the tensors to E' and seeds the CSR
                   cache for both orientations and the node-offset cache: the encoder and the trainer launch no gnf_build_csr
                   on `noisy`.
      exact=False  copies nothing to the host and synchronises nowhere - the capturable form.  Returns (noisy, num_removed,
                   info): the edge tensors of noisy have the capacity E of which the first info["total_edges"] (0-d device
                   int64) are valid, the rest unspecified; info also holds "rowptr", "col", "rowptr_t", "col_t".  No cache is
                   seeded (as flow.decode_graphs' edge_capacity mode).
    seed_tensor: None, or an int64 [1] tensor on the batch's device whose 64 bits are the seed, read by the kernels at run time
    instead of `seed`: a captured call replayed after the tensor changed draws fresh noise.
    On a CPU batch the same arrays come from perturb_arrays_host (numpy); exact is always True there and no cache is seeded."""
    import ctypes as C
    import torch
    from . import _abi
    from .graphs import (Csr, GraphsTuple, csr_desc, csr_of, node_offsets_of, seed_csr_cache, seed_node_offsets_cache)
    loops = PERTURB_LOOPS[self_loops]
    perturb_threshold(deletion_prob)                                 # ValueError for a bad probability, on every route
    dev = graph.senders.device
    b, n, e = int(graph.n_node.shape[0]), int(graph.nodes.shape[0]), int(graph.senders.shape[0])
    if dev.type != "cuda":
        if seed_tensor is not None:
            seed = int(seed_tensor.reshape(-1)[0])
        out = perturb_arrays_host(graph.senders.numpy(), graph.receivers.numpy(), n, graph.n_edge.numpy(), deletion_prob, seed,
                                  self_loops)
        e2 = int(out["totals"][0])
        noisy = graph.replace(senders=torch.from_numpy(out["senders"]), receivers=torch.from_numpy(out["receivers"]),
                              edges=torch.zeros(e2, dtype=torch.float32), n_edge=torch.from_numpy(out["n_edge"]))
        return noisy, torch.from_numpy(out["num_removed"])
    lib = _abi.lib()
    csr, csr_t = csr_of(graph), csr_of(graph, by_sender=True)
    offsets = node_offsets_of(graph)
    ws_bytes = lib.gnf_perturb_edges_workspace_bytes(b, n, e)
    live = b > 0 and n > 0       # otherwise the call writes rowptr[0] and totals only: everything else is zeros
    snd, rcv, rowptr, col, rowptr_t, col_t, n_edge, removed, tot, ws = _int32_arena(
        [e, e, n + 1, e, n + 1, e, b, b, 4, (ws_bytes + 3) // 4 + 1], dev, zero=not live)
    totals = tot.view(torch.int64)
    if seed_tensor is not None and (seed_tensor.device != dev or seed_tensor.dtype != torch.int64 or seed_tensor.numel() < 1):
        raise ValueError("perturb_batch: seed_tensor is an int64 [1] tensor on the batch's device")
    spec = _abi.GnfPerturbSpec(float(deletion_prob), int(seed) & _M64, 0 if seed_tensor is None else seed_tensor.data_ptr(), loops)
    d, d_t = csr_desc(graph, csr, node_offsets=True), csr_desc(graph, csr_t, node_offsets=True)
    edge_ptr = lambda t: _abi.ptr(t if e else None)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_perturb_edges(edge_ptr(graph.senders), edge_ptr(graph.receivers), _abi.ptr(graph.n_edge), C.byref(d),
                                         C.byref(d_t), C.byref(spec), _abi.ptr(snd), _abi.ptr(rcv), _abi.ptr(rowptr),
                                         _abi.ptr(col), _abi.ptr(rowptr_t), _abi.ptr(col_t), _abi.ptr(n_edge), _abi.ptr(removed),
                                         _abi.ptr(totals), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)), "gnf_perturb_edges")
    if not exact:
        noisy = GraphsTuple(nodes=graph.nodes, edges=torch.zeros(e, dtype=torch.float32, device=dev), receivers=rcv, senders=snd,
                            globals=graph.globals, n_node=graph.n_node, n_edge=n_edge)
        return noisy, removed, dict(total_edges=totals[0], rowptr=rowptr, col=col, rowptr_t=rowptr_t, col_t=col_t)
    e2 = int(totals[0].item())
    noisy = GraphsTuple(nodes=graph.nodes, edges=torch.zeros(e2, dtype=torch.float32, device=dev), receivers=rcv[:e2],
                        senders=snd[:e2], globals=graph.globals, n_node=graph.n_node, n_edge=n_edge)
    seed_csr_cache(noisy, Csr(rowptr, col[:e2], n, e2))
    seed_csr_cache(noisy, Csr(rowptr_t, col_t[:e2], n, e2), by_sender=True)
    seed_node_offsets_cache(noisy, offsets)
    return noisy, removed


class NoisyGraphDataset(GraphDataset):
    """graph_data.py:206-280 for the denoising encoder (run_gnn.py --denoising): get_next_train_batch hands out
    (true, noisy, num_removed) - the clean batch, the same batch with edges deleted by perturb_batch, and the deleted directed
    entries per graph.  Two things the reference does not do and this class does: it ACTUALLY DELETES the edges (the
    reference's remove_edges_from is commented out, graph_data.py:247) and it RETURNS THE NOISY BATCH (the reference returns
    the clean batch twice, graph_data.py:279-280).  The noise seed is `seed` plus a counter of the train batches handed out, so
    no two steps share a mask.  Test batches are clean: the reference feeds the test batch as its own noisy version
    (run_gnn.py:445-446).
    device=None: a GraphDataset - batches are assembled and perturbed on the host (numpy), then moved to the `device` argument
    of the batch methods, if any.  Otherwise it wraps a DeviceGraphDataset on that device: the true batch and both of its CSRs
    come from one gnf_batch_assemble, the noisy batch and both of its CSRs from one gnf_perturb_edges; `dataset_name` may then
    also be an EdgeListDataset."""

    def __init__(self, dataset_name, node_embedding_dim, deletion_prob=0.5, gaussian_scale=1.0, seed=12345, device=None,
                 self_loops="keep"):
        perturb_threshold(deletion_prob)
        PERTURB_LOOPS[self_loops]
        self.deletion_prob, self.self_loops, self.seed, self.calls = float(deletion_prob), self_loops, int(seed), 0
        if device is None:
            super().__init__(dataset_name, node_embedding_dim, gaussian_scale, seed)
            self.on_device = None
        else:
            self.on_device = inner = DeviceGraphDataset(dataset_name, node_embedding_dim, gaussian_scale, seed, device)
            self.all, self.train_ids, self.test_ids = inner.all, inner.train_ids, inner.test_ids
            self.dim, self.scale, self.rng = inner.dim, inner.scale, inner.rng

    def get_next_train_batch(self, batch_size, device=None):
        noise_seed = (self.seed + self.calls) & _M64
        self.calls += 1
        if self.on_device is not None:
            true = self.on_device.get_next_train_batch(batch_size)
            noisy, removed = perturb_batch(true, self.deletion_prob, noise_seed, self.self_loops)
            return true, noisy, removed
        true = super().get_next_train_batch(batch_size)
        noisy, removed = perturb_batch(true, self.deletion_prob, noise_seed, self.self_loops)
        if device is not None:
            true, noisy, removed = true.to(device), noisy.to(device), removed.to(device)
        return true, noisy, removed

    def get_next_test_batch(self, batch_size, device=None):
        if self.on_device is not None:
            return self.on_device.get_next_test_batch(batch_size)
        return super().get_next_test_batch(batch_size, device)


def fully_connected_edges(n):
    """All ordered pairs (a, b) incl. self, sender-major (utils.py:138-143 order; same edge SET as
    grevnet_synthetic_data.py:17-21)."""
    a = np.repeat(np.arange(n, dtype=np.int32), n)
    b = np.tile(np.arange(n, dtype=np.int32), n)
    return a, b


def senders_receivers(n_node):
    """utils.py:164-183 for a whole batch: returns (senders, receivers, n_edge = n_node**2) with global ids."""
    s, r, off = [], [], 0
    for n in n_node:
        a, b = fully_connected_edges(int(n))
        s.append(a + off)
        r.append(b + off)
        off += int(n)
    return np.concatenate(s), np.concatenate(r), np.asarray(n_node, np.int32) ** 2


def with_fully_connected_topology(ds):
    """Same node counts, complete-graph topology (train_grevnet_with_data.py:237-244 transform_example)."""
    S, R = [], []
    for n in ds.n_node:
        a, b = fully_connected_edges(int(n))
        S.append(a)
        R.append(b)
    return EdgeListDataset(ds.n_node, ds.n_node.astype(np.int64) ** 2, np.concatenate(S), np.concatenate(R))


def _knn_graph(rng, n, k):
    """Random geometric k-NN graph in the unit square, symmetrised, + self loops first
    (the data shape of graph_data.py:33-50)."""
    pts = rng.random((n, 2))
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    nbr = np.argsort(d2, axis=1)[:, :k]
    adj = np.zeros((n, n), bool)
    adj[np.repeat(np.arange(n), k), nbr.ravel()] = True
    adj |= adj.T
    s, r = np.nonzero(adj)
    idx = np.arange(n)
    return np.concatenate([idx, s]).astype(np.int32), np.concatenate([idx, r]).astype(np.int32)


def synthetic_protein(num_graphs, seed=12345):
    """Stand-in for the absent protein dataset: n ~ U{100..500}, geometric k-NN
    graph with mean degree about 5, + self loops."""
    rng = np.random.default_rng(seed)
    nn, ne, S, R = [], [], [], []
    for _ in range(num_graphs):
        n = int(rng.integers(100, 501))
        s, r = _knn_graph(rng, n, 3)
        nn.append(n); ne.append(len(s)); S.append(s); R.append(r)
    return EdgeListDataset(nn, ne, np.concatenate(S), np.concatenate(R))


def synthetic_ego(num_graphs, seed=12345):
    """Stand-in for the absent citeseer (ego) dataset: n ~ U{50..399}; node 0 is
    the ego hub (linked to a third of the nodes), the rest grows by preferential attachment with 2
    links per new node (mean degree about 5-6), + self loops first."""
    rng = np.random.default_rng(seed)
    nn, ne, S, R = [], [], [], []
    for _ in range(num_graphs):
        n = int(rng.integers(50, 400))
        deg = np.zeros(n)
        edges = set()
        for v in range(1, n):
            if v % 3 == 1:
                edges.add((0, v)); deg[0] += 1; deg[v] += 1
            w = deg[:v] + 1.0
            for u in rng.choice(v, size=min(2, v), replace=False, p=w / w.sum()):
                e = (int(u), v)
                if e not in edges:
                    edges.add(e); deg[u] += 1; deg[v] += 1
        und = np.array(sorted(edges), dtype=np.int32).reshape(-1, 2)
        idx = np.arange(n, dtype=np.int32)
        s = np.concatenate([idx, und[:, 0], und[:, 1]])
        r = np.concatenate([idx, und[:, 1], und[:, 0]])
        nn.append(n); ne.append(len(s)); S.append(s); R.append(r)
    return EdgeListDataset(nn, ne, np.concatenate(S), np.concatenate(R))


# ----------------------------------------------------------------------------------------------
# On-disk embedding chunks of the data-backed trainer
#   writer: generate_grevnet_training_data.py:89-97,116-120   reader: train_grevnet_with_data.py:145-234
# A chunk is pickle.dump((node_embeddings[sum(n_node), D] float, n_node[B] int32)); a directory of chunks
# is consumed in os.listdir order.
# ----------------------------------------------------------------------------------------------
def write_embedding_chunk(path, node_embeddings, n_node):
    """generate_grevnet_training_data.py:91-92."""
    import pickle
    node_embeddings = np.asarray(node_embeddings)
    n_node = np.asarray(n_node, np.int32)
    if node_embeddings.ndim != 2 or int(n_node.sum()) != node_embeddings.shape[0]:
        raise ValueError("node_embeddings must be [sum(n_node), D]")
    with open(path, "wb") as f:
        pickle.dump((node_embeddings, n_node), f)


def _read_embedding_chunk(path):
    import pickle
    with open(path, "rb") as f:
        node_embeddings, n_node = pickle.load(f)[:2]
    return node_embeddings, np.asarray(n_node)


def plan_fixed_batches(n_node, batch_size):
    """Graph ranges [lo, hi) of one chunk for a fixed number of graphs per batch: whole batches only - the graphs
    left over at the end of a chunk are dropped (train_grevnet_with_data.py:163-176 moves on to the next file as
    soon as the current one cannot supply `train_batch_size` more graphs)."""
    whole = len(n_node) // batch_size
    return [(k * batch_size, (k + 1) * batch_size) for k in range(whole)]


def plan_variable_batches(n_node, max_nodes):
    """Graph ranges [lo, hi) of one chunk for batches of consecutive graphs holding FEWER than max_nodes nodes
    (strict, train_grevnet_with_data.py:221): a batch closes in front of the first graph that would reach the
    limit; the range that runs into the end of the chunk is emitted short (:201-219)."""
    out, lo, total = [], 0, 0
    for g, n in enumerate(n_node):
        if total + int(n) >= max_nodes:
            out.append((lo, g))
            lo, total = g, 0
            # the graph that did not fit opens the next batch - unless it cannot fit in ANY batch
            if int(n) >= max_nodes:
                raise ValueError(f"graph {g} has {int(n)} nodes: never fits under max_nodes={max_nodes} "
                                 "(the reference would hand out empty batches forever)")
        total += int(n)
    out.append((lo, len(n_node)))
    return out


class _ChunkBatches:
    """Batches out of a directory of embedding chunks: the files are visited once in order, each chunk is cut by
    `plan` into graph ranges, a batch is (node_embeddings[rows of the range], n_node[range]).  Running past the
    last file raises IndexError, like the reference's `self.files[self.file_ind]`.
    The first chunk is opened (and cut) by the constructor, as the reference's readers do in theirs
    (train_grevnet_with_data.py:150-157, 188-195): an empty or unreadable directory, or a graph that can never fit under
    max_nodes, fails there and not in the middle of an epoch; `file_ind` exists from the start.
    One deliberate difference: the short LAST batch of the LAST file is handed out (the variable-size reader of the
    reference loses it - it raises IndexError while opening the file after the last one, before returning the batch).
    device (not in the reference; None = the behaviour above): a chunk's embeddings are uploaded once, as float32, when the chunk
    is opened, and a batch's embeddings are a row-range VIEW of that device tensor (the ranges are consecutive rows: no copy,
    nothing crosses the bus per batch); n_node stays a host array."""

    def __init__(self, directory, files, plan, device=None):
        import os
        self.device = device
        self._paths = [os.path.join(directory, f) for f in files]
        self.files = list(files)
        self._plan = plan
        self.file_ind = 0
        if not self._paths:
            raise IndexError(f"{type(self).__name__}: no training files in {directory!r}")
        self._first = self._cut(self._paths[0])
        self._batches = self._generate()

    def _cut(self, path):
        emb, n_node = _read_embedding_chunk(path)
        if self.device is not None:
            import torch
            emb = torch.as_tensor(np.ascontiguousarray(emb, np.float32)).to(self.device)
        row_end = np.concatenate([[0], np.cumsum(n_node)])
        self.n_node = n_node      # the chunk just opened, like the reference readers' self.n_node = d[1] (:157, 172)
        return emb, n_node, row_end, self._plan(n_node)

    def _generate(self):
        for ind, path in enumerate(self._paths):
            self.file_ind = ind
            emb, n_node, row_end, ranges = self._first if ind == 0 else self._cut(path)
            self._first = None
            for lo, hi in ranges:
                yield emb[int(row_end[lo]):int(row_end[hi])], n_node[lo:hi]

    def train_batch(self):
        try:
            return next(self._batches)
        except StopIteration:
            raise IndexError(f"{type(self).__name__}: out of training files (the reference raises IndexError too)") from None


def _chunk_files(directory, sort_files):
    import os
    # os.listdir order, like the reference: unspecified, it changes from one directory to the next.
    # sort_files=True (not in the reference) makes a run reproducible.
    return sorted(os.listdir(directory)) if sort_files else os.listdir(directory)


class GrevnetDatasetFixed(_ChunkBatches):
    """train_grevnet_with_data.py:145-180: `train_batch_size` graphs per batch, chunk tails dropped;
    `train_epochs` is FLAGS.train_epochs (the file list is repeated that many times)."""

    def __init__(self, train_data_dir, train_batch_size, train_epochs=1, sort_files=False, device=None):
        self.train_batch_size = int(train_batch_size)
        super().__init__(train_data_dir, _chunk_files(train_data_dir, sort_files) * int(train_epochs),
                         lambda n_node: plan_fixed_batches(n_node, self.train_batch_size), device=device)


class GrevnetDatasetVariable(_ChunkBatches):
    """train_grevnet_with_data.py:183-234: consecutive graphs up to (not reaching) max_nodes per batch."""

    def __init__(self, train_data_dir, max_nodes, sort_files=False, device=None):
        self.max_nodes = int(max_nodes)
        super().__init__(train_data_dir, _chunk_files(train_data_dir, sort_files),
                         lambda n_node: plan_variable_batches(n_node, self.max_nodes), device=device)


def transform_example(node_embeddings, n_node, device=None):
    """train_grevnet_with_data.py:237-271: a (node_embeddings, n_node) batch -> GraphsTuple with the complete
    topology incl. self loops (utils.py:164-183), n_edge = n_node**2, zero edges / globals."""
    import torch
    from .graphs import GraphsTuple
    n_node = np.asarray(n_node, np.int32)
    s, r, n_edge = senders_receivers(n_node)
    g = GraphsTuple(nodes=torch.as_tensor(np.asarray(node_embeddings, np.float32)),
                    edges=torch.zeros(len(s), dtype=torch.float32),
                    receivers=torch.as_tensor(r.astype(np.int32)), senders=torch.as_tensor(s.astype(np.int32)),
                    globals=torch.zeros(len(n_node), dtype=torch.float32),
                    n_node=torch.as_tensor(n_node), n_edge=torch.as_tensor(n_edge.astype(np.int32)))
    return g.to(device) if device is not None else g


def complete_batch(node_embeddings, n_node, device):
    """transform_example's GraphsTuple through gnf_complete_batch (include/gnf_batches.h): node offsets, n_edge = n_node**2,
    senders and receivers in senders_receivers' sender-major order and the row pointers are written by one launch from the B
    node counts - nothing of size sum(n_node**2) is built on the host or uploaded, and no gnf_build_csr runs: for this topology
    the by-receiver col, the by-sender col and `receivers` are one array and the two rowptrs are equal, so both CSR cache entries
    are seeded with col = the receivers tensor itself (and the node-offset cache with the offsets of the same launch).
    node_embeddings: [sum(n_node), D]; a tensor already on `device` is used as it is.  n_node: host integers."""
    import torch
    from . import _abi
    from .graphs import Csr, GraphsTuple, seed_csr_cache, seed_node_offsets_cache
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _abi.GnfError("complete_batch needs a HIP device; there is no CPU path (transform_example is the host route)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    counts = np.asarray(n_node, np.int64).reshape(-1)
    if len(counts) and counts.min() < 0:
        raise ValueError("complete_batch: negative n_node")
    b, n, e = len(counts), int(counts.sum()), int((counts * counts).sum())
    if isinstance(node_embeddings, torch.Tensor):
        nodes = node_embeddings if node_embeddings.device == dev else node_embeddings.to(dev)
    else:
        nodes = torch.as_tensor(np.asarray(node_embeddings, np.float32)).to(dev)
    if nodes.shape[0] != n:
        raise ValueError(f"complete_batch: {nodes.shape[0]} embedding rows for {n} nodes")
    lib = _abi.lib()
    ws_bytes = lib.gnf_complete_batch_workspace_bytes(b)
    live = b > 0 and n > 0
    fits = e <= 2 ** 31 - 1        # beyond: the call refuses (GNF_ESHAPE) before it touches anything
    offsets, n_edge, rowptr, snd, rcv, ws = _int32_arena([b + 1, b, n + 1, e if fits else 0, e if fits else 0,
                                                          (ws_bytes + 3) // 4 + 1], dev, zero=not live)
    n_dev = torch.as_tensor(counts.astype(np.int32)).to(dev)
    with torch.cuda.device(dev):
        _abi.check(lib.gnf_complete_batch(_abi.ptr(n_dev), b, n, e, _abi.ptr(offsets), _abi.ptr(n_edge), _abi.ptr(rowptr),
                                          _abi.ptr(snd), _abi.ptr(rcv), _abi.ptr(ws), ws_bytes, _abi.stream_ptr(dev)),
                   "gnf_complete_batch")
    graph = GraphsTuple(nodes=nodes, edges=torch.zeros(e, dtype=torch.float32, device=dev), receivers=rcv, senders=snd,
                        globals=torch.zeros(b, dtype=torch.float32, device=dev), n_node=n_dev, n_edge=n_edge)
    csr = Csr(rowptr, rcv, n, e)
    seed_csr_cache(graph, csr)
    seed_csr_cache(graph, csr, by_sender=True)
    seed_node_offsets_cache(graph, offsets)
    return graph
