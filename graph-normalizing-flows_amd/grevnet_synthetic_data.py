"""Synthetic 2-D datasets of the GRevNet driver (/root/reference/grevnet_synthetic_data.py:14-124): every
example is a fully connected directed graph WITH self loops whose node features are points of two moons
/ a mixture of Gaussians.  Same names, same `SyntheticDataset.get_next_batch_data_dicts(batch_size)` data
dicts (grevnet_synthetic_data.py:28-43); `get_next_batch` returns this package's GraphsTuple (on `device`).
networkx is not needed: the complete digraph's edge list is written directly, in networkx's edge order
(complete_graph(create_using=DiGraph) + add_edges_from(zip(r, r)): adjacency iteration, self loop last in
every row)."""
import functools
import random
from functools import partial

import numpy as np

from .graphs import data_dicts_to_graphs_tuple

MAX_SEED = 2 ** 32 - 1
GAUSSIAN_MEAN = [0, 0]
GAUSSIAN_COV = [[1, 0], [0, 1]]


@functools.lru_cache(maxsize=64)
def _fully_connected_edge_list(num_nodes):
    m = np.arange(num_nodes, dtype=np.int32)
    grid = np.tile(m, (num_nodes, 1))
    off_diag = grid[grid != m[:, None]].reshape(num_nodes, num_nodes - 1)
    receivers = np.concatenate([off_diag, m[:, None]], axis=1).ravel()      # the self loop was added last
    senders = np.repeat(m, num_nodes)
    senders.setflags(write=False)
    receivers.setflags(write=False)
    return senders, receivers


def fully_connected_edge_list(num_nodes):
    """Edges of fully_connected_nx_graph (grevnet_synthetic_data.py:17-21) in `g.edges()` order: for every node u
    its out-edges to v != u ascending, then the self loop (cached per size; read-only arrays)."""
    return _fully_connected_edge_list(int(num_nodes))


class SyntheticDataset:
    def __init__(self, graph_generator_fn):
        self.graph_generator_fn = graph_generator_fn

    def get_next_batch_data_dicts(self, batch_size):
        data_dicts = []
        for _ in range(batch_size):
            num_nodes, node_features = self.graph_generator_fn()
            s, r = fully_connected_edge_list(num_nodes)
            data_dicts.append({"n_node": num_nodes, "n_edge": len(s), "senders": s, "receivers": r,
                               "nodes": node_features, "globals": 0, "edges": np.zeros(len(s))})
        return data_dicts

    def get_next_batch(self, batch_size, device=None):
        return data_dicts_to_graphs_tuple(self.get_next_batch_data_dicts(batch_size), device)


@functools.lru_cache(maxsize=None)
def _moons_template(n_samples):
    """The noise-free, unshuffled point set of sklearn.datasets.make_moons(n_samples): outer half circle first,
    then the inner one (read-only [n, 2] float64)."""
    n_out = n_samples // 2
    n_in = n_samples - n_out
    t_out, t_in = np.linspace(0, np.pi, n_out), np.linspace(0, np.pi, n_in)
    x = np.vstack([np.append(np.cos(t_out), 1 - np.cos(t_in)), np.append(np.sin(t_out), 1 - np.sin(t_in) - 0.5)]).T
    x.setflags(write=False)
    return x


def make_moons(n_samples, noise, seed):
    """sklearn.datasets.make_moons(n_samples, shuffle=True, noise=noise, random_state=seed)[0], restated: the same
    point set, the same RandomState draws in the same order (one shuffle of arange(n), then one normal(scale=noise)
    of shape [n, 2]) - identical arrays (tests/test_host_logic_cpu.py checks against sklearn), without sklearn's
    parameter validation, which cost 1 ms per graph (32 graphs per batch: more host time than the GPU needs for the
    whole training iteration)."""
    rs = np.random.RandomState(seed)
    idx = np.arange(n_samples)
    rs.shuffle(idx)
    x = _moons_template(int(n_samples))[idx]
    if noise is not None:
        x += rs.normal(scale=noise, size=x.shape)
    return x


def moons_sample(n_samples, noise=0.05):
    # grevnet_synthetic_data.py:50-56: make_moons(..., random_state=random.randrange(MAX_SEED))[0].astype(np.float32)
    return n_samples, make_moons(n_samples, noise, random.randrange(MAX_SEED)).astype(np.float32)


def mom_sample(n_samples_choices, noise=0.05):
    return moons_sample(int(np.random.choice(n_samples_choices)), noise=noise)


def mog_sample(offsets_choices, rotate=False):
    offsets = random.choice(offsets_choices).copy()
    num_nodes = len(offsets)
    np.random.shuffle(offsets)
    features = np.random.multivariate_normal(GAUSSIAN_MEAN, GAUSSIAN_COV, num_nodes).astype(np.float32) + offsets
    if rotate:
        angle = np.random.random() * np.pi
        rot_mat = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
        features = np.transpose(np.matmul(rot_mat, np.transpose(features))).astype(np.float32)
    return num_nodes, features


OFFSETS_4 = np.array([[-5, 5], [5, 5], [-5, -5], [5, -5]]).astype(np.float32)
OFFSETS_6 = np.array([[-5, 5], [5, 5], [-5, -5], [5, -5], [15, 5], [15, -5]]).astype(np.float32)
OFFSETS_9 = np.array([[-5, 5], [5, 5], [-5, -5], [5, -5], [15, 5], [15, -5], [-5, 15], [5, 15],
                      [15, 15]]).astype(np.float32)

DATASETS_MAP = {
    "moons_100": SyntheticDataset(partial(moons_sample, n_samples=100)),
    "moons_10": SyntheticDataset(partial(moons_sample, n_samples=10)),
    "moons_6": SyntheticDataset(partial(moons_sample, n_samples=6)),
    "mom_6_10": SyntheticDataset(partial(mom_sample, n_samples_choices=[6, 10])),
    "mom_6_10_20": SyntheticDataset(partial(mom_sample, n_samples_choices=[6, 10, 20])),
    "mog_4": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_4])),
    "mog_6": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_6])),
    "mog_9": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_9])),
    "mog_4_rotate": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_4], rotate=True)),
    "mog_4_6": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_4, OFFSETS_6])),
    "mog_4_9": SyntheticDataset(partial(mog_sample, offsets_choices=[OFFSETS_4, OFFSETS_9])),
}


# ----------------------------------------------------------------------------------------------
# The same datasets as ready batches made on the device (include/gnf_synthetic.h).  Opt-in: everything above is unchanged.
# ----------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
SYN_STREAM_KEY, SYN_STREAM_U1, SYN_STREAM_U2, SYN_STREAM_ANGLE, SYN_STREAM_CHOICE = range(5)


def _u64(v):
    if isinstance(v, (int, np.integer)):
        v = int(v) & _M64
    return np.atleast_1d(np.asarray(v, dtype=np.uint64))


def _mix64(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def synthetic_draw(seed, graph, index, stream):
    """gnf_syn_draw of include/gnf_synthetic.h in numpy (wrapping uint64 arrays; the arguments broadcast): uint32 draws."""
    one = np.uint64(1)
    seed, graph, index, stream = _u64(seed), _u64(graph), _u64(index), _u64(stream)
    x = _mix64(seed + np.uint64(0x9E3779B97F4A7C15) * (graph + one))
    x = _mix64(x ^ (np.uint64(0xBF58476D1CE4E5B9) * (index + one)))
    x = _mix64(x ^ (np.uint64(0x94D049BB133111EB) * (stream + one)))
    return (x >> np.uint64(32)).astype(np.uint32)


def synthetic_choice(seed, n_graphs, n_choices):
    """choice[b] = (draw(seed, b, 0, 4) * n_choices) >> 32 for b in [0, n_graphs): int64 in [0, n_choices)."""
    d = synthetic_draw(seed, np.arange(n_graphs, dtype=np.uint64), 0, SYN_STREAM_CHOICE).astype(np.uint64)
    return ((d * np.uint64(n_choices)) >> np.uint64(32)).astype(np.int64)


class SyntheticSpec:
    """What a dataset name means to the generator: kind "moons" (sizes = the n_samples choices, noise) or "mog" (offset_sets =
    the offsets choices, rotate).  A graph's size is its choice of `sizes`, or the size of its chosen offset set."""

    def __init__(self, kind, sizes=(), noise=0.05, offset_sets=(), rotate=False):
        self.kind, self.noise, self.rotate = kind, float(noise), bool(rotate)
        self.offset_sets = [np.asarray(o, np.float32).reshape(-1, 2) for o in offset_sets]
        self.sizes = [int(s) for s in sizes] if kind == "moons" else [len(o) for o in self.offset_sets]
        if kind not in ("moons", "mog") or not self.sizes:
            raise ValueError(f"SyntheticSpec: kind={kind!r} with {len(self.sizes)} choices")

    @property
    def n_choices(self):
        return len(self.sizes)

    @property
    def fixed_size(self):
        return len(self.sizes) == 1

    def choose(self, batch_size, seed):
        """(n_node int32 [B], set_id int32 [B]) of the batch with this seed; set_id is all zeros for moons."""
        c = synthetic_choice(seed, batch_size, self.n_choices)
        n_node = np.asarray(self.sizes, np.int32)[c]
        return n_node, (c.astype(np.int32) if self.kind == "mog" else np.zeros(batch_size, np.int32))


SYNTHETIC_SPECS = {
    "moons_100": SyntheticSpec("moons", [100]),
    "moons_10": SyntheticSpec("moons", [10]),
    "moons_6": SyntheticSpec("moons", [6]),
    "mom_6_10": SyntheticSpec("moons", [6, 10]),
    "mom_6_10_20": SyntheticSpec("moons", [6, 10, 20]),
    "mog_4": SyntheticSpec("mog", offset_sets=[OFFSETS_4]),
    "mog_6": SyntheticSpec("mog", offset_sets=[OFFSETS_6]),
    "mog_9": SyntheticSpec("mog", offset_sets=[OFFSETS_9]),
    "mog_4_rotate": SyntheticSpec("mog", offset_sets=[OFFSETS_4], rotate=True),
    "mog_4_6": SyntheticSpec("mog", offset_sets=[OFFSETS_4, OFFSETS_6]),
    "mog_4_9": SyntheticSpec("mog", offset_sets=[OFFSETS_4, OFFSETS_9]),
}


def synthetic_topology_host(n_node):
    """The index arrays of include/gnf_synthetic.h's TOPOLOGY from the counts alone (a negative count is 0), written from its
    formulas: node_offsets, n_edge, senders, receivers, rowptr, col - all int32."""
    n_node = np.maximum(np.asarray(n_node, np.int64).reshape(-1), 0)
    offs = np.concatenate([[0], np.cumsum(n_node)])
    snd, rcv, col, rowptr = [], [], [], []
    e0 = 0
    for o, n in zip(offs[:-1], n_node):
        k, p = np.divmod(np.arange(n * n, dtype=np.int64), max(n, 1))
        snd.append(o + k)
        rcv.append(o + np.where(p == n - 1, k, p + (p >= k)))
        col.append(o + p)
        rowptr.append(e0 + np.arange(n, dtype=np.int64) * n)
        e0 += n * n
    cat = lambda xs: np.concatenate(xs + [np.zeros(0, np.int64)]).astype(np.int32)
    return {"node_offsets": offs.astype(np.int32), "n_edge": (n_node * n_node).astype(np.int32), "senders": cat(snd),
            "receivers": cat(rcv), "col": cat(col), "rowptr": cat(rowptr + [np.asarray([e0])])}


def synthetic_batch_host(spec, n_node, set_id, seed):
    """The float64 restatement of include/gnf_synthetic.h: every array the device route returns - "nodes" (float64 [N, 2]),
    "source", "n_node", and synthetic_topology_host's - for the counts n_node, the offset sets set_id (None: set 0) and `seed`."""
    n_node = np.maximum(np.asarray(n_node, np.int64).reshape(-1), 0)
    out = synthetic_topology_host(n_node)
    nodes, source = [], []
    for b, n in enumerate(n_node):
        i = np.arange(n, dtype=np.uint64)
        idx = np.argsort(synthetic_draw(seed, b, i, SYN_STREAM_KEY), kind="stable")
        u1 = ((synthetic_draw(seed, b, i, SYN_STREAM_U1) >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (synthetic_draw(seed, b, i, SYN_STREAM_U2) >> 8).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1)
        if spec.kind == "moons":
            n_out = int(n) // 2
            n_in = int(n) - n_out
            t_out = np.pi * np.arange(n_out) / max(n_out - 1, 1)
            t_in = np.pi * np.arange(n_in) / max(n_in - 1, 1)
            tmpl = np.stack([np.append(np.cos(t_out), 1.0 - np.cos(t_in)), np.append(np.sin(t_out), 0.5 - np.sin(t_in))], axis=1)
            x = tmpl[idx] + spec.noise * z if spec.noise != 0.0 else tmpl[idx]
        else:
            offs = spec.offset_sets[int(set_id[b]) if set_id is not None else 0].astype(np.float64)
            padded = np.zeros((max(int(n), len(offs)), 2))
            padded[:len(offs)] = offs
            x = z + padded[idx]
            if spec.rotate:
                a = float(synthetic_draw(seed, b, 0, SYN_STREAM_ANGLE)[0] >> 8) * 2.0 ** -24 * np.pi
                x = np.stack([x[:, 0] * np.cos(a) - x[:, 1] * np.sin(a), x[:, 0] * np.sin(a) + x[:, 1] * np.cos(a)], axis=1)
        nodes.append(x.reshape(-1, 2))
        source.append(idx.astype(np.int32))
    out["nodes"] = np.concatenate(nodes + [np.zeros((0, 2))], axis=0)
    out["source"] = np.concatenate(source + [np.zeros(0, np.int32)])
    out["n_node"] = n_node.astype(np.int32)
    return out


class DeviceSyntheticDataset:
    """A DATASETS_MAP dataset whose batches are made where they are used (include/gnf_synthetic.h): get_next_batch(batch_size)
    returns a GraphsTuple on `device` with both CSR cache entries and the node-offset cache seeded, so that no gnf_build_csr
    runs for it; nothing is uploaded per batch but the B node counts (and set ids), and those only for the datasets whose
    graphs vary in size.  Batch t (counted from 0) uses seed + t.  `.last_source` is the `source` tensor of the last batch:
    which template point / mixture component every node came from.
    Fixed-size datasets (moons_*, single-set mog_*) build the topology once per batch size and hand the SAME index tensors (and
    the same all-zero edges / globals tensors) to every batch: per batch only gnf_synthetic_nodes runs.  Do not edit them in
    place.  The others (mom_*, mog_4_6, mog_4_9) run gnf_synthetic_topology per batch.
    The random stream is the header's hash, not numpy's: same distributions as DATASETS_MAP[name], other numbers.
    device="cpu": the same batches from synthetic_batch_host (float64 arithmetic, rounded once to float32), no cache seeded."""

    def __init__(self, name, device, seed=12345):
        import torch
        self.name, self.spec = name, SYNTHETIC_SPECS[name]
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.seed, self.batches_made, self.last_source = int(seed), 0, None
        self._fixed = {}           # batch size -> the topology tensors of a fixed-size dataset
        self._offsets_dev = None
        if self.spec.kind == "mog" and self.device.type == "cuda":
            stride = max(self.spec.sizes)
            table = np.zeros((len(self.spec.offset_sets), stride, 2), np.float32)
            for q, o in enumerate(self.spec.offset_sets):
                table[q, :len(o)] = o
            self._offsets_dev = torch.from_numpy(table).to(self.device)

    def _topology(self, n_node, set_id):
        import torch
        from . import _abi
        from .datasets import _int32_arena
        dev = self.device
        b, n, e = len(n_node), int(n_node.sum()), int((n_node.astype(np.int64) ** 2).sum())
        if dev.type != "cuda":
            t = {k: torch.from_numpy(v) for k, v in synthetic_topology_host(n_node).items()}
            t.update(n_node=torch.from_numpy(n_node.copy()), set_id=None)
        else:
            lib = _abi.lib()
            ws_bytes = lib.gnf_synthetic_topology_workspace_bytes(b)
            live = b > 0 and n > 0
            counts, offsets, n_edge, rowptr, snd, rcv, col, ws = _int32_arena(
                [2 * b, b + 1, b, n + 1, e, e, e, (ws_bytes + 3) // 4 + 1], dev, zero=not live)
            counts.copy_(torch.from_numpy(np.concatenate([n_node, set_id]).astype(np.int32)))   # the batch's only upload
            with torch.cuda.device(dev):
                _abi.check(lib.gnf_synthetic_topology(_abi.ptr(counts), b, n, e, _abi.ptr(offsets), _abi.ptr(n_edge),
                                                      _abi.ptr(rowptr), _abi.ptr(snd), _abi.ptr(rcv), _abi.ptr(col), _abi.ptr(ws),
                                                      ws_bytes, _abi.stream_ptr(dev)), "gnf_synthetic_topology")
            t = dict(n_node=counts[:b], set_id=counts[b:], node_offsets=offsets, n_edge=n_edge, rowptr=rowptr, senders=snd,
                     receivers=rcv, col=col)
        t.update(edges=torch.zeros(e, dtype=torch.float32, device=dev), globals=torch.zeros(b, dtype=torch.float32, device=dev),
                 sizes=(b, n, e))
        return t

    def get_next_batch(self, batch_size, device=None):
        import ctypes as C
        import torch
        from . import _abi
        from .graphs import Csr, GraphsTuple, seed_csr_cache, seed_node_offsets_cache
        if device is not None and torch.device(device).type != self.device.type:
            raise ValueError(f"DeviceSyntheticDataset lives on {self.device}, not on {device}")
        spec, dev = self.spec, self.device
        seed = (self.seed + self.batches_made) & _M64
        self.batches_made += 1
        n_node, set_id = spec.choose(int(batch_size), seed)
        topo = self._fixed.get(int(batch_size)) if spec.fixed_size else None
        if topo is None:
            topo = self._topology(n_node, set_id)
            if spec.fixed_size:
                self._fixed[int(batch_size)] = topo
        b, n, e = topo["sizes"]
        if dev.type != "cuda":
            host = synthetic_batch_host(spec, n_node, set_id, seed)
            nodes = torch.from_numpy(host["nodes"].astype(np.float32))
            self.last_source = torch.from_numpy(host["source"])
        else:
            nodes = torch.empty(n, 2, dtype=torch.float32, device=dev)
            self.last_source = torch.empty(n, dtype=torch.int32, device=dev)
            cspec = _abi.GnfSyntheticSpec()
            cspec.seed, cspec.seed_dev = seed, None
            cspec.kind = _abi.GNF_SYN_MOONS if spec.kind == "moons" else _abi.GNF_SYN_MOG
            cspec.rotate, cspec.noise = int(spec.rotate), spec.noise
            if spec.kind == "mog":
                cspec.offsets, cspec.n_sets = self._offsets_dev.data_ptr(), len(spec.sizes)
                cspec.set_stride = int(self._offsets_dev.shape[1])
                for q, s in enumerate(spec.sizes):
                    cspec.set_size[q] = s
            with torch.cuda.device(dev):
                _abi.check(_abi.lib().gnf_synthetic_nodes(C.byref(cspec), _abi.ptr(topo["n_node"]), _abi.ptr(topo["set_id"]),
                                                          _abi.ptr(topo["node_offsets"]), b, n, max(max(spec.sizes), 1),
                                                          _abi.ptr(nodes), 2, _abi.ptr(self.last_source), _abi.stream_ptr(dev)),
                           "gnf_synthetic_nodes")
        graph = GraphsTuple(nodes=nodes, edges=topo["edges"], receivers=topo["receivers"], senders=topo["senders"],
                            globals=topo["globals"], n_node=topo["n_node"], n_edge=topo["n_edge"])
        if dev.type == "cuda":
            # one rowptr for both orientations; `receivers` is the by-sender col (the header's array identity)
            seed_csr_cache(graph, Csr(topo["rowptr"], topo["col"], n, e))
            seed_csr_cache(graph, Csr(topo["rowptr"], topo["receivers"], n, e), by_sender=True)
            seed_node_offsets_cache(graph, topo["node_offsets"])
        return graph
