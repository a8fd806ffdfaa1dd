"""numpy reference for the batch-assembly entry points (include/gnf_batches.h), built from the package's existing host
functions only - graphs.graphs_tuple_from_edge_lists, graphs.build_csr_host, datasets.senders_receivers - plus the dataset
the tests assemble from.

Two statements per entry point, held against each other in tests/test_batches_cpu.py:
  host_route / complete_host_route   what the parent route computes: assemble the batch on the host, then sort it twice.
  cut_and_rebase / complete_closed_form   what the kernels compute: cut the dataset-wide CSRs and shift them; n_node
                                          arithmetic.
Every array is int32 except where noted; a result is the dict of the entry point's outputs under the header's names."""
import numpy as np

from gnf_amd.datasets import EdgeListDataset, senders_receivers
from gnf_amd.graphs import build_csr_host, graphs_tuple_from_edge_lists

ASSEMBLE_KEYS = ("n_node", "n_edge", "node_offsets", "senders", "receivers", "rowptr", "col", "rowptr_t", "col_t")
COMPLETE_KEYS = ("node_offsets", "n_edge", "rowptr", "senders", "receivers")
IDS_MIXED = [3, 3, 0, 6, 5, 1, 4, 2, 3]             # repeats, any order, the edgeless / loop-only / complete graphs among them
COMPLETE_SIZES = [1, 2, 17, 64, 65, 1, 33]
COMPLETE_GRID = [361]
COMPLETE = 2      # position of the complete 65-node graph in dataset(): a 2-node graph in front, the edgeless one behind
EDGELESS = 3
LOOP_ONLY = 5


def _random_graph(rng, n):
    """3 n + 2 directed edges drawn with replacement (multi-edges, self loops, both or one direction), any order"""
    e = 3 * n + 2
    return rng.integers(0, n, size=e).astype(np.int32), rng.integers(0, n, size=e).astype(np.int32)


def dataset():
    """Ten graphs: 1, 2, 17, 64, 65, 33 and 5 nodes with random directed edges (multi-edges included), one graph of 4 nodes
    without any edge, one of 3 nodes whose only edge is a self loop, and one complete 65-node graph (4 225 edges, sender-major)
    between a 2-node and the edgeless graph - so one graph spans several fill workgroups next to tiny neighbours."""
    rng = np.random.default_rng(20240611)
    parts = []
    for n in (1, 2):
        parts.append((n,) + _random_graph(rng, n))
    a = np.arange(65, dtype=np.int32)
    parts.append((65, np.repeat(a, 65), np.tile(a, 65)))
    parts.append((4, np.zeros(0, np.int32), np.zeros(0, np.int32)))
    parts.append((17,) + _random_graph(rng, 17))
    parts.append((3, np.array([1], np.int32), np.array([1], np.int32)))
    for n in (64, 65, 33, 5):
        parts.append((n,) + _random_graph(rng, n))
    ds = EdgeListDataset([p[0] for p in parts], [len(p[1]) for p in parts], np.concatenate([p[1] for p in parts]),
                         np.concatenate([p[2] for p in parts]))
    assert ds.n_node[COMPLETE] == 65 and ds.n_edge[COMPLETE] == 4225 and ds.n_edge[EDGELESS] == 0 and ds.n_edge[LOOP_ONLY] == 1
    return ds


def id_lists(ds):
    """the id lists of the GPU test: none, one, the mixed list, every id in reverse, 64 drawn with repeats"""
    g = len(ds)
    return {"empty": [], "one": [4], "mixed": IDS_MIXED, "reversed": list(range(g))[::-1],
            "drawn64": np.random.default_rng(64).integers(0, g, size=64).tolist()}


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _offsets(n_node):
    return _i32(np.concatenate([[0], np.cumsum(np.asarray(n_node, np.int64))]))


def host_route(ds, ids):
    """graphs_tuple_from_edge_lists, then build_csr_host by receiver and (senders and receivers swapped) by sender"""
    ids = [int(i) for i in ids]
    n = int(sum(int(ds.n_node[i]) for i in ids))
    g = graphs_tuple_from_edge_lists(ds.n_node, ds.n_edge, ds.senders, ds.receivers, ids, np.zeros((n, 1), np.float32))
    s, r = g.senders.numpy(), g.receivers.numpy()
    rowptr, col = build_csr_host(s, r, n)
    rowptr_t, col_t = build_csr_host(r, s, n)
    return dict(n_node=_i32(g.n_node.numpy()), n_edge=_i32(g.n_edge.numpy()), node_offsets=_offsets(g.n_node.numpy()),
                senders=_i32(s), receivers=_i32(r), rowptr=rowptr, col=col, rowptr_t=rowptr_t, col_t=col_t)


def store(ds):
    """the dataset as ONE big batch with dataset-wide node ids, and build_csr_host of it in both orientations"""
    node_off = np.concatenate([[0], np.cumsum(ds.n_node.astype(np.int64))])
    shift = np.repeat(node_off[:-1], ds.n_edge)
    s, r = ds.senders.astype(np.int64) + shift, ds.receivers.astype(np.int64) + shift
    rowptr, col = build_csr_host(s, r, int(node_off[-1]))
    rowptr_t, col_t = build_csr_host(r, s, int(node_off[-1]))
    return dict(node_off=node_off, edge_off=ds.eoff.astype(np.int64), senders=s, receivers=r, rowptr=rowptr.astype(np.int64),
                col=col.astype(np.int64), rowptr_t=rowptr_t.astype(np.int64), col_t=col_t.astype(np.int64))


def cut_and_rebase(ds, ids, st=None):
    """the header's rule: per slot b with graph g, every node id is id - node_off[g] + node_offsets[b], every row start is
    rowptr_all[node_off[g] + i] - edge_off[g] + (edges of the batch in front of b); rowptr[N] = E"""
    st = store(ds) if st is None else st
    ids = np.asarray(ids, np.int64).reshape(-1)
    n_node, n_edge = ds.n_node[ids].astype(np.int64), ds.n_edge[ids].astype(np.int64)
    nb, eb = np.concatenate([[0], np.cumsum(n_node)]), np.concatenate([[0], np.cumsum(n_edge)])
    out = {k: [] for k in ("senders", "receivers", "col", "col_t", "rowptr", "rowptr_t")}
    for b, g in enumerate(ids):
        n0, e0 = st["node_off"][g], st["edge_off"][g]
        for k in ("senders", "receivers", "col", "col_t"):
            out[k].append(st[k][e0:e0 + n_edge[b]] - n0 + nb[b])
        for k in ("rowptr", "rowptr_t"):
            out[k].append(st[k][n0:n0 + n_node[b]] - e0 + eb[b])
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    res = {k: _i32(cat(v)) for k, v in out.items()}
    for k in ("rowptr", "rowptr_t"):
        res[k] = _i32(np.concatenate([res[k], [eb[-1]]]))
    res.update(n_node=_i32(n_node), n_edge=_i32(n_edge), node_offsets=_i32(nb))
    return res


def complete_host_route(n_node):
    """datasets.senders_receivers, then build_csr_host in both orientations: (result, col, rowptr_t, col_t)"""
    n_node = np.asarray(n_node, np.int32).reshape(-1)
    n = int(n_node.sum())
    if len(n_node):
        s, r, n_edge = senders_receivers(n_node)
    else:
        s, r, n_edge = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    rowptr, col = build_csr_host(s, r, n)
    rowptr_t, col_t = build_csr_host(r, s, n)
    res = dict(node_offsets=_offsets(n_node), n_edge=_i32(n_edge), rowptr=rowptr, senders=_i32(s), receivers=_i32(r))
    return res, col, rowptr_t, col_t


def complete_closed_form(n_node):
    """the header's arithmetic: graph b's edge k n_b + l is (off_b + k) -> (off_b + l); rowptr = cumsum(repeat(n_b, n_b))"""
    n = np.asarray(n_node, np.int64).reshape(-1)
    off = np.concatenate([[0], np.cumsum(n)])
    per_edge_graph = np.repeat(np.arange(len(n)), n * n)
    eb = np.concatenate([[0], np.cumsum(n * n)])
    local = np.arange(int(eb[-1])) - eb[per_edge_graph]
    nn = n[per_edge_graph]
    return dict(node_offsets=_i32(off), n_edge=_i32(n * n), rowptr=_i32(np.concatenate([[0], np.cumsum(np.repeat(n, n))])),
                senders=_i32(off[per_edge_graph] + local // np.maximum(nn, 1)),
                receivers=_i32(off[per_edge_graph] + local % np.maximum(nn, 1)))
