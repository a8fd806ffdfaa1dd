"""numpy reference of gnf_amd.graph_stats.graph_components / keep_subgraphs: a union-find on the undirected simple graph an edge
list stands for, the six outputs of include/gnf_graph_components.h, the induced-subgraph edge lists in the order that header
defines, and the cases the GPU tests run.  Reads nothing but its arguments."""
import numpy as np

import graph_stats_ref as S

KEYS = ("component", "component_size", "n_components", "largest_component_size", "largest_component_root", "n_isolated")
RULES = ("largest_component", "non_isolated")


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def _simple_pairs(n_node, senders, receivers):
    """(off, unordered pairs i < j inside one graph, each once): self loops dropped, duplicates and directions merged"""
    off = np.concatenate([[0], np.cumsum([int(v) for v in n_node])]).astype(np.int64)
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    gs, gr = np.searchsorted(off, s, side="right") - 1, np.searchsorted(off, r, side="right") - 1
    ok = (s != r) & (gs == gr)
    lo, hi = np.minimum(s[ok], r[ok]), np.maximum(s[ok], r[ok])
    pairs = np.unique(np.stack([lo, hi], 1), axis=0) if len(lo) else np.zeros((0, 2), np.int64)
    return off, pairs


def components(n_node, senders, receivers):
    """Batch-wide edge list (global node ids) -> the dict graph_components returns, as numpy int32 arrays."""
    off, pairs = _simple_pairs(n_node, senders, receivers)
    n, b = int(off[-1]), len(n_node)
    parent = list(range(n))
    for i, j in pairs.tolist():
        a, c = _find(parent, i), _find(parent, j)
        if a != c:
            parent[max(a, c)] = min(a, c)      # the smaller index stays the root: NORMATIVE label = smallest node
    comp = np.array([_find(parent, i) for i in range(n)], np.int64).reshape(n)
    size = np.bincount(comp, minlength=n)[comp] if n else np.zeros(0, np.int64)
    deg = np.bincount(pairs.ravel(), minlength=n) if n else np.zeros(0, np.int64)
    out = {"component": comp.astype(np.int32), "component_size": size.astype(np.int32),
           "n_components": np.zeros(b, np.int32), "largest_component_size": np.zeros(b, np.int32),
           "largest_component_root": np.full(b, -1, np.int32), "n_isolated": np.zeros(b, np.int32)}
    for g in range(b):
        a, e = int(off[g]), int(off[g + 1])
        if e == a:
            continue
        roots = np.flatnonzero(comp[a:e] == np.arange(a, e)) + a
        sizes = size[roots]
        out["n_components"][g] = len(roots)
        out["largest_component_size"][g] = sizes.max()
        out["largest_component_root"][g] = roots[np.argmax(sizes)]      # argmax: the first maximum = the smallest root
        out["n_isolated"][g] = int((deg[a:e] == 0).sum())
    return out


def keep_mask(n_node, senders, receivers, rule, mask=None):
    """bool [N]: the nodes a rule keeps ("largest_component", "non_isolated", or "mask" with a [N] array)"""
    off, pairs = _simple_pairs(n_node, senders, receivers)
    n = int(off[-1])
    if rule == "mask":
        return np.asarray(mask).astype(bool).reshape(n)
    if rule == "non_isolated":
        return np.bincount(pairs.ravel(), minlength=n)[:n] > 0 if n else np.zeros(0, bool)
    assert rule == "largest_component"
    c = components(n_node, senders, receivers)
    gid = np.repeat(np.arange(len(n_node)), [int(v) for v in n_node])
    return c["component"] == c["largest_component_root"][gid]


def subgraph(n_node, senders, receivers, keep, self_loops=False):
    """The induced subgraph batch of include/gnf_graph_components.h: kept nodes renumbered in ascending old order, both
    directions of every simple edge, receivers ascending and senders ascending within a receiver, the loop (self_loops) on every
    kept node at its sorted place."""
    off, pairs = _simple_pairs(n_node, senders, receivers)
    n, b = int(off[-1]), len(n_node)
    keep = np.asarray(keep, bool).reshape(n)
    node_index = np.flatnonzero(keep)
    new_id = np.full(n, -1, np.int64)
    new_id[node_index] = np.arange(len(node_index))
    kept = pairs[keep[pairs[:, 0]] & keep[pairs[:, 1]]] if len(pairs) else pairs
    s = np.concatenate([new_id[kept[:, 0]], new_id[kept[:, 1]]])
    r = np.concatenate([new_id[kept[:, 1]], new_id[kept[:, 0]]])
    if self_loops:
        loops = np.arange(len(node_index))
        s, r = np.concatenate([s, loops]), np.concatenate([r, loops])
    order = np.lexsort((s, r))
    s, r = s[order], r[order]
    rowptr = np.zeros(len(node_index) + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=len(node_index)), out=rowptr[1:])
    gid = np.repeat(np.arange(b), [int(v) for v in n_node])
    new_n_node = np.bincount(gid[node_index], minlength=b)
    n_edge = np.bincount(gid[node_index[r]], minlength=b) if len(r) else np.zeros(b, np.int64)
    i32 = lambda x: np.asarray(x).astype(np.int32)
    return {"new_id": i32(new_id), "node_index": i32(node_index), "new_n_node": i32(new_n_node), "n_edge": i32(n_edge),
            "rowptr": i32(rowptr), "senders": i32(s), "receivers": i32(r)}


# ---- graph builders (local ids, one direction per edge) --------------------------------------------------------------------
def path(n):
    i = np.arange(max(n - 1, 0))
    return i, i + 1


def path_reversed(n):
    """the same path written from the far end: every edge points the other way, the last edge first"""
    s, r = path(n)
    return r[::-1].copy(), s[::-1].copy()


def path_folded(n):
    """a path whose node 0 sits in the middle: positions ..., 5, 3, 1, 0, 2, 4, ... - the search from the root runs both ways and
    crosses the word boundaries out of step"""
    odd, even = np.arange(1, n, 2)[::-1], np.arange(0, n, 2)
    order = np.concatenate([odd, even])
    return order[:-1].copy(), order[1:].copy()


def star_hub_last(n):
    return np.full(n - 1, n - 1, np.int64), np.arange(n - 1)


def single_edge(n, i, j):
    return np.array([i]), np.array([j])


def tie():
    """{0, 1} (the smallest root, but smaller), {2, 4, 6} and {3, 5, 7} (equal sizes: root 2 wins), 8 isolated"""
    return np.array([0, 2, 4, 3, 5]), np.array([1, 4, 6, 5, 7])


def no_edges(n):
    return np.zeros(0, np.int64), np.zeros(0, np.int64)


def sparse(n, rng, mean_degree=1.2):
    """G(n, mean_degree / n): below the giant-component threshold side by side with isolated nodes and small trees"""
    return S.gnp(n, min(1.0, mean_degree / max(n, 1)), rng) if n > 1 else no_edges(n)


def word_edge_cases():
    """[(name, n, (s, r))]: sizes on both sides of the 64-bit word edges in one batch, an empty graph in the middle and one at
    the end"""
    rng = np.random.default_rng(6465)
    sizes = [1, 2, 63, 64, 0, 65, 128, 129, 0]
    return [(f"sparse{n}" if n else "empty", n, S.complete(2) if n == 2 else sparse(n, rng)) for n in sizes]


def hazard_cases():
    """[(name, n, (s, r))]: one case per hazard of the search and of the tie rule"""
    return [("path130", 130, path(130)), ("path130_reversed", 130, path_reversed(130)), ("path130_folded", 130, path_folded(130)),
            ("star70_hub_last", 70, star_hub_last(70)), ("edge_63_64", 65, single_edge(65, 63, 64)), ("tie", 9, tie()),
            ("isolated70", 70, no_edges(70)), ("empty", 0, no_edges(0)), ("K65", 65, S.complete(65))]


def all_cases():
    return word_edge_cases() + hazard_cases()


def stride_lattice(n, rng, stride=64, p_keep=0.9, p_link=0.004):
    """i - i + stride for nine nodes in ten, i - i + 1 for a few: every edge of the first kind joins the same column of two
    neighbouring 64-bit words, so a search moves through ALL words of the graph, and the rare links merge some of the
    `stride` residue classes - components of many sizes, isolated nodes, roots anywhere in the first rows"""
    i = np.arange(n - stride)
    i = i[rng.random(len(i)) < p_keep]
    j = np.arange(n - 1)
    j = j[rng.random(len(j)) < p_link]
    return np.concatenate([i, j]), np.concatenate([i + stride, j + 1])


def large_cases():
    """[(name, n, (s, r))]: graphs of more than 64 words (4 200 nodes: the frontier no longer fits one 64-lane read) and of more
    than 256 words (16 500 nodes: a thread owns more than one word), a small graph between them"""
    rng = np.random.default_rng(16500)
    return [("lattice4200", 4200, stride_lattice(4200, rng)), ("tie", 9, tie()), ("lattice16500", 16500, stride_lattice(16500, rng))]


def batch(cases):
    return S.batch([(n, e) for _, n, e in cases])
