"""Brute-force Python-int reference of gnf_amd.graph_stats.graph_orbits / orbit_mmd: the definitions of include/gnf_graph_orbits.h spelled
out by enumeration.  Every connected induced subgraph on 2, 3 and 4 nodes is found by growing node sets one neighbour at a
time from every single node, then classified by (number of nodes, number of edges, degree sequence, the node's own degree
inside it) - Przulj's orbits 0..14, the numbering ORCA uses.  Nothing here knows a relation between orbit counts: it is an
independent statement of what the kernel must produce.  The vector MMD is an explicit double loop in float64.  Reads nothing
but its arguments."""
import numpy as np

from graph_stats_ref import dense_adjacency

N_ORBITS = 15
# (nodes, edges, sorted degree sequence) -> graphlet name;  (graphlet, own degree) -> orbit
GRAPHLETS = {(2, 1, (1, 1)): "edge", (3, 2, (1, 1, 2)): "path3", (3, 3, (2, 2, 2)): "triangle",
             (4, 3, (1, 1, 2, 2)): "path4", (4, 3, (1, 1, 1, 3)): "star4", (4, 4, (2, 2, 2, 2)): "cycle4",
             (4, 4, (1, 2, 2, 3)): "tailed_triangle", (4, 5, (2, 2, 3, 3)): "chorded_cycle", (4, 6, (3, 3, 3, 3)): "complete4"}
ORBIT = {("edge", 1): 0, ("path3", 1): 1, ("path3", 2): 2, ("triangle", 2): 3, ("path4", 1): 4, ("path4", 2): 5,
         ("star4", 1): 6, ("star4", 3): 7, ("cycle4", 2): 8, ("tailed_triangle", 1): 9, ("tailed_triangle", 2): 10,
         ("tailed_triangle", 3): 11, ("chorded_cycle", 2): 12, ("chorded_cycle", 3): 13, ("complete4", 3): 14}
# nodes of a graphlet per orbit: inside one graphlet the column sums over a graph stand in these ratios
ORBIT_SIZE = {0: 2, 1: 2, 2: 1, 3: 3, 4: 2, 5: 2, 6: 3, 7: 1, 8: 4, 9: 1, 10: 2, 11: 1, 12: 2, 13: 2, 14: 4}


def _bits(mask):
    while mask:
        low = mask & -mask
        yield low.bit_length() - 1
        mask ^= low


def connected_subsets(a, sizes=(2, 3, 4)):
    """Node tuples of every connected induced subgraph of the dense boolean adjacency `a` with 2, 3 or 4 nodes, each once."""
    n = len(a)
    adj = [sum(1 << j for j in np.flatnonzero(a[i]).tolist()) for i in range(n)]
    level = {1 << v for v in range(n)}
    out = []
    for size in range(2, max(sizes) + 1):
        grown = set()
        for s in level:
            border = 0
            for u in _bits(s):
                border |= adj[u]
            for u in _bits(border & ~s):
                grown.add(s | (1 << u))
        level = grown
        if size in sizes:
            out.extend(tuple(_bits(s)) for s in level)
    return out


def classify(a, nodes):
    """(graphlet name, degrees of `nodes` inside the induced subgraph)"""
    deg = [sum(1 for v in nodes if a[u][v]) for u in nodes]
    return GRAPHLETS[(len(nodes), sum(deg) // 2, tuple(sorted(deg)))], deg


def node_orbits(a):
    """int64 [n, 15] orbit counts of a dense boolean adjacency (symmetric, zero diagonal)."""
    a = np.asarray(a, bool)
    rows = [row.tolist() for row in a]
    out = [[0] * N_ORBITS for _ in range(len(a))]
    for nodes in connected_subsets(a):
        name, deg = classify(rows, nodes)
        for u, d in zip(nodes, deg):
            out[u][ORBIT[(name, d)]] += 1
    return np.asarray(out, np.int64).reshape(len(a), N_ORBITS)


def graph_orbits(n_node, senders, receivers):
    """Batch-wide edge list (global ids; graph of an edge = graph of its receiver) -> the dict graph_orbits returns."""
    n_node = [int(v) for v in n_node]
    b, n = len(n_node), sum(n_node)
    off = np.concatenate([[0], np.cumsum(n_node)]).astype(np.int64)
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    gid = np.searchsorted(off, r, side="right") - 1
    out = {"orbits": np.zeros((n, N_ORBITS), np.int64), "orbit_sums": np.zeros((b, N_ORBITS), np.int64),
           "orbit_mean": np.zeros((b, N_ORBITS), np.float64)}
    for g in range(b):
        k, n0 = n_node[g], int(off[g])
        sel = gid == g
        o = node_orbits(dense_adjacency(k, s[sel] - n0, r[sel] - n0))
        out["orbits"][n0:n0 + k] = o
        out["orbit_sums"][g] = o.sum(0)
        if k > 0:
            out["orbit_mean"][g] = o.sum(0).astype(np.float64) / float(k)
    return out


def vec_mmd_sums(sums_a, n_a, sums_b, n_b, sigma=30.0):
    """{sum AA, sum BB, sum AB, cnt_a, cnt_b}: rows sums / n in float64, rows with n <= 0 left out, diagonals in,
    k(x, y) = exp(-|x - y|_2^2 / (2 sigma^2)) - an explicit loop over every ordered pair."""
    sets = []
    for sums, cnt in ((sums_a, n_a), (sums_b, n_b)):
        rows = []
        for x, c in zip(np.asarray(sums, np.int64).reshape(len(cnt), -1), cnt):
            if int(c) > 0:
                rows.append(x.astype(np.float64) / float(int(c)))
        sets.append(rows)

    def block(u, v):
        tot = 0.0
        for x in u:
            for y in v:
                dist = 0.0
                for p, q in zip(x.tolist(), y.tolist()):
                    dist += (p - q) * (p - q)
                tot += float(np.exp(-dist / (2.0 * sigma * sigma)))
        return tot
    return np.array([block(sets[0], sets[0]), block(sets[1], sets[1]), block(sets[0], sets[1]), len(sets[0]), len(sets[1])],
                    np.float64)


def vec_mmd2(sums_a, n_a, sums_b, n_b, sigma=30.0):
    aa, bb, ab, ca, cb = vec_mmd_sums(sums_a, n_a, sums_b, n_b, sigma)
    if ca < 1 or cb < 1:
        raise ValueError("a set without a non-empty graph")
    return aa / (ca * ca) + bb / (cb * cb) - 2.0 * ab / (ca * cb)


# ---- graph builders of the tests (local ids, one direction per edge) -------------------------------------------------------
def petersen():
    s = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    r = [1, 2, 3, 4, 0, 5, 6, 7, 8, 9, 7, 8, 9, 5, 6]
    return np.asarray(s, np.int64), np.asarray(r, np.int64)


def complete_bipartite(p, q):
    i, j = np.meshgrid(np.arange(p), p + np.arange(q), indexing="ij")
    return i.ravel().astype(np.int64), j.ravel().astype(np.int64)


def tailed_triangle():
    """triangle {0, 1, 2} with the tail 3 on node 0"""
    return np.asarray([0, 1, 2, 0], np.int64), np.asarray([1, 2, 0, 3], np.int64)


def chorded_cycle():
    """4-cycle 0-1-2-3 with the chord 0-2"""
    return np.asarray([0, 1, 2, 3, 0], np.int64), np.asarray([1, 2, 3, 0, 2], np.int64)


def big_star():
    """131 nodes: a hub with 130 leaves and six more edges among the leaves (the hub's neighbour queue drains twice)"""
    extra = [(1, 2), (2, 3), (5, 70), (70, 129), (129, 130), (64, 65)]
    s = np.concatenate([np.zeros(130, np.int64), np.asarray([e[0] for e in extra], np.int64)])
    r = np.concatenate([np.arange(1, 131), np.asarray([e[1] for e in extra], np.int64)])
    return s, r
