"""numpy uint64 reference of gnf_amd.graph_stats.graph_hashes / uniqueness_novelty: the Weisfeiler-Lehman hash that
include/gnf_graph_hashes.h defines, restated with per-edge accumulation over the deduplicated edge set of the batch, the match
rules of gnf_graph_hash_match, and the cases the tests run.  Array arithmetic on numpy.uint64 wraps silently, which is the
arithmetic the definition asks for.  Reads nothing but its arguments (and, for dataset(), the project's data files)."""
import os

import numpy as np

import graph_components_ref as C
import graph_stats_ref as S

U = np.uint64
KA, KB, KC, KD = U(0xA5A5A5A5A5A5A5A5), U(0xD6E8FEB86659FD93), U(0xFF51AFD7ED558CCD), U(0xC4CEB9FE1A85EC53)
SIZE = U(0x100000001B3)
KEYS = ("hash", "node_colour", "n_edges", "n_node")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
DATASETS = ("caveman_small", "citeseer_small", "community_medium", "grid", "grid_small")


def mix(x):
    x = np.atleast_1d(np.asarray(x, U)) + U(0x9E3779B97F4A7C15)      # (arrays wrap silently; numpy scalars would warn)
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def _scatter(index, values, size):
    out = np.zeros(size, U)
    np.add.at(out, index, values)
    return out


def hashes(n_node, senders, receivers, iterations=3, labels=None):
    """Batch-wide edge list (global node ids) -> the dict graph_hashes returns, as numpy arrays (hash and node_colour as the
    int64 view of their bits)."""
    off, pairs = C._simple_pairs(n_node, senders, receivers)
    sizes = np.array([int(v) for v in n_node], np.int64).reshape(len(n_node))
    n, b = int(off[-1]), len(sizes)
    gid = np.repeat(np.arange(b), sizes)
    src = np.concatenate([pairs[:, 0], pairs[:, 1]])
    dst = np.concatenate([pairs[:, 1], pairs[:, 0]])
    degree = np.bincount(dst, minlength=n)[:n]
    e = np.bincount(gid[pairs[:, 0]], minlength=b)[:b] if n else np.zeros(b, np.int64)
    v = degree.astype(U) if labels is None else np.asarray(labels, np.int64).reshape(n).view(U)
    c = mix(v)
    h = mix(sizes.astype(U) * SIZE + e.astype(U))
    h = mix(h + _scatter(gid, mix(c ^ KA), b))
    for t in range(1, int(iterations) + 1):
        c = mix(c * KC + _scatter(dst, mix(c[src] ^ KB), n) + U(t))
        h = mix(h * KD + _scatter(gid, mix(c ^ KA), b))
    return {"hash": h.view(np.int64), "node_colour": c.view(np.int64), "n_edges": e.astype(np.int64),
            "n_node": sizes.astype(np.int32)}


def match(hash_a, n_node_a, hash_b, n_node_b):
    """gnf_graph_hash_match: first_in_a, match_in_b (int32 [a]) and counts (int64 [4])"""
    a = len(hash_a)
    first, found = np.full(a, -1, np.int32), np.full(a, -1, np.int32)
    seen_a, seen_b = {}, {}
    for j in range(len(hash_b)):
        seen_b.setdefault((int(hash_b[j]), int(n_node_b[j])), j)
    counts = np.zeros(4, np.int64)
    for g in range(a):
        if int(n_node_a[g]) == 0:
            continue
        key = (int(hash_a[g]), int(n_node_a[g]))
        first[g] = seen_a.setdefault(key, g)
        found[g] = seen_b.get(key, -1)
        counts += [1, first[g] == g, found[g] < 0, first[g] == g and found[g] < 0]
    return {"first_in_generated": first, "match_in_training": found, "counts": counts}


def shares(m):
    valid = float(m["counts"][0])
    return {"uniqueness": m["counts"][1] / valid, "novelty": m["counts"][2] / valid, "unique_novel": m["counts"][3] / valid}


# ---- cases -----------------------------------------------------------------------------------------------------------------
def permuted(n, edges, perm):
    """the graph renumbered: node i becomes perm[i]"""
    perm = np.asarray(perm, np.int64)
    return perm[np.asarray(edges[0], np.int64)], perm[np.asarray(edges[1], np.int64)]


def small_cases():
    """[(name, n, (s, r))] - local ids, one direction per edge; each names the kernel mistake it is there for"""
    rng = np.random.default_rng(4096)
    return [("K3", 3, S.complete(3)),
            ("empty", 0, C.no_edges(0)),                            # the graph's offset inside a batch
            ("single_node", 1, C.no_edges(1)),
            ("edge_63_64", 65, C.single_edge(65, 63, 64)),          # neighbours beyond the first bitmap word
            ("path130", 130, C.path(130)), ("path130_reversed", 130, C.path_reversed(130)),
            ("path130_folded", 130, C.path_folded(130)),            # three numberings: one hash
            ("star70_hub_last", 70, C.star_hub_last(70)),           # the last partial word
            ("K64", 64, S.complete(64)), ("K65", 65, S.complete(65)),
            ("sparse40", 40, C.sparse(40, rng, 2.5)), ("sparse129", 129, C.sparse(129, rng, 2.5))]   # irregular: the round salt


def spell(cases, how, rng=None):
    """(n_node, n_edge, senders, receivers) with global ids of one spelling of the cases: "one_direction", "symmetric", or
    "duplicates_and_loops" (both directions, one of them twice, every self loop twice, shuffled within the graph)"""
    n_node, n_edge, ss, rr, off = [], [], [], [], 0
    for _, n, (s, r) in cases:
        s, r = np.asarray(s, np.int64), np.asarray(r, np.int64)
        if how == "symmetric":
            s, r = np.concatenate([s, r]), np.concatenate([r, s])
        elif how == "duplicates_and_loops":
            loops = np.arange(n)
            s, r = np.concatenate([s, r, s, loops, loops]), np.concatenate([r, s, r, loops, loops])
            p = rng.permutation(len(s))
            s, r = s[p], r[p]
        else:
            assert how == "one_direction"
        n_node.append(n), n_edge.append(len(s)), ss.append(s + off), rr.append(r + off)
        off += n
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    return n_node, n_edge, cat(ss), cat(rr)


def cube():
    """Q3: 3-regular on 8 nodes, bipartite"""
    i = np.arange(8)
    s = np.concatenate([i, i, i])
    r = np.concatenate([i ^ 1, i ^ 2, i ^ 4])
    return s[s < r], r[s < r]


def wagner():
    """the 8-cycle with its four diameters: 3-regular on 8 nodes, with 5-cycles - not isomorphic to the cube"""
    i = np.arange(8)
    return np.concatenate([i, i[:4]]), np.concatenate([(i + 1) % 8, i[:4] + 4])


def two_triangles():
    return np.array([0, 1, 2, 3, 4, 5]), np.array([1, 2, 0, 4, 5, 3])


def triangles_per_node(n, edges):
    return S.node_stats(S.dense_adjacency(n, *edges))[1]


def dataset(name, index=None):
    """(n_node, n_edge, senders, receivers) of data/<name>.npz with global node ids; index selects graphs"""
    d = np.load(os.path.join(DATA, name + ".npz"))
    n_node, n_edge = d["n_node"].astype(np.int64), d["n_edge"].astype(np.int64)
    e_off = np.concatenate([[0], np.cumsum(n_edge)])
    index = range(len(n_node)) if index is None else index
    nn, ne, ss, rr, off = [], [], [], [], 0
    for g in index:
        sl = slice(int(e_off[g]), int(e_off[g + 1]))
        nn.append(int(n_node[g])), ne.append(int(n_edge[g]))
        ss.append(d["senders"][sl].astype(np.int64) + off), rr.append(d["receivers"][sl].astype(np.int64) + off)
        off += int(n_node[g])
    return nn, ne, np.concatenate(ss), np.concatenate(rr)
