"""Pure-Python restatement of include/gnf_random_graphs.h on top of synthetic_ref.draw: unbounded ints, one pair and one draw
at a time, a sequential Barabasi-Albert that keeps the list of accepted candidates - independent of the numpy twin
(gnf_amd.random_graphs.random_graphs_host), which works on whole matrices and finds first occurrences with np.unique."""
from synthetic_ref import draw

BA_DRAWS = 256
BA_SEED_XOR = 0xA5A5A5A5A5A5A5A5
M64 = (1 << 64) - 1


def threshold(p):
    """(uint64)(p * 2^32): p is a float; the product by a power of two is exact"""
    return int(p * 4294967296.0)


def planted_edges(n, graph, thr_in, thr_out, block, seed):
    """the undirected edge set {(lo, hi)} of one graph; block: a list of n labels"""
    edges = set()
    for lo in range(n):
        for hi in range(lo + 1, n):
            if draw(seed, graph, lo, hi) < (thr_in if block[lo] == block[hi] else thr_out):
                edges.add((lo, hi))
    return edges


def ba_targets(n, m, graph, seed):
    """({t: targets(t)}, number of nodes that took the fallback, most draws any node looked at) for n > m"""
    targets = {m: list(range(m))}
    fallbacks, most = 0, 0
    for t in range(m + 1, n):
        size = 2 * m * (t - m)
        accepted = []
        for j in range(BA_DRAWS):
            if len(accepted) == m:
                break
            k = (draw((seed ^ BA_SEED_XOR) & M64, graph, t, j) * size) >> 32
            tp, c = m + k // (2 * m), k % (2 * m)
            cand = targets[tp][c] if c < m else tp
            if cand not in accepted:
                accepted.append(cand)
            most = max(most, j + 1)
        if len(accepted) < m:
            fallbacks += 1
            for v in range(t):
                if len(accepted) == m:
                    break
                if v not in accepted:
                    accepted.append(v)
        targets[t] = accepted
    return targets, fallbacks, most


def ba_edges(n, m, graph, seed):
    """(edge set, fallback nodes)"""
    if n <= m:
        return set(), 0
    targets, fallbacks, _ = ba_targets(n, m, graph, seed)
    return {(u, t) for t, us in targets.items() for u in us}, fallbacks


def default_block(n, n_blocks):
    return [(i * n_blocks) // n for i in range(n)]


def batch(model, n_node, params, params_out=None, n_blocks=1, blocks=None, seed=0, first_graph=0, self_loops=False, max_m=64):
    """The arrays in the decoder's order for a batch: dict of plain lists "senders", "receivers", "rowptr", "n_edge", plus
    "total", "edge_sets" (per graph, local ids, lo < hi) and "fallbacks" (per graph).  model: "planted" (params / params_out:
    thresholds per graph; params_out None = params) or "ba" (params: m per graph, clamped into [1, max_m])."""
    senders, receivers, rowptr, n_edge, sets, fallbacks = [], [], [0], [], [], []
    o = 0
    for b, n in enumerate(n_node):
        g = first_graph + b
        if model == "ba":
            edges, fb = ba_edges(n, min(max(params[b], 1), max_m), g, seed)
        else:
            block = default_block(n, n_blocks) if blocks is None else list(blocks[o:o + n])
            edges, fb = planted_edges(n, g, params[b], params[b] if params_out is None else params_out[b], block, seed), 0
        nbrs = [[] for _ in range(n)]
        for lo, hi in edges:
            nbrs[lo].append(hi)
            nbrs[hi].append(lo)
        count = 0
        for i in range(n):
            row = sorted(nbrs[i] + ([i] if self_loops else []))
            senders += [o + j for j in row]
            receivers += [o + i] * len(row)
            rowptr.append(rowptr[-1] + len(row))
            count += len(row)
        n_edge.append(count)
        sets.append(edges)
        fallbacks.append(fb)
        o += n
    return {"senders": senders, "receivers": receivers, "rowptr": rowptr, "n_edge": n_edge, "total": rowptr[-1],
            "edge_sets": sets, "fallbacks": fallbacks}
