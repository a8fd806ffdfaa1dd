"""numpy float64 / Python-int reference of gnf_amd.graph_stats: per-node degree and triangle counts, clustering bins, the
per-graph histograms, the two histogram distances and the MMD estimator - the definitions of include/gnf.h spelled out with
dense matrices and Python integers.  Reads nothing but its arguments."""
import numpy as np


def dense_adjacency(n, senders, receivers):
    """The undirected simple graph an edge list stands for: A |= A.T, zero diagonal (local ids)."""
    a = np.zeros((n, n), dtype=bool)
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    a[r, s] = True
    a |= a.T
    a[np.arange(n), np.arange(n)] = False
    return a


def clustering_bin(d, t, bins):
    """NORMATIVE: 0 for d < 2, else min(bins - 1, (2 T bins) // (d (d - 1))) in Python integers."""
    d, t, bins = int(d), int(t), int(bins)
    if d < 2:
        return 0
    return min(bins - 1, (2 * t * bins) // (d * (d - 1)))


def node_stats(a):
    """(deg, tri) int64 of a dense boolean adjacency: deg = A.sum(1), tri = diag(A^3) / 2."""
    m = a.astype(np.int64)
    deg = m.sum(1)
    tri = np.einsum("ij,ji->i", m @ m, m) // 2
    return deg, tri


def graph_stats(n_node, senders, receivers, n_edge=None, max_nodes=None, bins=100):
    """Batch-wide edge list (global node ids; graph of an edge = graph of its receiver) -> the dict graph_stats returns."""
    n_node = [int(v) for v in n_node]
    b, n = len(n_node), sum(n_node)
    cap = max(n_node, default=0) if max_nodes is None else int(max_nodes)
    off = np.concatenate([[0], np.cumsum(n_node)]).astype(np.int64)
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    gid = np.searchsorted(off, r, side="right") - 1
    out = {"degree": np.zeros(n, np.int32), "triangles": np.zeros(n, np.int32), "clustering": np.zeros(n, np.float64),
           "degree_hist": np.zeros((b, cap), np.int32), "clustering_hist": np.zeros((b, bins), np.int32),
           "n_edges": np.zeros(b, np.int64), "n_triangles": np.zeros(b, np.int64)}
    for g in range(b):
        k, n0 = n_node[g], int(off[g])
        sel = gid == g
        a = dense_adjacency(k, s[sel] - n0, r[sel] - n0)
        deg, tri = node_stats(a)
        out["degree"][n0:n0 + k], out["triangles"][n0:n0 + k] = deg, tri
        for i in range(k):
            d, t = int(deg[i]), int(tri[i])
            out["degree_hist"][g, d] += 1
            out["clustering_hist"][g, clustering_bin(d, t, bins)] += 1
            out["clustering"][n0 + i] = 2.0 * t / (d * (d - 1)) if d >= 2 else 0.0
        out["n_edges"][g] = int(deg.sum()) // 2
        out["n_triangles"][g] = int(tri.sum()) // 3
    return out


def _pad(h, width):
    h = np.asarray(h, np.float64)
    out = np.zeros((h.shape[0], width))
    out[:, :h.shape[1]] = h
    return out


def emd(x, y, distance_scaling=1.0):
    """1-D earth mover's distance of two pmfs with unit bin spacing: sum_{k <= L-2} |cumsum(x - y)_k| / scaling."""
    c = np.cumsum(np.asarray(x, np.float64) - np.asarray(y, np.float64))
    return float(np.abs(c[:-1]).sum()) / distance_scaling


def tv(x, y):
    return 0.5 * float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).sum())


def mmd_sums(ha, hb, kernel="gaussian_emd", sigma=1.0, distance_scaling=1.0):
    """{sum AA, sum BB, sum AB, cnt_a, cnt_b}: rows normalised in float64, all-zero rows left out, diagonals in."""
    width = max(np.asarray(ha).shape[1], np.asarray(hb).shape[1])
    sets = []
    for h in (ha, hb):
        p = _pad(h, width)
        tot = p.sum(1)
        sets.append(p[tot > 0] / tot[tot > 0, None])

    def k(x, y):
        w = emd(x, y, distance_scaling) if kernel == "gaussian_emd" else tv(x, y)
        return np.exp(-w * w / (2.0 * sigma * sigma))
    block = lambda u, v: float(sum(k(x, y) for x in u for y in v))
    return np.array([block(sets[0], sets[0]), block(sets[1], sets[1]), block(sets[0], sets[1]),
                     len(sets[0]), len(sets[1])], np.float64)


def mmd2(ha, hb, kernel="gaussian_emd", sigma=1.0, distance_scaling=1.0):
    aa, bb, ab, ca, cb = mmd_sums(ha, hb, kernel, sigma, distance_scaling)
    if ca < 1 or cb < 1:
        raise ValueError("a set without a non-empty histogram")
    return aa / (ca * ca) + bb / (cb * cb) - 2.0 * ab / (ca * cb)


def evaluate(stats_a, stats_b):
    return {"degree_mmd": mmd2(stats_a["degree_hist"], stats_b["degree_hist"], "gaussian_emd", 1.0, 1.0),
            "clustering_mmd": mmd2(stats_a["clustering_hist"], stats_b["clustering_hist"], "gaussian_emd", 0.1, 100.0)}


# ---- graph builders of the tests (local ids, one direction per edge: senders < receivers) ----------------------------------
def complete(n):
    i, j = np.triu_indices(n, 1)
    return i, j


def cycle(n):
    i = np.arange(n)
    return i, (i + 1) % n


def star(n):
    return np.zeros(max(n - 1, 0), np.int64), np.arange(1, n)


def gnp(n, p, rng):
    i, j = np.triu_indices(n, 1)
    keep = rng.random(len(i)) < p
    return i[keep], j[keep]


def batch(graphs):
    """[(n, (s, r)), ...] -> n_node, senders, receivers with global ids, each edge once."""
    n_node, s, r, off = [], [], [], 0
    for n, (a, b) in graphs:
        n_node.append(int(n))
        s.append(np.asarray(a, np.int64) + off)
        r.append(np.asarray(b, np.int64) + off)
        off += int(n)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    return n_node, cat(s), cat(r)
