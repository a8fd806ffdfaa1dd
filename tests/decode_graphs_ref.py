"""numpy reference of flow.decode_graphs: the edge lists, rowptr and n_edge that follow from a list of per-graph
probability blocks, a threshold and a self-loop flag - and a generator of clustered embeddings whose edge set is known in
closed form (disjoint cliques), with a margin that makes float32 / float64 rounding irrelevant."""
import numpy as np


def edges_from_blocks(blocks, threshold, self_loops):
    """Edge (sender = j, receiver = i) of graph g iff blocks[g][i, j] > threshold (strictly, in the blocks' own dtype);
    the diagonal is an edge iff self_loops.  Receivers ascend, senders ascend within a receiver (numpy.nonzero's row-major
    order).  Returns dict(senders, receivers int32 batch-wide ids; rowptr int32 [N + 1]; n_edge int32 [B]; total)."""
    s, r, n_edge, counts, off = [], [], [], [], 0
    for b in blocks:
        b = np.asarray(b)
        n = b.shape[0]
        m = b.reshape(n, n) > b.dtype.type(threshold)
        if n:
            m[np.arange(n), np.arange(n)] = bool(self_loops)
        i, j = np.nonzero(m)
        r.append(i + off)
        s.append(j + off)
        n_edge.append(len(i))
        counts.append(m.sum(axis=1))
        off += n
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    rowptr = np.zeros(off + 1, np.int64)
    np.cumsum(cat(counts), out=rowptr[1:])
    return {"senders": cat(s).astype(np.int32), "receivers": cat(r).astype(np.int32), "rowptr": rowptr.astype(np.int32),
            "n_edge": np.asarray(n_edge, np.int32), "total": int(rowptr[-1])}


def clique_blocks(n_node, labels):
    """The closed form for clustered inputs as 0 / 1 float64 blocks: P = 1 inside a cluster, 0 across."""
    out, off = [], 0
    for n in n_node:
        lab = labels[off:off + int(n)]
        out.append((lab[:, None] == lab[None, :]).astype(np.float64))
        off += int(n)
    return out


# margins of clustered_embeddings, in units of d2 / sqrt(D): a pair inside a cluster stays below INSIDE_MAX, a pair across
# clusters above ACROSS_MIN, hence P >= sigmoid(10 (1 - 0.25)) > 0.999 inside and P <= sigmoid(10 (1 - 4)) < 1e-12 across
INSIDE_MAX, ACROSS_MIN = 0.25, 4.0


def clustered_embeddings(rng, n_node, d):
    """Every graph's nodes in 2 - 4 clusters.  Centres on the first axis, 4.5 D^(1/4) apart (>= 2 D^(1/4) sqrt(4) + twice
    the cluster radius); each node within 0.24 D^(1/4) of its centre, so two nodes of a cluster are at most 0.48 D^(1/4)
    apart (d2 / sqrt(D) <= 0.2304) and two nodes of different clusters at least 4.02 D^(1/4) (d2 / sqrt(D) >= 16.1).
    Returns (z float32 [N, d], labels int [N])."""
    q = float(d) ** 0.25
    zs, labs = [], []
    for n in n_node:
        n = int(n)
        k = int(rng.integers(2, 5))
        lab = rng.integers(0, k, size=n)
        u = rng.standard_normal((n, d))
        u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-30)
        z = u * (0.24 * q * rng.uniform(0.0, 1.0, size=(n, 1)))
        z[:, 0] += 4.5 * q * lab
        zs.append(z)
        labs.append(lab)
    z = np.concatenate(zs) if zs else np.zeros((0, d))
    return z.astype(np.float32), (np.concatenate(labs) if labs else np.zeros(0, np.int64))
