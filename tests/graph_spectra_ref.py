"""numpy float64 reference of gnf_amd.graph_stats.graph_spectra: the normalised Laplacian of include/gnf_graph_spectra.h spelled
out with dense matrices, its eigenvalues by numpy.linalg.eigvalsh (LAPACK), the clamped histogram, and the cases the GPU tests
run.  Reads nothing but its arguments."""
import numpy as np

import graph_stats_ref as S

BINS, LO, HI = 200, -1e-5, 2.0     # the Python layer's defaults
EIG_ATOL = 1e-11                   # device eigenvalues against this reference (derived in tests/test_graph_spectra_gpu.py)
MARGIN = 1e-9                      # every case keeps its eigenvalues this far from a bin edge: EIG_ATOL cannot move a count


def laplacian(a):
    """NORMATIVE: L_ii = 1 if d_i > 0 else 0, L_ij = -1 / sqrt(d_i d_j) for an edge, else 0 (a boolean simple adjacency)."""
    a = np.asarray(a, bool)
    d = a.sum(1).astype(np.float64)
    prod = np.sqrt(np.outer(d, d))
    lap = np.where(a, -1.0 / np.where(prod > 0, prod, 1.0), 0.0)
    lap[np.diag_indices(len(d))] = (d > 0).astype(np.float64)
    return lap


def eigenvalues(n, senders, receivers):
    """ascending eigenvalues of the graph an edge list (local ids) stands for"""
    if n == 0:
        return np.zeros(0, np.float64)
    return np.linalg.eigvalsh(laplacian(S.dense_adjacency(n, senders, receivers)))


def bin_of(x, lo=LO, hi=HI, bins=BINS):
    """NORMATIVE: clamp(floor((x - lo) * bins / (hi - lo)), 0, bins - 1) - values outside [lo, hi) are kept, not dropped"""
    t = np.floor((np.asarray(x, np.float64) - lo) * bins / (hi - lo))
    return np.clip(t, 0, bins - 1).astype(np.int64)


def histogram(eigs, lo=LO, hi=HI, bins=BINS):
    return np.bincount(bin_of(eigs, lo, hi, bins), minlength=bins).astype(np.int32)


def edge_margin(eigs, lo=LO, hi=HI, bins=BINS):
    """smallest distance of any eigenvalue to an interior bin edge lo + k (hi - lo) / bins, k = 1 .. bins - 1 (inf without one)"""
    eigs = np.asarray(eigs, np.float64)
    if bins < 2 or len(eigs) == 0:
        return np.inf
    edges = lo + np.arange(1, bins) * (hi - lo) / bins
    return float(np.abs(eigs[:, None] - edges[None, :]).min())


def graph_spectra(n_node, senders, receivers, lo=LO, hi=HI, bins=BINS):
    """Batch-wide edge list (global node ids; graph of an edge = graph of its receiver) -> the dict graph_spectra returns."""
    n_node = [int(v) for v in n_node]
    off = np.concatenate([[0], np.cumsum(n_node)]).astype(np.int64)
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    gid = np.searchsorted(off, r, side="right") - 1
    out = {"eigenvalues": np.zeros(int(off[-1]), np.float64), "spectral_hist": np.zeros((len(n_node), max(bins, 0)), np.int32),
           "n_node": np.asarray(n_node, np.int32)}
    for g, k in enumerate(n_node):
        n0 = int(off[g])
        sel = gid == g
        e = eigenvalues(k, s[sel] - n0, r[sel] - n0)
        out["eigenvalues"][n0:n0 + k] = e
        if bins > 0:
            out["spectral_hist"][g] = histogram(e, lo, hi, bins)
    return out


# ---- graph builders (local ids, one direction per edge) --------------------------------------------------------------------
def ring_with_chords(n):
    """the cycle on n nodes plus the chords i - (i + 2 + i % 3) for every third node: connected, irregular, not bipartite"""
    if n < 3:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64)) if n < 2 else (np.array([0]), np.array([1]))
    s, r = S.cycle(n)
    i = np.arange(0, n, 3)
    j = (i + 2 + i % 3) % n
    keep = (i != j) & ((i + 1) % n != j) & ((j + 1) % n != i)
    return np.concatenate([s, i[keep]]), np.concatenate([r, j[keep]])


def grid(rows, cols):
    idx = np.arange(rows * cols).reshape(rows, cols)
    s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    r = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return s, r


def two_components_and_isolated():
    """a triangle on 0 1 2, a path 3 - 4 - 5 - 6, and the isolated nodes 7 8 9"""
    return np.array([0, 1, 2, 3, 4, 5]), np.array([1, 2, 0, 4, 5, 6])


def mixed_cases():
    """[(name, n, (s, r))]: the batch of the first GPU test, in its order"""
    rng = np.random.default_rng(40008)
    cases = [("empty", 0, S.complete(0)), ("single", 1, S.complete(1)), ("edge", 2, S.complete(2)), ("triangle", 3, S.complete(3)),
             ("K4", 4, S.complete(4)), ("star9", 9, S.star(9))]
    cases += [(f"ring{n}", n, ring_with_chords(n)) for n in (5, 17, 64, 65)]
    cases += [("grid6x6", 36, grid(6, 6)), ("components", 10, two_components_and_isolated()), ("gnp40", 40, S.gnp(40, 0.08, rng))]
    return cases


def other_cases():
    """a second, different set of graphs (spectral_mmd and evaluate_generated compare it with the mixed batch)"""
    rng = np.random.default_rng(9)
    return [("gnp12", 12, S.gnp(12, 0.5, rng)), ("empty", 0, S.complete(0)), ("cycle9", 9, S.cycle(9)),
            ("gnp15", 15, S.gnp(15, 0.3, rng)), ("K6", 6, S.complete(6)), ("grid3x5", 15, grid(3, 5))]


def route_cases(n_lds):
    """the three graphs of the route test: n_lds and n_lds + 1 nodes (either side of the LDS limit), G(n_lds + 60, 0.05)"""
    rng = np.random.default_rng(139)
    return [(f"ring{n_lds}", n_lds, ring_with_chords(n_lds)), (f"ring{n_lds + 1}", n_lds + 1, ring_with_chords(n_lds + 1)),
            (f"gnp{n_lds + 60}", n_lds + 60, S.gnp(n_lds + 60, 0.05, rng))]


def batch(cases):
    return S.batch([(n, e) for _, n, e in cases])
