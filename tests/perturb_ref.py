"""Independent restatement of the edge-deletion noise (include/gnf_perturb.h) for the tests: the hash in pure Python integers,
the filter as a list comprehension, the CSRs from Python's stable sort.  Nothing of the package is imported here beyond what
tests/batches_ref.py uses to build its data set and its batches.

A result is the dict of gnf_perturb_edges' outputs under the header's names (KEYS), as numpy arrays."""
from fractions import Fraction

import numpy as np

import batches_ref as B

KEYS = ("senders", "receivers", "rowptr", "col", "rowptr_t", "col_t", "n_edge", "num_removed", "totals")
M64 = (1 << 64) - 1
KNOWN_ANSWERS = ((0, 0, 0, 4048309744), (0, 0, 1, 3439329295), (12345, 3, 7, 33396603),
                 ((1 << 64) - 1, 65535, 65535, 1033956438), (12345, 0, 2147483646, 2456002885))


def draw(seed, lo, hi):
    x = (seed & M64) ^ ((0x9E3779B97F4A7C15 * (lo + 1)) & M64) ^ ((0xBF58476D1CE4E5B9 * (hi + 1)) & M64)
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def threshold(p):
    """floor(p * 2^32) in exact rational arithmetic (a double is a rational)"""
    return int(Fraction(p) * (1 << 32))


def survives(seed, s, r, thr, self_loops):
    if s == r and self_loops == "keep":
        return True
    return draw(seed, min(s, r), max(s, r)) >= thr


def _csr(rows, cols, n):
    """rows' stable sort: (rowptr [n + 1], col) with each row's entries in their original order"""
    order = sorted(range(len(rows)), key=lambda e: rows[e])
    rowptr = [0] * (n + 1)
    for v in rows:
        rowptr[v + 1] += 1
    for i in range(n):
        rowptr[i + 1] += rowptr[i]
    return rowptr, [cols[e] for e in order]


def perturb(senders, receivers, n_nodes, n_edge, p, seed, self_loops="keep"):
    s, r = [int(v) for v in senders], [int(v) for v in receivers]
    thr = threshold(p)
    keep = [survives(seed, a, b, thr, self_loops) for a, b in zip(s, r)]
    s2 = [a for a, k in zip(s, keep) if k]
    r2 = [b for b, k in zip(r, keep) if k]
    rowptr, col = _csr(r2, s2, n_nodes)
    rowptr_t, col_t = _csr(s2, r2, n_nodes)
    kept, e0 = [], 0
    for ne in n_edge:
        kept.append(sum(keep[e0:e0 + int(ne)]))
        e0 += int(ne)
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)
    return dict(senders=i32(s2), receivers=i32(r2), rowptr=i32(rowptr), col=i32(col), rowptr_t=i32(rowptr_t), col_t=i32(col_t),
                n_edge=i32(kept), num_removed=i32([int(a) - b for a, b in zip(n_edge, kept)]),
                totals=np.array([len(s2), len(s) - len(s2)], np.int64))


def batch(ds, ids):
    """the true batch of the graphs `ids` of batches_ref.dataset(): batches_ref.host_route's arrays (n_node, n_edge,
    node_offsets, senders, receivers and both CSRs)"""
    return B.host_route(ds, ids)


def perturb_batch(ds, ids, p, seed, self_loops="keep"):
    t = batch(ds, ids)
    return perturb(t["senders"], t["receivers"], int(t["node_offsets"][-1]), t["n_edge"], p, seed, self_loops)
