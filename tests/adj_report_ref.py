"""float64 restatement of gnf_amd.adj_loss.reconstruction_report (include/gnf_adj_report.h) in numpy, on the blocks of
tests/adj_loss_ref.py: the classified edge list of embeddings against a true batch, its counts, and the quantile rule the device
and the host share.  Also the batches the GPU tests use and the conditions on them that tests/test_adj_report_cpu.py asserts.

Block convention (adj_loss_ref.graph_blocks): a[s, r] = 1 iff some true edge has sender s and receiver r; u is symmetric.
"""
import numpy as np

import adj_loss_ref as R

# the width at which the count kernel stops keeping its 16-row tile in LDS (16 * D * 4 bytes > 64 KB); it never keeps a column
# tile: columns are read from global memory at every width
D_ROWS_LEAVE_LDS = 1025
WIDTHS = (1, 7, 64, D_ROWS_LEAVE_LDS)
# (D, distance, symmetric true graph, graph seed): every width directed with duplicates, one symmetric batch, the two other
# fixed tokens.  Graph seed 1 at the widest: with seed 0 the largest graph has 247 false negatives, and the conditions below
# ask for more than 256 (a condition on the inputs, checked by tests/test_adj_report_cpu.py).
BATCHES = [(1, R.SCALED_HACKY, False, 0), (7, R.SCALED_HACKY, False, 0), (64, R.SCALED_HACKY, False, 0),
           (D_ROWS_LEAVE_LDS, R.SCALED_HACKY, False, 1), (7, R.SCALED_HACKY, True, 0), (7, R.HACKY, False, 0),
           (7, R.sigmoid_l2(3.0, 2.0), False, 0)]
QUANTILES = (0.0, 0.25, 0.5, 0.75, 1.0)
_CACHE = {}


def batch(d, dist=R.SCALED_HACKY, symmetric=False, graph_seed=0):
    """(seed, z, (n_edge, senders, receivers)) of adj_loss_ref.pick_seed with duplicate rows, so that equal scores occur;
    computed once per process"""
    key = (d, dist, symmetric, graph_seed)
    if key not in _CACHE:
        _CACHE[key] = R.pick_seed(R.SIZES, d, dist, duplicate_rows=True, graph_seed=graph_seed, symmetric=symmetric)
    return _CACHE[key]


def report(z, sizes, senders, receivers, dist=R.SCALED_HACKY, threshold=0.5):
    """the edge list in the device's order (receivers ascending, senders ascending within a receiver): dict of senders,
    receivers, cls (int32), score (float64), rowptr [N + 1], n_edge [B], class_pairs int64 [B, 3], totals int64 [4]"""
    n = int(np.sum(sizes))
    ss, rr, cc, pp, n_edge, pairs = [], [], [], [], [], []
    rowcnt = np.zeros(n, np.int64)
    for b in R.graph_blocks(z, sizes, senders, receivers, dist):
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-b["u"]))
        pred = (p > threshold) & b["off"]
        a = b["a"] & b["off"]
        r_loc, s_loc = np.nonzero((a | pred).T)            # rows of the transpose are receivers
        cls = np.where(a & pred, 1, np.where(pred, 2, 3))[s_loc, r_loc]
        ss.append(s_loc + b["n0"]), rr.append(r_loc + b["n0"]), cc.append(cls), pp.append(p[s_loc, r_loc])
        n_edge.append(len(s_loc))
        pairs.append([int((cls == c).sum()) for c in (1, 2, 3)])
        rowcnt[b["n0"]:b["n0"] + b["ng"]] = np.bincount(r_loc, minlength=b["ng"])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    pairs = np.asarray(pairs, np.int64).reshape(len(sizes), 3)
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(rowcnt, out=rowptr[1:])
    return dict(senders=cat(ss, np.int32), receivers=cat(rr, np.int32), cls=cat(cc, np.int32), score=cat(pp, np.float64),
                rowptr=rowptr, n_edge=np.asarray(n_edge, np.int32), class_pairs=pairs,
                totals=np.asarray([int(np.sum(n_edge))] + pairs.sum(0).tolist(), np.int64))


def true_edges(sizes, senders, receivers):
    """the true batch's deduplicated, loop-free, in-graph edges in the device's order: (senders, receivers)"""
    s, r = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    keep = (s != r) & (gid[s] == gid[r])
    pairs = np.unique(np.stack([r[keep], s[keep]], 1), axis=0)   # sorted by receiver, then sender
    return pairs[:, 1].astype(np.int32), pairs[:, 0].astype(np.int32)


# ---- the quantile rule -------------------------------------------------------------------------------------------------------
def order_stats(x, quantiles):
    """x: float32 scores of one class in one segment.  (stat float32 [nq, 2] = {x[lo], x[hi]}, n) with the order of the bit
    patterns read as uint32, h = (n - 1) q one float64 product, lo = floor(h), hi = min(lo + 1, n - 1); NaN for n = 0"""
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    stat = np.full((len(quantiles), 2), np.nan, np.float32)
    if n:
        srt = np.sort(x.view(np.uint32)).view(np.float32)
        for k, q in enumerate(quantiles):
            h = np.float64(n - 1) * np.float64(q)
            lo = int(np.floor(h))
            stat[k] = srt[lo], srt[min(lo + 1, n - 1)]
    return stat, n


def interpolate(stat, n, quantiles):
    """the host side: x[lo] + (h - lo) (x[hi] - x[lo]) in float64, two operations after the difference"""
    h = np.float64(max(n - 1, 0)) * np.asarray(quantiles, np.float64)
    x = stat.astype(np.float64)
    return x[:, 0] + (h - np.floor(h)) * (x[:, 1] - x[:, 0])


def segment_stats(score, cls, rowptr, seg_nodes, quantiles):
    """(stat float32 [S, 2, nq, 2], count int64 [S, 2]) over the segments of node offsets seg_nodes, classes 2 and 3"""
    n_seg = len(seg_nodes) - 1
    stat = np.full((n_seg, 2, len(quantiles), 2), np.nan, np.float32)
    count = np.zeros((n_seg, 2), np.int64)
    for s in range(n_seg):
        e0, e1 = int(rowptr[seg_nodes[s]]), int(rowptr[seg_nodes[s + 1]])
        for c in (0, 1):
            stat[s, c], count[s, c] = order_stats(score[e0:e1][cls[e0:e1] == c + 2], quantiles)
    return stat, count
