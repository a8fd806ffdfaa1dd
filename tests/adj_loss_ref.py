"""float64 restatement of what gnf_amd.adj_loss.binary_loss computes (include/gnf_adj_loss.h): loss.py's binary_loss, its
edge-error counts and the gradient of the summed loss, graph by graph in numpy.

Two forms of the loss: `binary_loss` works in logit space (ce = softplus(u_c) - t u_c, u_c the clipped logit), which is what
the device evaluates; `binary_loss_literal` follows loss.py:162-188 to the letter on dense [N, N] matrices - mask,
remove_diag, tf.keras.backend.binary_crossentropy as TF 1.x writes it (clip the probability to [1e-7, 1 - 1e-7], logit,
sigmoid cross-entropy with logits).  tests/test_adj_loss_cpu.py holds the two against each other.

Also here: the test batches (sizes, embeddings, true graphs) and the margin condition on them - a condition on the INPUTS,
computed from this restatement alone: every pair's float64 logit stays 2 delta_ij away from the kinks u = +-U (the clip)
and u = 0 (the counts' threshold at abs_tol = 0.5), delta_ij bounding what fp32 arithmetic can move the logit by, so counts
and clip decisions are well defined for an fp32 implementation.  No pair is ever left out of a comparison.
"""
import numpy as np

KERAS_EPSILON = 1e-7
U = float(np.log((1.0 - KERAS_EPSILON) / KERAS_EPSILON))
SIZES = [1, 0, 17, 16, 33, 65, 2, 64]   # tile edge 16 / 17 / 33, bitmap word edge 64 / 65, an empty and a 1-node graph

SCALED_HACKY = (10.0, 1.0, True)    # loss.py:45-53
HACKY = (10.0, 1.0, False)          # loss.py:36-42


def sigmoid_l2(temp, shift):        # loss.py:56-62
    return (float(temp), float(shift), True)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def embeddings(sizes, d, seed, duplicate_rows=False):
    """fp32 [N, d]: N(0, 1) * 0.5 * d^-1/4, one row in eight (at random) stretched by 4; duplicate_rows: in every graph of 4
    or more nodes row 1 repeats row 0 and row 3 row 2 (d2 = 0 pairs)"""
    n = int(np.sum(sizes))
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, d)) * 0.5 * d ** -0.25
    z[rng.random(n) < 0.125] *= 4.0
    if duplicate_rows:
        o = 0
        for ng in sizes:
            if ng >= 4:
                z[o + 1], z[o + 3] = z[o], z[o + 2]
            o += ng
    return z.astype(np.float32)


def true_graph(sizes, seed, p=0.3, symmetric=False, duplicates=3):
    """(n_edge [B], senders, receivers): directed G(n, p) per graph (both directions of an undirected one if symmetric), one
    self loop per node and, per graph with edges, `duplicates` repeated edges; edges grouped by graph, shuffled inside."""
    rng = np.random.default_rng(seed + 1000)
    n_edge, ss, rr, o = [], [], [], 0
    for ng in sizes:
        m = rng.random((ng, ng)) < p
        np.fill_diagonal(m, False)
        if symmetric:
            m = np.triu(m) | np.triu(m).T
        s, r = np.nonzero(m)
        if len(s) and duplicates:
            pick = rng.integers(0, len(s), size=duplicates)
            s, r = np.concatenate([s, s[pick]]), np.concatenate([r, r[pick]])
        loops = np.arange(ng)
        s, r = np.concatenate([s, loops]), np.concatenate([r, loops])
        perm = rng.permutation(len(s))
        ss.append(s[perm] + o), rr.append(r[perm] + o), n_edge.append(len(s))
        o += ng
    return (np.asarray(n_edge, np.int32), np.concatenate(ss).astype(np.int32) if ss else np.zeros(0, np.int32),
            np.concatenate(rr).astype(np.int32) if rr else np.zeros(0, np.int32))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _scale(dist, d):
    return 1.0 / np.sqrt(np.float64(d)) if dist[2] else 1.0


def graph_blocks(z, sizes, senders, receivers, dist=SCALED_HACKY):
    """per graph: dict(n0, ng, d2, u, a, off) - [ng, ng] float64 d2 / u, hard labels a[i, j] = 1 iff some edge has sender i and
    receiver j (duplicates once; edges into another graph and self loops dropped), off = the off-diagonal mask"""
    z = np.asarray(z, np.float64)
    temp, shift, _ = dist
    scale = _scale(dist, z.shape[1])
    senders, receivers = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    out, o = [], 0
    for ng in sizes:
        zg = z[o:o + ng]
        diff = zg[:, None, :] - zg[None, :, :]
        d2 = (diff * diff).sum(-1)
        u = temp * (shift - d2 * scale)
        a = np.zeros((ng, ng), bool)
        keep = (senders >= o) & (senders < o + ng) & (receivers >= o) & (receivers < o + ng) & (senders != receivers)
        a[senders[keep] - o, receivers[keep] - o] = True
        out.append(dict(n0=o, ng=ng, d2=d2, u=u, a=a, off=~np.eye(ng, dtype=bool)))
        o += ng
    return out


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def binary_loss(z, sizes, senders, receivers, dist=SCALED_HACKY, soft=False, epsilon=0.1, abs_tol=0.5):
    """logit space.  Returns loss_per_graph [B], sum_loss, mean_loss, fp / fn (ordered pairs, int64 [B]), grad (d sum_loss /
    d z, float64 [N, D]; grad / (N^2 - N) differentiates mean_loss), and per graph the [ng, ng] blocks "ce", "c", "clipped"."""
    z64 = np.asarray(z, np.float64)
    n, d = z64.shape
    temp = dist[0]
    scale = _scale(dist, d)
    blocks = graph_blocks(z, sizes, senders, receivers, dist)
    loss, fp, fn, grad = [], [], [], np.zeros((n, d))
    for b in blocks:
        u, a, off = b["u"], b["a"], b["off"]
        t = np.where(a, 1.0 - epsilon, epsilon) if soft else a.astype(np.float64)
        uc = np.clip(u, -U, U)
        ce = np.where(off, softplus(uc) - t * uc, 0.0)
        with np.errstate(over="ignore"):   # (a far pair: exp(-u) = inf, p = 0)
            p = 1.0 / (1.0 + np.exp(-u))
        hard = a.astype(np.float64)
        fp.append(int(((p - hard > abs_tol) & off).sum()))
        fn.append(int(((hard - p > abs_tol) & off).sum()))
        clipped = ~(np.abs(u) < U)
        c = np.where(off & ~clipped, -2.0 * temp * scale * ((p - t) + (p - t.T)), 0.0)
        zg = z64[b["n0"]:b["n0"] + b["ng"]]
        # grad_i = sum_j c_ij (z_i - z_j)
        grad[b["n0"]:b["n0"] + b["ng"]] = c.sum(1)[:, None] * zg - c @ zg
        loss.append(float(ce.sum()))
        b.update(ce=ce, c=c, clipped=clipped & off, p=p)
    total = float(np.sum(loss))
    return dict(loss_per_graph=np.asarray(loss), sum_loss=total, mean_loss=total / (n * n - n) if n >= 2 else 0.0,
                fp=np.asarray(fp, np.int64), fn=np.asarray(fn, np.int64), grad=grad, blocks=blocks)


def binary_loss_literal(z, sizes, senders, receivers, dist=SCALED_HACKY, soft=False, epsilon=0.1):
    """loss.py:162-188 on dense [N, N] matrices (true_adj read as 0 / 1: duplicates once).  Returns (sum_loss, mean_loss,
    masked_ce_loss [N, N])."""
    z64 = np.asarray(z, np.float64)
    n, d = z64.shape
    temp, shift, _ = dist
    lm = np.zeros((n, n))
    o = 0
    for ng in sizes:
        lm[o:o + ng, o:o + ng] = 1.0
        o += ng
    true_adj = np.zeros((n, n))
    true_adj[np.asarray(senders, np.int64), np.asarray(receivers, np.int64)] = 1.0
    if soft:
        true_adj = np.where(true_adj > 0.5, 1.0 - epsilon, 0.0 + epsilon)
    r = (z64 * z64).sum(1)[:, None]
    dist2 = r - 2.0 * z64 @ z64.T + r.T
    with np.errstate(over="ignore"):
        pred = 1.0 / (1.0 + np.exp(-(temp * (shift - dist2 * _scale(dist, d)))))
    pred = pred * lm
    # tf.keras.backend.binary_crossentropy (TF 1.x): clip, logit, sigmoid_cross_entropy_with_logits
    out = np.clip(pred, KERAS_EPSILON, 1.0 - KERAS_EPSILON)
    x = np.log(out / (1.0 - out))
    ce = np.maximum(x, 0.0) - x * true_adj + np.log1p(np.exp(-np.abs(x)))
    masked = (lm * (1.0 - np.eye(n))) * ce
    total = float(masked.sum())
    return total, (total / (n * n - n) if n >= 2 else 0.0), masked


# ---- the margin condition and the derived bounds ---------------------------------------------------------------------------
def delta(blocks, d, dist=SCALED_HACKY):
    """per graph [ng, ng]: what fp32 arithmetic can move u_ij by: the rounding bound of the fmaf chain over d features,
    (d + 3) 2^-24 relative on d2, carried through temp * scale, plus 2^-16 for the last three operations at |u| <= U
    (= 10 (d + 3) 2^-24 d2 / sqrt(d) + 2^-16 for scaled_hacky_sigmoid_l2)"""
    temp = abs(dist[0])
    scale = _scale(dist, d)
    return [temp * (d + 3) * 2.0 ** -24 * b["d2"] * scale + 2.0 ** -16 for b in blocks]


def margin_ok(blocks, d, dist=SCALED_HACKY):
    """every off-diagonal pair keeps 2 delta_ij from u = -U, u = 0 and u = +U"""
    for b, dl in zip(blocks, delta(blocks, d, dist)):
        u, off = b["u"], b["off"]
        gap = np.minimum(np.minimum(np.abs(u - U), np.abs(u + U)), np.abs(u))
        if (off & (gap < 2.0 * dl)).any():
            return False
    return True


def pick_seed(sizes, d, dist=SCALED_HACKY, duplicate_rows=False, graph_seed=0, symmetric=False):
    """the first seed in range(16) whose embeddings satisfy margin_ok (None: there is none), with that batch"""
    n_edge, s, r = true_graph(sizes, graph_seed, symmetric=symmetric)
    for seed in range(16):
        z = embeddings(sizes, d, seed, duplicate_rows)
        if margin_ok(graph_blocks(z, sizes, s, r, dist), d, dist):
            return seed, z, (n_edge, s, r)
    return None, None, (n_edge, s, r)


def loss_bounds(ref, d, dist=SCALED_HACKY):
    """per graph: sum over its ordered pairs of delta_ij + 2^-20 (1 + ce_ij) - |d ce / d u| <= 1 carries the logit's error
    into the term, a few ulp of the fp32 softplus on top"""
    return np.asarray([float(((dl + 2.0 ** -20 * (1.0 + b["ce"])) * b["off"]).sum())
                       for b, dl in zip(ref["blocks"], delta(ref["blocks"], d, dist))])
