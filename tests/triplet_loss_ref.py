"""numpy restatement of what gnf_amd.triplet_loss.triplet_loss computes (include/gnf_triplet_loss.h): the reference's sampled
triplet loss (loss.py:221-270) with the header's random stream, graph by graph, with a `dtype` argument - float64 is the
reference the GPU tests compare against, float32 the yardstick whose own deviation from float64 enters their bounds.

Here: the hash and the candidate rule in Python integers; the six scores and the two losses; per-node, per-graph and total
sums and the skipped counts; the gradient by the closed forms; `triplet_loss_literal`, which follows loss.py:242-270 to the
letter on dense [N, N] matrices given the chosen indices (tests/test_triplet_loss_cpu.py holds the two against each other);
the test batches; and `pick_seed`, a condition on the INPUTS: every hinge argument margin - p + q and every p + q of the
relative loss is either exactly 0 in both precisions or stays a gap away from 0, the gap derived from the fp32-against-float64
difference of the restated scores, so that no kink can flip on the device.  No term is ever left out of a comparison."""
import functools

import numpy as np

import adj_loss_ref as AL

M64 = (1 << 64) - 1
SIZES = AL.SIZES + [130]        # + a graph whose rows span 3 bitmap words
COMPLETE, EDGELESS = 9, 5       # appended by batch(): a complete graph (no negatives) and an edgeless one (no positives)

L2, DOT, EXP_L2, CAUCHY, SIGMOID_DOT = ("l2",), ("dot",), ("exp_l2",), ("hacky_cauchy_l2",), ("sigmoid_dot",)
HACKY = ("sigmoid_l2", 10.0, 1.0, False)           # loss.py:36-42
SCALED_HACKY = ("sigmoid_l2", 10.0, 1.0, True)     # loss.py:45-53
SCORES = {"l2": L2, "dot": DOT, "exp_l2": EXP_L2, "hacky_sigmoid_l2": HACKY, "hacky_cauchy_l2": CAUCHY, "sigmoid_dot": SIGMOID_DOT}
MARGIN, RELATIVE = ("margin", 0.65), ("relative",)


def sigmoid_l2(temp, shift):    # loss.py:56-62
    return ("sigmoid_l2", float(temp), float(shift), True)


# ---- the random stream -----------------------------------------------------------------------------------------------------
def hash_draw(seed, l, which, i):
    """the 32-bit draw of (seed, l, which, i), in Python integers"""
    x = (seed ^ (0x9E3779B97F4A7C15 * (i + 1)) ^ (0xBF58476D1CE4E5B9 * (2 * l + which + 1))) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def hash_draws(seed, loops, n):
    """uint32 [L, 2, N]: what the device draws without a `draws` tensor"""
    return np.asarray([[[hash_draw(int(seed) & M64, l, w, i) for i in range(n)] for w in (0, 1)] for l in range(loops)],
                      np.uint32).reshape(loops, 2, n)


def choose(r, cnt):
    """candidate number of draw r among cnt"""
    return (int(r) * int(cnt)) >> 32


def candidates(sizes, senders, receivers, self_loops="keep"):
    """per node (positives: the receivers of its out-edges inside its graph, in edge order, with multiplicity; negatives: the
    other nodes of its graph without an edge from it, ascending)"""
    n = int(np.sum(sizes))
    senders, receivers = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    rows = [[] for _ in range(n)]
    for s, r in zip(senders.tolist(), receivers.tolist()):
        rows[s].append(r)
    out, o = [], 0
    for ng in sizes:
        for i in range(o, o + ng):
            pos = [j for j in rows[i] if o <= j < o + ng and not (self_loops == "skip" and j == i)]
            taken = set(pos) | {i}
            out.append((pos, [j for j in range(o, o + ng) if j not in taken]))
        o += ng
    return out


def sample(sizes, senders, receivers, draws, self_loops="keep"):
    """(pos, neg) int32 [L, N] of the draws uint32 [L, 2, N]: -1 for a node without a candidate of either kind"""
    draws = np.asarray(draws)
    loops, n = draws.shape[0], draws.shape[2]
    pos, neg = np.full((loops, n), -1, np.int32), np.full((loops, n), -1, np.int32)
    rows = [[] for _ in range(n)]
    for s, r in zip(np.asarray(senders, np.int64).tolist(), np.asarray(receivers, np.int64).tolist()):
        rows[s].append(r)
    o = 0
    for ng in sizes:   # candidates() without the negatives' lists (a 4000-node ring): the k-th node that is not taken
        for i in range(o, o + ng):
            cp = [j for j in rows[i] if o <= j < o + ng and not (self_loops == "skip" and j == i)]
            taken = sorted(set(cp) | {i})
            if not cp or len(taken) == ng:
                continue
            for l in range(loops):
                pos[l, i] = cp[choose(draws[l, 0, i], len(cp))]
                j = o + choose(draws[l, 1, i], ng - len(taken))
                for t in taken:
                    if t > j:
                        break
                    j += 1
                neg[l, i] = j
        o += ng
    return pos, neg


# ---- scores and losses -----------------------------------------------------------------------------------------------------
def is_dot(score):
    return score[0] in ("dot", "sigmoid_dot")


def score_of(score, x, d, dtype=np.float64):
    """(s, ds / dx) of x = d2 or dot, in `dtype`"""
    f = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    with np.errstate(over="ignore", under="ignore"):
        if score[0] in ("l2", "dot"):
            return x, np.ones_like(x)
        if score[0] == "exp_l2":
            s = np.exp(-x)
            return s, -s
        if score[0] == "sigmoid_l2":
            scale = f(1.0) / np.sqrt(f(d)) if score[3] else f(1.0)
            s = f(1.0) / (f(1.0) + np.exp(-(f(score[1]) * (f(score[2]) - x * scale))))
            return s, -(f(score[1]) * scale) * (s * (f(1.0) - s))
        if score[0] == "hacky_cauchy_l2":
            a = -(x - f(4.0))
            return np.arctan(a) * f(1.0 / np.pi) + f(0.5), -f(1.0 / np.pi) / (f(1.0) + a * a)
        if score[0] == "sigmoid_dot":
            s = f(1.0) / (f(1.0) + np.exp(-(x - f(0.5))))
            return s, s * (f(1.0) - s)
    raise ValueError(score)


def _pair_x(z, i, j, dot):
    """d2 or dot of the pairs (i, j), the features in ascending order, in z's dtype"""
    acc = np.zeros(len(i), z.dtype)
    for f in range(z.shape[1]):
        a, b = z[i, f], z[j, f]
        acc = acc + (a * b if dot else (a - b) * (a - b))
    return acc


def triplet_loss(z, sizes, senders, receivers, score=L2, loss=MARGIN, loops=8, seed=0, draws=None, self_loops="keep",
                 dtype=np.float64, indices=None):
    """Returns dict(pos, neg [L, N] (-1 where the term is skipped), loss_per_node [N], loss_per_graph [B], sum_loss, mean_loss,
    skipped int64 [B], grad (d sum_loss / d z, [N, D]), kink [L, N]: the hinge argument / p + q of every term with candidates
    (nan elsewhere), p, q [L, N]).  Scores, terms, coefficients and the gradient's sums are evaluated in `dtype`; the loss sums are
    float64 (as on the device).  indices =
    (pos, neg) overrides the sampling."""
    z = np.asarray(z, dtype)
    n, d = z.shape
    if indices is None:
        if draws is None:
            draws = hash_draws(seed, loops, n)
        indices = sample(sizes, senders, receivers, draws, self_loops)
    pos, neg = (np.array(a, np.int32) for a in indices)
    loops = pos.shape[0]
    dot = is_dot(score)
    term, kink = np.zeros((loops, n)), np.full((loops, n), np.nan)
    ps, qs = np.full((loops, n), np.nan), np.full((loops, n), np.nan)
    grad = np.zeros((n, d), dtype)
    for l in range(loops):
        i = np.flatnonzero(pos[l] >= 0)
        if not len(i):
            continue
        jp, jn = pos[l, i].astype(np.int64), neg[l, i].astype(np.int64)
        p, dp = score_of(score, _pair_x(z, i, jp, dot), d, dtype)
        q, dq = score_of(score, _pair_x(z, i, jn, dot), d, dtype)
        own = jp == i
        p, dp = np.where(own, 0, p).astype(dtype), np.where(own, 0, dp).astype(dtype)   # the zeroed diagonal
        if loss[0] == "margin":
            t = (np.dtype(dtype).type(loss[1]) - p) + q
            on = t > 0
            kept = np.ones(len(i), bool)
            tv, cp, cq = np.where(on, t, 0), np.where(on, -dp, 0), np.where(on, dq, 0)
            kink[l, i] = t
        else:
            s = p + q
            kept = s != 0
            with np.errstate(divide="ignore", invalid="ignore"):
                tv, cp, cq = np.where(kept, p / s, 0), np.where(kept, ((q / s) / s) * dp, 0), np.where(kept, -((p / s) / s) * dq, 0)
            kink[l, i] = s
        ps[l, i], qs[l, i] = p, q
        term[l, i] = np.asarray(tv, np.float64)
        pos[l, i[~kept]] = neg[l, i[~kept]] = -1
        two = np.dtype(dtype).type(2.0)
        for j, c in ((jp, np.asarray(cp, dtype)), (jn, np.asarray(cq, dtype))):   # (the gradient too accumulates in `dtype`)
            use = (c != 0) & (j != i)
            ii, jj, cc = i[use], j[use], c[use][:, None]
            if dot:
                np.add.at(grad, ii, cc * z[jj])
                np.add.at(grad, jj, cc * z[ii])
            else:
                np.add.at(grad, ii, two * cc * (z[ii] - z[jj]))
                np.add.at(grad, jj, two * cc * (z[jj] - z[ii]))
    per_node = term.sum(0)
    per_graph, skipped, o = [], [], 0
    for ng in sizes:
        per_graph.append(float(per_node[o:o + ng].sum()))
        skipped.append(int((pos[:, o:o + ng] < 0).sum()))
        o += ng
    total, kept_terms = float(np.sum(per_graph)), n * loops - int(np.sum(skipped))
    return dict(pos=pos, neg=neg, loss_per_node=per_node, loss_per_graph=np.asarray(per_graph), sum_loss=total,
                mean_loss=total / kept_terms if kept_terms else 0.0, skipped=np.asarray(skipped, np.int64), grad=grad.astype(np.float64), kink=kink,
                p=ps, q=qs, loss=loss, sizes=list(sizes))


def triplet_loss_literal(z, sizes, senders, receivers, score, loss, pos, neg):
    """loss.py:242-270 on dense [N, N] matrices in float64, with sample_examples' gather at the given indices (a skipped term,
    index -1, adds 0).  Returns (unreduced_loss [N], true_adj, inv_true_adj): the two matrices are what the reference samples
    from - the caller checks that every chosen index has weight there."""
    z = np.asarray(z, np.float64)
    n, d = z.shape
    true_adj = np.zeros((n, n))
    np.add.at(true_adj, (np.asarray(senders, np.int64), np.asarray(receivers, np.int64)), 1.0)   # the einsum of loss.py:66-70
    lm, o = np.zeros((n, n)), 0
    for ng in sizes:
        lm[o:o + ng, o:o + ng] = 1.0
        o += ng
    inv = lm * ((1.0 - np.eye(n)) * (1.0 - true_adj))
    r = (z * z).sum(1)[:, None]
    dist2, gram = r - 2.0 * z @ z.T + r.T, z @ z.T
    with np.errstate(over="ignore"):
        if score[0] == "l2":
            dm = dist2
        elif score[0] == "dot":
            dm = gram
        elif score[0] == "exp_l2":
            dm = np.exp(-dist2)
        elif score[0] == "sigmoid_l2":
            dm = 1.0 / (1.0 + np.exp(-(score[1] * (score[2] - (dist2 / np.sqrt(d) if score[3] else dist2)))))
        elif score[0] == "hacky_cauchy_l2":
            dm = (1.0 / np.pi) * np.arctan(-1.0 * (dist2 - 4.0)) + 0.5
        else:
            dm = 1.0 / (1.0 + np.exp(-(gram - 0.5)))
    dm = (1.0 - np.eye(n)) * dm
    total, rows = np.zeros(n), np.arange(n)
    for l in range(pos.shape[0]):
        ok = pos[l] >= 0
        p, q = dm[rows[ok], pos[l, ok]], dm[rows[ok], neg[l, ok]]
        total[ok] += np.maximum(loss[1] - p + q, 0.0) if loss[0] == "margin" else p / (p + q)
    return total, true_adj, inv


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def embeddings(sizes, d, seed):
    """fp32 [N, d]: N(0, 1) * sqrt(0.5 / d) - squared distances around 1, where every score has slope"""
    n = int(np.sum(sizes))
    return (np.random.default_rng(seed).standard_normal((n, d)) * np.sqrt(0.5 / d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(graph_seed=0):
    """(sizes, n_edge, senders, receivers): adj_loss_ref.true_graph on SIZES (directed, three duplicated edges per graph) with
    the self loops of every other node removed, then a complete graph of COMPLETE nodes and an edgeless one of EDGELESS"""
    n_edge, s, r = AL.true_graph(SIZES, graph_seed)
    keep = ~((s == r) & (s % 2 == 1))
    eg = np.repeat(np.arange(len(SIZES)), n_edge)
    n_edge = np.bincount(eg[keep], minlength=len(SIZES)).astype(np.int32)
    s, r = s[keep], r[keep]
    o = int(np.sum(SIZES))
    cs, cr = np.nonzero(~np.eye(COMPLETE, dtype=bool))
    sizes = list(SIZES) + [COMPLETE, EDGELESS]
    return (sizes, np.concatenate([n_edge, [len(cs), 0]]).astype(np.int32), np.concatenate([s, cs + o]).astype(np.int32),
            np.concatenate([r, cr + o]).astype(np.int32))


# ---- the margin condition and the bounds -----------------------------------------------------------------------------------
FLOOR = 2.0 ** -100   # far above where fp32 flushes a sum to zero, far below any score the test batches produce


def margin_ok(r64, r32):
    """every term with candidates: its kink argument (margin - p + q, or p + q) is exactly 0 in both precisions, or stays
    4 (|p32 - p64| + |q32 - q64|) + 2^-20 (|p| + |q| + |margin|) + FLOOR away from 0 in both - 4 x what fp32 arithmetic moved the
    two scores by in the restatement, and 16 ulp of the operands' size for the device's own rounding (the relative loss has no
    margin operand: its p + q only has to stay a nonzero fp32 number)"""
    has = ~np.isnan(r64["kink"])
    k64, k32 = r64["kink"][has], r32["kink"][has]
    gap = 4.0 * (np.abs(r32["p"][has] - r64["p"][has]) + np.abs(r32["q"][has] - r64["q"][has])) \
        + 2.0 ** -20 * (np.abs(r64["p"][has]) + np.abs(r64["q"][has]) + (abs(r64["loss"][1]) if r64["loss"][0] == "margin" else 0.0)) + FLOOR
    zero = (k64 == 0) & (k32 == 0)
    return bool((zero | ((np.abs(k64) >= gap) & (np.abs(k32) >= gap))).all())


@functools.lru_cache(maxsize=None)
def pick_seed(d, score=L2, loss=MARGIN, loops=8, self_loops="keep", graph_seed=0):
    """(seed, z, ref64, ref32): the first seed in range(16) - it seeds the embeddings and the hash alike - whose batch satisfies
    margin_ok; (None, ...) if there is none.  Cached: callers must not change the references."""
    sizes, _, s, r = batch(graph_seed)
    for seed in range(16):
        z = embeddings(sizes, d, seed)
        idx = sample(sizes, s, r, hash_draws(seed, loops, len(z)), self_loops)
        r64 = triplet_loss(z, sizes, s, r, score, loss, indices=idx)
        r32 = triplet_loss(z, sizes, s, r, score, loss, indices=idx, dtype=np.float32)
        if margin_ok(r64, r32):
            return seed, z, r64, r32
    return None, None, None, None


KEYS = ("loss_per_node", "loss_per_graph", "sum_loss", "grad")


def bounds(r64, r32):
    """per output: 4 x the float32 restatement's own deviation from float64 (the rule of tests/timestep_gnn_grad_ref.bounds)
    plus 16 fp32 ulp of the output's size: the device rounds expf / atanf and its fmaf chain differently from numpy, and where
    fp32 happens to be exact (D = 1, a score that is its argument) the first part alone would be zero.
    loss_per_node, grad: the largest deviation / the largest entry of the tensor.  loss_per_graph, sum_loss: these add node
    losses up, so their yardstick is the SUM of the nodes' absolute deviations / absolute values (per graph: the largest such
    sum) - the deviation of the float32 sum itself is no yardstick, since the nodes' rounding errors are independent and how
    far they cancel in one float32 run says nothing about another (dot with relative_loss has terms p / (p + q) of size 1e3
    beside thousands of size 1)."""
    n64, n32 = np.asarray(r64["loss_per_node"], np.float64), np.asarray(r32["loss_per_node"], np.float64)
    dev, size = np.abs(n64 - n32), np.abs(n64)
    ends = np.cumsum([0] + list(r64["sizes"]))
    per_graph = [(float(dev[a:b].sum()), float(size[a:b].sum())) for a, b in zip(ends[:-1], ends[1:])]
    g64, g32 = np.asarray(r64["grad"], np.float64), np.asarray(r32["grad"], np.float64)
    rule = lambda d, v: 4.0 * d + 2.0 ** -20 * v
    return {"loss_per_node": rule(float(dev.max(initial=0.0)), float(size.max(initial=0.0))),
            "loss_per_graph": rule(max(d for d, _ in per_graph), max(v for _, v in per_graph)),
            "sum_loss": rule(float(dev.sum()), float(size.sum())),
            "grad": rule(float(np.abs(g64 - g32).max(initial=0.0)), float(np.abs(g64).max(initial=0.0)))}
