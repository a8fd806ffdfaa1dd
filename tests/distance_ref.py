"""The gradient of binary_loss' sum_loss with respect to the two parameters of sigmoid_l2, temp and shift
(include/gnf_distance.h, gnf_adj_loss_dist_f32), restated over tests/adj_loss_ref.py:

  closed form in float64    dL/dtemp = sum (p_ij - t_ij) w_ij,  dL/dshift = temp sum (p_ij - t_ij),  w_ij = shift - d2_ij scale,
                            over the ordered pairs i != j of every graph with |u_ij| < U (the clip passes no gradient)
  the same in float32       what an fp32 implementation can be expected to give: d2, w, u, p and p - t in float32 (numpy: no
                            fused multiply-add, features added in ascending order), the terms added in float64
  the bound between them    from adj_loss_ref.delta, which bounds what fp32 arithmetic moves a logit by

and the cases the GPU tests run (tests/test_distance_gpu.py), with the seed condition adj_loss_ref.pick_seed applies to them."""
import functools

import numpy as np

import adj_loss_ref as R

DISTS = (R.sigmoid_l2(3.0, 2.0), R.sigmoid_l2(20.0, 1.0), R.HACKY)   # (3, 2, scaled), (20, 1, scaled), (10, 1, unscaled)
GRAD_DIMS = (1, 7, 200, 400, 1030)   # 7, 200, 400, 1030: one per k_adj_loss_pairs instance (switches near D = 191, 330, 960)
GRAD_CASES = [(d, dist, soft) for d in GRAD_DIMS for dist in DISTS for soft in (False, True)]


def case_id(c):
    d, dist, soft = c
    return f"D{d}_t{dist[0]:g}_s{dist[1]:g}_{'scaled' if dist[2] else 'unscaled'}_{'soft' if soft else 'hard'}"


def _labels(a, soft, epsilon):
    return np.where(a, 1.0 - epsilon, epsilon) if soft else a.astype(np.float64)


def param_grads(z, sizes, senders, receivers, dist, soft=False, epsilon=0.1):
    """float64 (dL/dtemp, dL/dshift) of adj_loss_ref.binary_loss(...)["sum_loss"], closed form"""
    temp, shift, _ = dist
    scale = R._scale(dist, np.asarray(z).shape[1])
    dtemp = dsum = 0.0
    for b in R.graph_blocks(z, sizes, senders, receivers, dist):
        live = b["off"] & (np.abs(b["u"]) < R.U)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-b["u"]))
        e = np.where(live, p - _labels(b["a"], soft, epsilon), 0.0)
        dtemp += float((e * (shift - b["d2"] * scale)).sum())
        dsum += float(e.sum())
    return dtemp, temp * dsum


def param_grad_bounds(z, sizes, senders, receivers, dist, soft=False, epsilon=0.1):
    """(bound on |dtemp error|, bound on |dshift error|) of an fp32 implementation, over the pairs that contribute:
         dtemp   sum [(0.25 delta_ij + 2^-22) |w_ij| + |p_ij - t_ij| delta_ij / |temp|] + 2^-22 |dL/dtemp|
         dshift  |temp| sum (0.25 delta_ij + 2^-22) + 2^-22 |dL/dshift|
    0.25 is the sigmoid's largest slope (delta through it is p's error), 2^-22 covers expf, the division and the rounding
    of p - t, delta / |temp| is delta carried back to w, the last term the final rounding to fp32 (and to spare)."""
    temp, shift, _ = dist
    d = np.asarray(z).shape[1]
    scale = R._scale(dist, d)
    blocks = R.graph_blocks(z, sizes, senders, receivers, dist)
    ref_t, ref_s = param_grads(z, sizes, senders, receivers, dist, soft, epsilon)
    bt = bs = 0.0
    for b, dl in zip(blocks, R.delta(blocks, d, dist)):
        live = b["off"] & (np.abs(b["u"]) < R.U)
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-b["u"]))
        e = np.abs(p - _labels(b["a"], soft, epsilon))
        w = np.abs(shift - b["d2"] * scale)
        pe = 0.25 * dl + 2.0 ** -22
        bt += float(np.where(live, pe * w + e * dl / abs(temp), 0.0).sum())
        bs += float(np.where(live, pe, 0.0).sum())
    return bt + 2.0 ** -22 * abs(ref_t), abs(temp) * bs + 2.0 ** -22 * abs(ref_s)


def param_grads_f32(z, sizes, senders, receivers, dist, soft=False, epsilon=0.1):
    """the float32 restatement: every per-pair quantity in float32, the sums in float64"""
    f = np.float32
    z = np.asarray(z, f)
    d = z.shape[1]
    temp, shift = f(dist[0]), f(dist[1])
    scale = f(1.0) / np.sqrt(f(d)) if dist[2] else f(1.0)
    t1, t0 = (f(1.0) - f(epsilon), f(epsilon)) if soft else (f(1.0), f(0.0))
    dtemp = dsum = 0.0
    for b in R.graph_blocks(z, sizes, senders, receivers, dist):
        zg = z[b["n0"]:b["n0"] + b["ng"]]
        d2 = np.zeros((b["ng"], b["ng"]), f)
        for k in range(d):
            df = zg[:, None, k] - zg[None, :, k]
            d2 = d2 + df * df
        w = shift - d2 * scale
        u = temp * w
        with np.errstate(over="ignore"):
            p = f(1.0) / (f(1.0) + np.exp(-u))
        assert w.dtype == u.dtype == p.dtype == f
        e = p - np.where(b["a"], t1, t0).astype(f)
        live = b["off"] & (np.abs(u) < f(R.U))
        dtemp += float(np.where(live, e.astype(np.float64) * w.astype(np.float64), 0.0).sum())
        dsum += float(np.where(live, e.astype(np.float64), 0.0).sum())
    return dtemp, float(temp) * dsum


@functools.lru_cache(maxsize=None)
def grad_case(d, dist, soft):
    """(seed, z fp32, (n_edge, senders, receivers)) of a GPU gradient case: the first seed with margin, None if there is none"""
    return R.pick_seed(R.SIZES, d, dist)
