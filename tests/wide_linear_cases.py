"""Batches, nets and host-side restatements for tests/test_wide_linear_gpu.py (the wide-layer kernels of
csrc/gnf_linear_big.hip against the generic tile).

Everything restated here - the row deal of launch_linear_big_impl / launch_linear_short, the two "fits the LDS-resident
kernels" rules, the layer predicates of gnf_common.h and the layout of a net's packed copy - is used to CHOOSE a batch, to
assert a case's precondition before it runs, or to name a region of the packed buffer.  None of it is ever an expected
value: what the kernels compute is compared with what the generic tile (or the float64 oracle) computes."""
import copy

import numpy as np

from timestep_gnn_ref import ring_chord_batch


def pad16(v):
    return (int(v) + 15) // 16 * 16


# ---- which kernels a net can reach (gnf_common.h, gnf_fused.hip, gnf_fused_bwd.hip) ----------------------------------
def big_fwd_layer(i, o):
    return i >= 512 and o >= 256


def big_bwd_layer(i, o):
    return o >= 512 and i >= 256


def short_fwd_layer(i, o):
    return i <= 208 and i % 4 == 0 and o >= 256


def fused_last(dims, j):
    """layer j is the thin last layer the wide layer in front of it multiplies out of its accumulators"""
    return j >= 1 and j == len(dims) - 2 and dims[j + 1] <= 128 and big_fwd_layer(dims[j - 1], dims[j])


def fused_fwd_fits(dims):
    """fused_fits_lds: the LDS-resident forward kernel holds this net (then the layered path, and with it the wide
    kernels, never sees the forward or the inverse pass)"""
    ls = max(16, max(pad16(d) for d in dims)) + 4
    floats = 2 * 16 * ls + sum(pad16(d) for d in dims[1:]) + 2
    return 4 * floats + 8 * 8 + 4 * (8 * 8 + 40 + 2048) <= 160 * 1024


def fused_bwd_fits(dims):
    """fused_bwd_fits_lds: the LDS-resident backward kernel holds this net (then the generic walk never runs)"""
    k = len(dims) - 1
    wmax = max(16, max(pad16(d) for d in dims))
    bias = sum(pad16(d) for d in dims[1:]) + wmax
    mld = max([1] + [pad16(d) // 16 for d in dims[1:k]])
    floats = 4 * 16 * (wmax + 4) + 2 * bias
    floats += floats & 1
    hp = pad16(dims[k])
    return (4 * floats + 4 * (16 * 16 + 40 + 2048) + 2 * max(k - 1, 0) * 4 * mld * 8 + 4 * (40 + 2048)
            + 2 * 16 * hp * 4) <= 160 * 1024


def wide_only(dims):
    """gnf_optim.hip: only the copies with a reader among the wide kernels follow an optimiser step"""
    return not fused_fwd_fits(dims) and not fused_bwd_fits(dims)


def need_w(dims, j):
    i, o = dims[j], dims[j + 1]
    return not wide_only(dims) or big_fwd_layer(i, o) or fused_last(dims, j) or short_fwd_layer(i, o)


def need_wt(dims, j):
    return not wide_only(dims) or big_bwd_layer(dims[j], dims[j + 1])


# ---- the row deals (launch_linear_big_impl, launch_linear_short) ------------------------------------------------------
def big_deal(n, out_width, cus):
    """-> dict(rounds, wpp, wg_base, wg_rem, sizes) of k_linear_big for n rows and this output width, or None where the
    launcher answers "not my case"; sizes = the set of row tiles per workgroup (MW instances) the deal reaches"""
    n_rt = (n + 15) // 16
    panels = 2 * ((pad16(out_width) + 255) // 256)
    slots = 2 * cus
    units = n_rt * panels
    if units < 2 * slots:
        return None
    rounds = (units + 4 * slots - 1) // (4 * slots)
    wpp = (rounds * slots + panels - 1) // panels
    if wpp * 4 < n_rt:
        wpp = (n_rt + 3) // 4
    wpp = min(wpp, n_rt)
    base, rem = n_rt // wpp, n_rt % wpp
    if base + (1 if rem else 0) > 4 or base < 1:
        return None
    sizes = ({base + 1} if rem else set()) | ({base} if rem < wpp else set())
    return dict(rounds=rounds, wpp=wpp, wg_base=base, wg_rem=rem, sizes=sizes, n_rt=n_rt, panels=panels)


def short_deal(n, in_width, out_width, cus):
    """the same for k_linear_short (None: refused by the shape, or a batch too small)"""
    if not short_fwd_layer(in_width, out_width) or out_width % 4:
        return None
    ipg = pad16(in_width) // 16
    cols = 128 if ipg > 8 else 256
    n_rt = (n + 15) // 16
    panels = 2 * ((pad16(out_width) + cols - 1) // cols)
    if n_rt * panels < 2 * cus:
        return None
    slots = 2 * cus
    rounds = (n_rt * panels + 16 * slots - 1) // (16 * slots)
    wpp = min((rounds * slots + panels - 1) // panels, n_rt)
    inst = "7x4" if ipg <= 7 else "8x4" if ipg == 8 else "11x2" if ipg <= 11 else "13x2"
    return dict(rounds=rounds, wpp=wpp, wg_base=n_rt // wpp, wg_rem=n_rt % wpp, ipg=ipg, instance=inst, n_rt=n_rt,
                panels=panels)


# ---- a net's packed copy: [Wp_0 .. Wp_{K-1} | bias rows | WpT_0 .. WpT_{K-1}], padded-to-16 dims -----------------------
def packed_floats(dims):
    return sum(2 * pad16(i) * pad16(o) + pad16(o) for i, o in zip(dims[:-1], dims[1:]))


def packed_region(dims, kind, j):
    """(offset, length) in floats, inside one net's copy, of kind "w" | "b" | "wt" of layer j"""
    w = [pad16(i) * pad16(o) for i, o in zip(dims[:-1], dims[1:])]
    b = [pad16(o) for o in dims[1:]]
    if kind == "w":
        return sum(w[:j]), w[j]
    if kind == "b":
        return sum(w) + sum(b[:j]), b[j]
    return sum(w) + sum(b) + sum(w[:j]), w[j]


def net_index(kind, half, t_steps=1, step=0):
    """position of a net's copy in the flow's packed buffer: all s-nets (half * T + step), then all t-nets"""
    return (0 if kind == "s" else 2 * t_steps) + half * t_steps + step


# ---- nets and batches -----------------------------------------------------------------------------------------------------
def net_dims(d, latent, k, combine):
    h = d // 2
    return [2 * h if combine == "concat" else h] + [latent] * (k - 1) + [h]


def make_hp(d, latent, k=3, act="relu", combine="agg", t=1):
    return dict(D=d, latent=latent, K=k, T=t, agg="mean", combine=combine, epsilon=0.0 if combine == "concat" else 1.0,
                activation=act, weight_sharing=False)


def make_params(hp, seed):
    from oracle import gnf_oracle as O
    return O.make_grevnet_params(seed, hp["D"] // 2, hp["latent"], hp["K"], hp["T"], combine=hp["combine"], final_scale=0.3)


def doubled(params, half, j):
    """a copy of `params` with W_j of the s- and the t-net of one half-step (time step 0) times 2"""
    p = copy.deepcopy(params)
    for kind in ("s", "t"):
        layers = list(p[kind][half][0])
        w, b = layers[j]
        layers[j] = (np.asarray(w) * np.float32(2.0), b)
        p[kind][half][0] = layers
    return p


def ring_batch(n, size=37):
    """exactly n nodes: disjoint ring-plus-chord graphs of `size` nodes and one smaller graph for the rest"""
    sizes = [size] * (n // size) + ([n % size] if n % size else [])
    return ring_chord_batch(sizes, edgeless=())


def features(n, d, seed):
    return (np.random.default_rng(seed).standard_normal((n, d)) * 0.7).astype(np.float32)
