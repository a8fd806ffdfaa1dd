"""numpy / torch-CPU restatement of gnf_amd.gnn.TimestepGNN (include/gnf_timestep_gnn.h) with a `dtype` argument: float64 is
the reference the GPU tests compare against, float32 the yardstick whose own deviation from float64 sets their bounds.

Built on the oracle's module forward (oracle.gnf_oracle.Fp32Gather through tests/graph_attn_ref.GraphAttnGather, which adds
the graph-scope attention blocks) plus the norm formulas of the header:
  batch norm   mean, var = tf.nn.moments(x, [0]) (biased) or the moving statistics; inv = rsqrt(var + eps) * gamma;
               y = x * inv + (beta - mean * inv);  training: moving -= (moving - batch) * (1 - decay)
  layer norm   per row, biased variance, eps 1e-5, the same two-step arithmetic

Also here: the batches and parameter sets of the GPU tests, and pick_seed - a condition on the INPUTS: the first seed in
range(16) for which, in float64, no hidden pre-activation of any timestep lies closer to 0 than 4 x what the float32
restatement's value of that unit differs by.  An activation kink then cannot decide a comparison, and no element is ever
left out of one."""
import zlib
from collections import namedtuple

import numpy as np

from oracle import gnf_oracle as O
import graph_attn_ref as GA

BN_EPS, BN_DECAY = 1e-3, 0.999          # Sonnet-1 snt.BatchNorm defaults (UNPINNED upstream facts)
SIZES = [1, 17, 16, 33, 2]              # the whole-module batch: 69 nodes, the 2-node graph has no edges
DM_ATTN = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80, concat=True, kq_dim_division=False, residual=False)
GRAPH_ATTN = dict(num_heads=2, kq_dim=6, v_dim=5, out_dim=12, kq_dim_division=True)

# family: "avg" (avg_then_mlp, eps 2.0 as run_gnn.py:106-108, leaky_relu) | "sumcat" (sum_concat_then_mlp, relu) |
#         "dm" (dm_attn, relu) | "graph" (graph-scope multihead block, relu)
Case = namedtuple("Case", "family d latent k t bn ln residual sharing")


def case_id(c):
    return (f"{c.family}_D{c.d}_K{c.k}_T{c.t}" + ("_bn" if c.bn else "") + ("_ln" if c.ln else "") +
            ("_res" if c.residual else "") + ("_shared" if c.sharing else ""))


def _mk(family, d, k, bn, ln, residual, sharing, t=3, latent=32):
    return Case(family, d, latent, k, t, bn, ln, residual, sharing)


# every family under BN, BN + LN and LN only; D, K, residual and weight sharing alternate so that each value meets each family
MODULE_CASES = [
    _mk("avg", 6, 2, True, False, True, False), _mk("avg", 100, 3, True, True, False, True), _mk("avg", 100, 2, False, True, True, False),
    _mk("sumcat", 100, 2, True, False, False, True), _mk("sumcat", 6, 3, True, True, True, False), _mk("sumcat", 6, 2, False, True, False, True),
    _mk("dm", 6, 3, True, False, True, True), _mk("dm", 100, 2, True, True, True, False), _mk("dm", 100, 3, False, True, False, False),
    _mk("graph", 100, 3, True, False, False, False), _mk("graph", 6, 2, True, True, False, True), _mk("graph", 6, 3, False, True, True, True),
]


def family_kw(family):
    """Fp32Gather keywords of a family"""
    if family == "avg":
        return dict(agg="mean", combine="agg", epsilon=2.0, activation="leaky_relu")
    if family == "sumcat":
        return dict(agg="sum", combine="concat", epsilon=0.0, activation="relu")
    return dict(activation="relu")


def family_hp(c):
    """gnf_amd.encoder.make_encoder hyper-parameters of a case"""
    kw = family_kw(c.family)
    hp = dict(node_dim=c.d, latent=c.latent, K=c.k, activation=kw["activation"], agg=kw.get("agg", "sum"),
              combine=kw.get("combine", "agg"), epsilon=kw.get("epsilon", 0.0), num_timesteps=c.t, weight_sharing=c.sharing,
              use_batch_norm=c.bn, use_layer_norm=c.ln, residual=c.residual)
    if c.family == "dm":
        hp["attn"] = dict(DM_ATTN)
    elif c.family == "graph":
        hp["attn"] = dict(GRAPH_ATTN, scope="graph", layer_norm=False)
    return hp


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def ring_chord_batch(sizes, edgeless=(4,)):
    """(n_node, n_edge, senders, receivers): every graph a ring in both directions plus the chords i -> i + 3 (directed, so
    in-degrees differ from out-degrees); a one-node graph is one self loop; the graphs listed in `edgeless` have no edges."""
    s_l, r_l, ne, off = [], [], [], 0
    for g, m in enumerate(sizes):
        pairs = set()
        if g not in edgeless:
            if m == 1:
                pairs.add((0, 0))
            for i in range(m if m > 2 else m - 1):
                pairs.add((i, (i + 1) % m))
                pairs.add(((i + 1) % m, i))
            if m > 6:
                for i in range(0, m, 2):
                    pairs.add((i, (i + 3) % m))
        pairs = sorted(pairs)
        s_l.append(np.array([u for u, _ in pairs], np.int32) + off)
        r_l.append(np.array([v for _, v in pairs], np.int32) + off)
        ne.append(len(pairs))
        off += m
    return (np.array(sizes, np.int32), np.array(ne, np.int32), np.concatenate(s_l).astype(np.int32),
            np.concatenate(r_l).astype(np.int32))


def make_params(c):
    """{"nets": [...], "bn": [...], "ln": [...]} of a case: non-trivial in every variable (trained values are what matters)"""
    seed = zlib.crc32(repr(tuple(c)).encode()) % 9973
    rng = np.random.default_rng(seed)
    n_nets = 1 if c.sharing else c.t

    def net():
        if c.family == "dm":
            return O.make_attn_net_params(rng, c.d, c.latent, c.k, final_scale=0.5, **DM_ATTN)
        if c.family == "graph":
            return GA.make_graph_attn_net_params(rng, c.d, c.latent, c.k, final_scale=0.5, **GRAPH_ATTN)
        in_dim = 2 * c.d if c.family == "sumcat" else c.d
        return O.make_mlp_params(rng, in_dim, c.latent, c.d, c.k, final_scale=0.5)
    p = {"nets": [net() for _ in range(n_nets)]}
    if c.bn:
        p["bn"] = make_bn_params(rng, c.d, c.t)
    if c.ln:
        p["ln"] = make_ln_params(rng, c.d, c.t)
    return p


def make_bn_params(rng, d, t):
    return [{"gamma": rng.uniform(0.5, 1.5, d).astype(np.float32), "beta": (0.2 * rng.standard_normal(d)).astype(np.float32),
             "moving_mean": (0.3 * rng.standard_normal(d)).astype(np.float32),
             "moving_variance": rng.uniform(0.5, 2.0, d).astype(np.float32)} for _ in range(t)]


def make_ln_params(rng, d, t):
    return [{"gamma": rng.uniform(0.5, 1.5, d).astype(np.float32), "beta": (0.2 * rng.standard_normal(d)).astype(np.float32)}
            for _ in range(t)]


def module_inputs(c, seed):
    return np.random.default_rng(1000 + seed).standard_normal((int(np.sum(SIZES)), c.d)).astype(np.float32)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def batch_norm(x, bn, use_batch_stats, eps=BN_EPS):
    """torch, in x's dtype: (y, mean, var) - tf.nn.moments then tf.nn.batch_normalization"""
    import torch
    if use_batch_stats:
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)   # biased
    else:
        mean, var = bn["moving_mean"], bn["moving_variance"]
    inv = torch.rsqrt(var + eps) * bn["gamma"]
    return x * inv + (bn["beta"] - mean * inv), mean, var


def moving_update(moving, batch, decay=BN_DECAY):
    """assign_moving_average without zero-debias, in moving's dtype (the rate 1 - decay formed in that dtype too)"""
    one = moving.new_tensor(1.0)
    return moving - (moving - batch) * (one - moving.new_tensor(decay))


def layer_norm(x, ln):
    import torch
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    inv = torch.rsqrt(var + O.LN_EPS) * ln["gamma"]
    return x * inv + (ln["beta"] - mean * inv)


class _Recording(GA.GraphAttnGather):
    """the oracle's module forward that also keeps every hidden pre-activation: pre[(call, layer)] = [n, L]"""

    def mlp(self, h, layers):
        call, a = getattr(self, "_mlp_calls", -1) + 1, h
        for j, (w, b) in enumerate(layers[:-1]):
            a = a @ w + b
            self.pre[call, j] = a.numpy().astype(np.float64)
            a = self.act(a)
        return super().mlp(h, layers)


def forward(batch, x, params, t, dtype, family="avg", weight_sharing=False, residual=True, is_training=False,
            test_local_stats=False, eps=BN_EPS, decay=BN_DECAY, gnn_kw=None):
    """TimestepGNN._build (gnn.py:217-235) in `dtype` (np.float64 / np.float32).  batch = (n_node, n_edge, senders, receivers).
    Returns dict(out [n, D] float64 array, moments [(mean, var)] * T (None entries where the moving statistics normalised),
    moving [(mean, var)] * T after the call, pre {(timestep, layer): hidden pre-activations})."""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    n_node, _, s, r = batch
    o = _Recording(s, r, n_node, dtype=tdt, **(gnn_kw if gnn_kw is not None else family_kw(family)))
    o.pre = {}
    pt = o.prep_params({k: v for k, v in params.items() if k == "nets"})
    conv = lambda lst: [{k: o.to_t(v) for k, v in d.items()} for d in lst]
    bns = conv(params["bn"]) if params.get("bn") else None
    lns = conv(params["ln"]) if params.get("ln") else None
    x0 = o.to_t(x)
    nodes, moments, moving = x0, [], []
    with torch.no_grad():
        for i in range(t):
            if bns:
                local = is_training or test_local_stats
                nodes, mean, var = batch_norm(nodes, bns[i], local, eps)
                moments.append((mean.numpy().astype(np.float64), var.numpy().astype(np.float64)) if local else None)
                mm, mv = bns[i]["moving_mean"], bns[i]["moving_variance"]
                if is_training:
                    mm, mv = moving_update(mm, mean, decay), moving_update(mv, var, decay)
                moving.append((mm.numpy().astype(np.float64), mv.numpy().astype(np.float64)))
            if lns:
                nodes = layer_norm(nodes, lns[i])
            nodes = o.gnn(nodes, pt["nets"][0 if weight_sharing else i])
        if residual:
            nodes = nodes + x0
    return dict(out=nodes.numpy().astype(np.float64), moments=moments, moving=moving, pre=o.pre)


def run_case(c, x, dtype, is_training=False, test_local_stats=False, params=None):
    return forward(ring_chord_batch(SIZES), x, make_params(c) if params is None else params, c.t, dtype, c.family, c.sharing,
                   c.residual, is_training, test_local_stats)


def margin_ok(pre64, pre32):
    """no hidden unit's float64 pre-activation closer to 0 than 4 x what float32 moved that unit by"""
    return all((np.abs(pre64[k]) >= 4.0 * np.abs(pre32[k] - pre64[k])).all() for k in pre64)


_PICKED = {}


def pick_seed(c, is_training=True, test_local_stats=False):
    """(seed, x, ref64, ref32) for the first seed in range(16) whose inputs satisfy margin_ok on case c, (None, ...) if there
    is none.  Cached: the references are computed once and shared; callers must not change them."""
    key = (c, is_training, test_local_stats)
    if key not in _PICKED:
        params = make_params(c)
        found = (None, None, None, None)
        for seed in range(16):
            x = module_inputs(c, seed)
            r64 = run_case(c, x, np.float64, is_training, test_local_stats, params)
            r32 = run_case(c, x, np.float32, is_training, test_local_stats, params)
            if margin_ok(r64["pre"], r32["pre"]):
                found = (seed, x, r64, r32)
                break
        _PICKED[key] = found
    return _PICKED[key]


# ---- the norm stage alone: an edgeless batch and the identity net --------------------------------------------------------------
NORM_SIZES = {"b5_1_11": [5, 1, 11], "n1": [1], "n32": [32], "n33": [33], "n513": [513]}
NORM_WIDTHS = (1, 2, 6, 64, 100, 130, 257)


def norm_inputs(n, d):
    """fp32 [n, d]: N(0, 1); column 0 constant 0.75 (variance exactly 0); with d >= 2, column 1 = 100 + 0.1 N(0, 1) (a mean
    1e3 times its spread: an fp32 moment sum loses the variance)"""
    rng = np.random.default_rng(7 * n + d)
    x = rng.standard_normal((n, d))
    x[:, 0] = 0.75
    if d >= 2:
        x[:, 1] = 100.0 + 0.1 * x[:, 1]
    return x.astype(np.float32)


def identity_net(d):
    return [(np.eye(d, dtype=np.float32), np.zeros(d, np.float32))]


def edgeless_batch(sizes):
    return (np.array(sizes, np.int32), np.zeros(len(sizes), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))


def norm_only(x, bn, ln, dtype, is_training=True, test_local_stats=False):
    """the norm stage of one timestep on its own (what the identity net on an edgeless batch passes through)"""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    conv = lambda d: {k: torch.as_tensor(np.asarray(v), dtype=tdt) for k, v in d.items()}
    y = torch.as_tensor(np.asarray(x), dtype=tdt)
    out = {}
    if bn is not None:
        b = conv(bn)
        y, mean, var = batch_norm(y, b, is_training or test_local_stats)
        out["mean"], out["var"] = mean.numpy().astype(np.float64), var.numpy().astype(np.float64)
        if is_training:
            out["moving_mean"] = moving_update(b["moving_mean"], mean).numpy().astype(np.float64)
            out["moving_variance"] = moving_update(b["moving_variance"], var).numpy().astype(np.float64)
    if ln is not None:
        y = layer_norm(y, conv(ln))
    out["y"] = y.numpy().astype(np.float64)
    return out


def z_bound(ref64, ref32):
    """tests/batch_norm_routes.py's rule for z: the larger of 5e-4 max(1, |ref|max) and 4 x the float32 restatement's own
    maximum deviation from float64 on the same case"""
    return max(5e-4 * max(1.0, float(np.abs(ref64).max())), 4.0 * float(np.abs(ref32 - ref64).max()))
