"""Shared by tests/test_backward_routes_gpu.py and tests/test_backward_routes_cpu.py: directed, skewed batches for the
message-passing backward walk without batch norm (gnf_grevnet_backward_f32), the float64 / float32 oracle pair of one case
(computed once, shared by every route of that case), one device run of a (case, route) and the two-tier comparison of its
gradients.  Report, flat_grads, the kink band and the side fit are tests/batch_norm_routes.py's."""
import zlib
from collections import namedtuple

import numpy as np

import batch_norm_routes as B
from oracle import gnf_oracle as O

DEV = B.DEV
Report = B.Report

# graphs: ((generator, nodes), ...); band: the most hidden units the case's seed may leave inside the oracle's kink band
Case = namedtuple("Case", "name graphs d latent k t agg combine eps act ws band")


# ---- topologies: one generator per graph, directed edges, (senders, receivers) local to the graph ------------------------
def _ring(m):
    i = np.arange(m)
    return i, (i + 1) % m          # (one node: a self loop)


def ring_directed(m, rng):
    """i -> i + 1 only, plus m random directed edges (duplicates and self loops as they come)."""
    s, r = _ring(m)
    return np.concatenate([s, rng.integers(0, m, size=m)]), np.concatenate([r, rng.integers(0, m, size=m)])


def star_in(m, rng):
    """every node -> node 0 (node 0 included), plus the directed ring: one receiver row of m edges"""
    s, r = _ring(m)
    return np.concatenate([np.arange(m), s]), np.concatenate([np.zeros(m, np.int64), r])


def star_out(m, rng):
    """node 0 -> every node (node 0 included), plus the directed ring: one sender row of m edges"""
    s, r = _ring(m)
    return np.concatenate([np.zeros(m, np.int64), s]), np.concatenate([np.arange(m), r])


def empty(m, rng):
    """m isolated nodes: rows of in-degree 0 (the mean aggregator divides by max(in-degree, 1))"""
    return np.zeros(0, np.int64), np.zeros(0, np.int64)


def make_batch(graphs, rng):
    """n_node, n_edge, senders, receivers of the batch; the edge order inside each graph is shuffled with `rng`."""
    s_l, r_l, nn, ne, off = [], [], [], [], 0
    for gen, m in graphs:
        s, r = gen(m, rng)
        order = rng.permutation(len(s))
        s_l.append(s[order] + off)
        r_l.append(r[order] + off)
        nn.append(m)
        ne.append(len(s))
        off += m
    return (np.array(nn, np.int32), np.array(ne, np.int32), np.concatenate(s_l).astype(np.int32),
            np.concatenate(r_l).astype(np.int32))


# ---- cases: the smallest shapes at which each branch of the walk exists -----------------------------------------------
def _big(n_empty):
    return (ring_directed, 1500), (star_in, 70), (empty, n_empty), (ring_directed, 1500)


def _wide(m):
    return (ring_directed, 2000), (star_out, m), (ring_directed, 2000)


CASES = [
    #    name       graphs                                              D  latent K  T  agg     combine   eps  activation    ws     band
    Case("n1", ((ring_directed, 1),), 6, 16, 1, 1, "mean", "agg", 0.5, "relu", False, 0),
    Case("noedges", ((empty, 5),), 8, 16, 3, 2, "sum", "concat", 0.0, "leaky_relu", True, 0),
    Case("n17", ((ring_directed, 1), (empty, 3), (ring_directed, 13)), 10, 24, 1, 3, "sum", "agg", 1.0, "leaky_relu", False, 0),
    Case("n33", ((ring_directed, 20), (empty, 2), (star_in, 11)), 8, 20, 3, 3, "mean", "concat", 0.0, "relu", True, 0),
    Case("star_in", ((star_in, 2100), (ring_directed, 37)), 8, 16, 2, 2, "mean", "agg", 0.0, "leaky_relu", False, 16),
    Case("star_out", ((star_out, 2100), (ring_directed, 37)), 6, 16, 2, 2, "sum", "agg", 0.5, "relu", False, 16),
    Case("n3072", _big(2), 6, 16, 3, 1, "mean", "agg", 1.0, "leaky_relu", False, 16),
    Case("n3073", _big(3), 8, 24, 2, 2, "sum", "concat", 1.0, "relu", False, 16),
    Case("n4096", _wide(96), 10, 16, 2, 2, "mean", "agg", 0.5, "leaky_relu", True, 16),
    Case("n4097", _wide(97), 8, 16, 3, 2, "sum", "agg", 1.0, "relu", False, 16),
]
BY_NAME = {c.name: c for c in CASES}


def n_nodes(c):
    return sum(m for _, m in c.graphs)


def final_scale(c):
    """0.05 under the sum aggregator (a receiver row of tens of edges), 0.3 under the mean: the randomised sweep's - 0.1 under
    the mean with weight sharing, where the same net's scale compounds over the T steps (n4096 at 0.3 and T = 3: |z| past 50)."""
    return 0.05 if c.agg == "sum" else 0.1 if c.ws else 0.3


# ---- problem, seed, reference ---------------------------------------------------------------------------------------------
_SEEDED, _PICKED, _REFS = {}, {}, {}


def seeded_problem(c, seed):
    """The case's batch, inputs and weights under one seed (topology, edge order, x and the nets all depend on it)."""
    if (c, seed) in _SEEDED:
        return _SEEDED[c, seed]
    base = zlib.crc32(c.name.encode())
    rng = np.random.default_rng([base, seed])
    nn, ne, s, r = make_batch(c.graphs, rng)
    n = n_nodes(c)
    hp = dict(D=c.d, latent=c.latent, K=c.k, T=c.t, agg=c.agg, combine=c.combine, epsilon=c.eps, activation=c.act,
              weight_sharing=c.ws)
    p = O.make_grevnet_params(base % 9973 + seed, c.d // 2, c.latent, c.k, c.t, combine=c.combine, weight_sharing=c.ws,
                              final_scale=final_scale(c))
    pr = dict(nn=nn, ne=ne, s=s, r=r, n=n, x=rng.standard_normal((n, c.d)).astype(np.float32), hp=hp, p=p, ws=c.ws,
              kw=dict(agg=c.agg, combine=c.combine, epsilon=c.eps, activation=c.act), seed=seed)
    _SEEDED[c, seed] = pr
    return pr


def kink_band(pr, t):
    """batch_norm_routes.reference's band: hidden units whose float64 pre-activation lies within max(2e-5, 4 x what the
    float32 oracle's pre-activations differ from the float64 ones by) of zero."""
    import torch
    _, _, pre64 = B._gather_run(pr, t, torch.float64, False)
    _, _, pre32 = B._gather_run(pr, t, torch.float32, False)
    tol = max([2e-5] + [4.0 * float(np.abs(pre32[k] - pre64[k]).max()) for k in pre64])
    units = [(k, int(v), int(u)) for k in sorted(pre64) for v, u in zip(*np.nonzero(np.abs(pre64[k]) < tol))]
    total = sum(v.size for v in pre64.values())
    return dict(tol=tol, units=units, sides={k: pre64[k] > 0 for k in {k for k, _, _ in units}}, total=total)


def pick_seed(c):
    """The first seed in range(16) whose kink band holds at most c.band hidden units (0 for the small cases: the side fit
    never runs there; 16 for the four-digit ones: a fit costs at most 16 autograd runs).  (seed, problem, band) or None."""
    if c not in _PICKED:
        _PICKED[c] = None
        for seed in range(16):
            pr = seeded_problem(c, seed)
            kink = kink_band(pr, c.t)
            if len(kink["units"]) <= c.band:
                _PICKED[c] = (seed, pr, kink)
                break
    return _PICKED[c]


def problem(c):
    picked = pick_seed(c)
    assert picked is not None, f"{c.name}: no seed in range(16) leaves at most {c.band} hidden units in the kink band"
    return B.register_problem(c, picked[1])


def round_trip32(pr, t):
    """max |g(f(x)) - x| of the float32 oracle: what the reversible reconstruction costs on these inputs."""
    import torch
    o = O.Fp32Gather(pr["s"], pr["r"], pr["n"], dtype=torch.float32, **pr["kw"])
    pt = o.prep_params(pr["p"])
    with torch.no_grad():
        x = o.to_t(pr["x"])
        z, _ = o.f(x, pt, t, pr["ws"])
        return float((o.g(z, pt, t, pr["ws"]) - x).abs().max())


def reference(c):
    """float64: z, loss, log-det and gradients from loss_and_grads; "dev": what the oracle's own float32 run differs by, per
    quantity (per gradient tensor) - the measure of what float32 costs on these inputs, and the other half of every bound."""
    if c in _REFS:
        return _REFS[c]
    import torch
    pr = problem(c)
    r64 = O.loss_and_grads(pr["s"], pr["r"], pr["n"], pr["x"], pr["p"], c.t, c.ws, **pr["kw"])
    r32 = O.loss_and_grads(pr["s"], pr["r"], pr["n"], pr["x"], pr["p"], c.t, c.ws, dtype=torch.float32, **pr["kw"])
    g64, g32 = B.flat_grads(r64["grads"]), B.flat_grads(r32["grads"])
    ref = dict(z=r64["z"], loss=r64["total_loss"], logdet=r64["log_det_jacobian"], grads=g64, moments={}, gz=None,
               kink=pick_seed(c)[2],
               dev=dict(z=float(np.abs(r32["z"] - r64["z"]).max()), loss=abs(r32["total_loss"] - r64["total_loss"]),
                        logdet=abs(r32["log_det_jacobian"] - r64["log_det_jacobian"]), gz=None, mean={}, var={},
                        grads={nm: float(np.abs(a.astype(np.float64) - b).max()) for (nm, a), (_, b) in zip(g32, g64)}))
    assert np.isfinite(ref["z"]).all() and np.abs(ref["z"]).max() < 50.0, "the oracle itself cannot take these inputs"
    _REFS[c] = ref
    return ref


def csr_pair(pr):
    """(rowptr, col) by receiver and by sender, as the library builds them (stable sorts of the edge list)."""
    from gnf_amd.graphs import build_csr_host
    return build_csr_host(pr["s"], pr["r"], pr["n"]), build_csr_host(pr["r"], pr["s"], pr["n"])


# ---- routes ---------------------------------------------------------------------------------------------------------------
# name: (net.fused, library options, trainer attributes)
ROUTES = {
    "default": (True, {}, {}),                                           # 1: stash as offered
    "recompute": (True, {}, {"stash_mlp_rows": False}),                  # 2: the recomputing tile kernel
    "layered": (False, {}, {}),                                          # 3: layered forward, generic backward
    "bwd_generic": (True, {"bwd_generic": 1}, {}),                       # 4: fused forward, generic backward
    "dw_grouped": (True, {"dw_grouped": 1}, {}),                         # 5: tile kernel without the merged launch
    "dw_grouped_serial": (True, {"dw_grouped": 1}, {"overlap_weight_grads": False}),   # 6: ... and no auxiliary stream
}
_RUNS = {}


def device_run(c, route):
    """GRevNetTrainer.loss_and_grads of the case on one route, twice on the same trainer; cached per (case, route)."""
    if (c, route) in _RUNS:
        return _RUNS[c, route]
    import ctypes as C
    import torch
    from gnf_amd import _abi
    from gnf_amd.factories import make_product_grevnet
    from gnf_amd.train import GRevNetTrainer
    from helpers import graph_from_arrays
    pr = problem(c)
    fused, options, attrs = ROUTES[route]
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = fused
    graph = graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)
    try:
        for k, v in options.items():
            _abi.set_option(k, v)
        tr = GRevNetTrainer(net)
        for k, v in attrs.items():
            setattr(tr, k, v)
        out = tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        got = dict(z=out["z_graph"].nodes.cpu().numpy(), loss=float(out["total_loss"]), logdet=float(out["log_det_jacobian"]),
                   moments={}, recon=out["reconstruction"].cpu().numpy(), grads=B.flat_grads(tr.named_gradients()),
                   flat=tr.grad.detach().cpu().clone(), stash=tr._mlp_stash is not None,
                   stash_bytes=int(_abi.lib().gnf_mlp_stash_bytes(pr["n"], c.d, C.byref(net._flow(c.d // 2, torch.device(DEV))))))
        tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        got["flat_again"] = tr.grad.detach().cpu().clone()
    finally:
        for k in options:
            _abi.set_option(k, 0)
    _RUNS[c, route] = got
    return got


# ---- the two tiers ----------------------------------------------------------------------------------------------------------
def needed_slack(err, dev, gmax):
    """err / dev, the figure SLACK is measured from.  A tensor the float32 oracle gets exactly (dev = 0: the one-node and
    no-edge cases have some) says nothing about SLACK while the device is within the 1e-6 gmax term of it."""
    if dev > 0.0:
        return err / dev
    return 0.0 if err <= 1e-6 * gmax else float("inf")


def compare_grads(rep, got_grads, want, ref, slack, label="grad"):
    """Every tensor of `got_grads` against `want` under both tiers; prints err / max|g| next to the float32 oracle's figure
    for every tensor and returns the largest needed_slack.
    project: 3e-4 max|g| + 1e-5 + 1e-6 gmax, widened to 4 x the float32 oracle's deviation (Report.add);
    tight:   slack x the float32 oracle's deviation of that tensor + 1e-6 gmax, never looser than the project tier."""
    gmax = max(float(np.abs(b).max()) for _, b in want)
    worst = 0.0
    for (nm, a), (_, b) in zip(got_grads, want):
        top, err, dev = float(np.abs(b).max()), float(np.abs(a - b).max()), ref["dev"]["grads"][nm]
        project = 3e-4 * top + 1e-5 + 1e-6 * gmax
        rep.add(label, nm, err, project, dev)
        tight = min(slack * dev + 1e-6 * gmax, max(project, 4.0 * dev))
        ratio = needed_slack(err, dev, gmax)
        worst = max(worst, ratio)
        scale = top if top > 0.0 else 1.0
        print(f"[bwd-routes] {rep.title} {nm}: err/max|g| {err / scale:.2e} float32-oracle {dev / scale:.2e} ratio {ratio:.2f}")
        if not err <= tight:
            rep.bad.append(f"{nm}: err {err:.3e} > tight bound {tight:.3e} ({slack:g} x float32 oracle's {dev:.3e} + 1e-6 x {gmax:.3e})")
    return worst


def check_grads(rep, got, ref, c, slack):
    """compare_grads against the float64 gradient; where a tensor misses and the reference has hidden units inside its kink
    band, once more against float64 autograd that takes, for THOSE units only, the side the device's gradient shows it took
    (batch_norm_routes.check_grads' fit).  Returns (largest needed slack, the float64 gradient the device was held to)."""
    assert [nm for nm, _ in got["grads"]] == [nm for nm, _ in ref["grads"]]
    units = ref["kink"]["units"]
    if units:
        trial = Report(rep.title)
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            compare_grads(trial, got["grads"], ref["grads"], ref, slack)
        if trial.bad:
            flips = B._kink_sides_taken(c, got, ref)
            print(f"[bwd-routes] {rep.title}: {len(units)} hidden units within {ref['kink']['tol']:.1e} of a kink, "
                  f"{len(flips)} on the other side on the device: {flips}; against the float64 sides: {trial.bad[0]}")
            want = B._grads_with_sides(c, ref, flips) if flips else ref["grads"]
            return compare_grads(rep, got["grads"], want, ref, slack), want
    return compare_grads(rep, got["grads"], ref["grads"], ref, slack), ref["grads"]
