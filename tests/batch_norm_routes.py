"""Shared by tests/test_batch_norm_routes_gpu.py: exact-size batches with ring + random edges, inputs with three hard
columns per half, the float64 / float32 oracle pair of one case (computed once, shared by every test of that case), one
device run of a case and the comparison.

Run as a program it is the child interpreter of the attention cases' attn_bwd_rows runs: the training step of every
attention case on both kernel paths, under whatever GNF_OPTIONS the parent set, saved to the .npz named on the command
line (python tests/batch_norm_routes.py OUT.npz); the parent compares the file with the references it already holds."""
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gnf_oracle as O  # noqa: E402

DEV = "cuda:0"
ATTN = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80, kq_dim_division=False, residual=False)   # run_grevnet.py:74-76

# kind: "mp" (avg_then_mlp, epsilon 1, leaky_relu) | "attn" (dm_self_attn with ATTN, relu); n: exact node count
Case = namedtuple("Case", "kind d n latent k t concat layer_norm")


def mp(d, n, latent=16, k=2, t=2):
    return Case("mp", d, n, latent, k, t, True, False)


def attn(d, n, latent=32, k=2, t=2, concat=True, layer_norm=False):
    return Case("attn", d, n, latent, k, t, concat, layer_norm)


def case_id(c):
    tag = f"D{c.d}_n{c.n}"
    if c.kind == "attn":
        tag = "attn_" + tag + ("" if c.concat else "_noconcat") + ("_ln" if c.layer_norm else "")
    return tag + (f"_T{c.t}" if c.t != 2 else "")


def graph_sizes(n, most=200):
    """n nodes as graphs of `most` nodes and one remainder: the node count is exact."""
    return [most] * (n // most) + ([n % most] if n % most else [])


def make_batch(sizes, rng):
    """Every graph a ring (both directions) plus about as many random undirected edges; two nodes: one edge pair; one node:
    a self loop.  Sparse by the library's rule (fewer than 24 edges per node), never empty."""
    s_l, r_l, ne, off = [], [], [], 0
    for m in sizes:
        pairs = set()
        if m == 1:
            pairs.add((0, 0))
        for i in range(m if m > 2 else m - 1):
            pairs.add((i, (i + 1) % m))
            pairs.add(((i + 1) % m, i))
        if m > 3:
            for u, v in zip(rng.integers(0, m, size=m), rng.integers(0, m, size=m)):
                if u != v:
                    pairs.add((int(u), int(v)))
                    pairs.add((int(v), int(u)))
        pairs = sorted(pairs)
        s_l.append(np.array([u for u, _ in pairs], np.int32) + off)
        r_l.append(np.array([v for _, v in pairs], np.int32) + off)
        ne.append(len(pairs))
        off += m
    return np.array(sizes, np.int32), np.array(ne, np.int32), np.concatenate(s_l), np.concatenate(r_l)


def hard_nodes(rng, n, d):
    """N(0, 1) with, in each half of at least three columns: 100 + 0.1 N(0, 1) (a float32 column sum is off by percent of
    the variance), a constant 0.75 (variance exactly zero: the clamp) and 1e-3 N(0, 1) (variance far below epsilon)."""
    x = rng.standard_normal((n, d))
    h = d // 2
    if h >= 3:
        for c0 in (0, h):
            x[:, c0] = 100.0 + 0.1 * x[:, c0]
            x[:, c0 + 1] = 0.75
            x[:, c0 + 2] *= 1e-3
    return x.astype(np.float32)


_PROBLEMS, _REFS = {}, {}


def problem(c):
    if c in _PROBLEMS:
        return _PROBLEMS[c]
    seed = zlib.crc32(repr(tuple(c)).encode())
    rng = np.random.default_rng(seed)
    nn, ne, s, r = make_batch(graph_sizes(c.n, 200 if c.kind == "mp" else 60), rng)
    h = c.d // 2
    if c.kind == "mp":
        hp = dict(D=c.d, latent=c.latent, K=c.k, T=c.t, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu",
                  weight_sharing=False)
        p = O.make_grevnet_params(seed % 9973, h, c.latent, c.k, c.t, final_scale=0.05)
        kw = dict(agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu")
    else:
        a = dict(ATTN, concat=c.concat, layer_norm=c.layer_norm)
        hp = dict(D=c.d, latent=c.latent, K=c.k, T=c.t, agg="mean", combine="agg", epsilon=0.0, activation="relu",
                  weight_sharing=False, attn=a)
        p = O.make_attn_grevnet_params(seed % 9973, h, c.latent, c.k, c.t, final_scale=0.05, **a)
        kw = dict(activation="relu")
    p["bn"] = O.make_bn_params(seed % 9973 + 1, h, c.t)
    pr = dict(nn=nn, ne=ne, s=s, r=r, n=c.n, x=hard_nodes(rng, c.n, c.d),
              zs=rng.standard_normal((c.n, c.d)).astype(np.float32), hp=hp, p=p, kw=kw)
    _PROBLEMS[c] = pr
    return pr


def register_problem(c, pr):
    """A case of another family (tests/backward_routes.py) with the problem its own module built: any hashable `c` with .t,
    `pr` with the keys of problem()'s result (+ "ws": weight sharing, False where absent).  _gather_run, _grads_with_sides
    and check_grads then work on it as on this module's cases."""
    _PROBLEMS[c] = pr
    return pr


def flat_grads(g):
    """(name, array) of every tensor of a gradient container, bijectors last; the same order for the same layout.  With
    weight sharing a half holds one net (its list of (W, b)) instead of a list of T nets: named as net 0 of that half."""
    out = []
    for kind in ("s", "t"):
        for half, nets in enumerate(g[kind]):
            if nets and isinstance(nets[0], tuple) and hasattr(nets[0][0], "shape"):
                nets = [nets]
            for i, net in enumerate(nets):
                mlp = net["mlp"] if isinstance(net, dict) else net
                if isinstance(net, dict):
                    for key in sorted(net["attn"]):
                        out.append((f"{kind}[{half}][{i}].{key}", net["attn"][key]))
                for j, (w, b) in enumerate(mlp):
                    out.append((f"{kind}[{half}][{i}].W{j}", w))
                    out.append((f"{kind}[{half}][{i}].b{j}", b))
    for half, bns in enumerate(g.get("bn", [])):
        for i, bn in enumerate(bns):
            out.append((f"bn[{half}][{i}].gamma", bn["gamma"]))
            out.append((f"bn[{half}][{i}].beta", bn["beta"]))
    return out


def _gather_run(pr, t, dtype, inverse=True):
    """The gather oracle (the op graph loss_and_grads differentiates) in `dtype`: every bijector's batch moments, the hidden
    pre-activations of every MLP evaluation of f ({(call, layer): [n, L]}, call numbered as Fp32Gather._act_kink numbers
    them), g(zs)."""
    import torch

    class Recording(O.Fp32Gather):
        def bn_inverse(self, x, bn):
            mean = x.mean(dim=0)
            self.moments.append((mean.numpy().astype(np.float64), ((x - mean) ** 2).mean(dim=0).numpy().astype(np.float64)))
            return super().bn_inverse(x, bn)

        def mlp(self, h, layers):
            if self.pre is not None:
                call, a = getattr(self, "_mlp_calls", -1) + 1, h
                for j, (w, b) in enumerate(layers[:-1]):
                    a = a @ w + b
                    self.pre[call, j] = a.numpy().astype(np.float64)
                    a = self.act(a)
            return super().mlp(h, layers)

    o = Recording(pr["s"], pr["r"], pr["n"], dtype=dtype, **pr["kw"])
    o.moments, o.pre = [], {}
    pt, ws = o.prep_params(pr["p"]), pr.get("ws", False)
    with torch.no_grad():
        o.f(o.to_t(pr["x"]), pt, t, ws)
        pre, o.pre = o.pre, None
        gz = o.g(o.to_t(pr["zs"]), pt, t, ws).numpy().astype(np.float64) if inverse else None
    moments = {(q % 2, q // 2): mv for q, mv in enumerate(o.moments)}      # f visits (0, i) then (1, i)
    return moments, gz, pre


def reference(c):
    """float64: z, loss, log-det and gradients from loss_and_grads; moments and g(zs) from Fp64Dense (its dense adjacency
    is n^2 doubles: batches of more than 4096 nodes take both from the float64 gather oracle instead).  "dev": what the
    oracle's own float32 run differs by, per quantity - the other half of every bound.  g(zs) is left out (None) of flows
    of more than two steps: twenty-five de-normalisations with unrelated moving statistics overflow in any precision."""
    if c in _REFS:
        return _REFS[c]
    import torch
    pr = problem(c)
    r64 = O.loss_and_grads(pr["s"], pr["r"], pr["n"], pr["x"], pr["p"], c.t, **pr["kw"])
    r32 = O.loss_and_grads(pr["s"], pr["r"], pr["n"], pr["x"], pr["p"], c.t, dtype=torch.float32, **pr["kw"])
    inv = c.t <= 2
    if c.n <= 4096:
        dense = O.Fp64Dense(pr["s"], pr["r"], pr["n"], **pr["kw"])
        dense.f(pr["x"], pr["p"], c.t)
        moments, gz = dict(dense.last_bn_moments), dense.g(pr["zs"], pr["p"], c.t) if inv else None
        _, _, pre64 = _gather_run(pr, c.t, torch.float64, False)
    else:
        moments, gz, pre64 = _gather_run(pr, c.t, torch.float64, inv)
    m32, gz32, pre32 = _gather_run(pr, c.t, torch.float32, inv)
    # relu / leaky-relu kinks: a hidden unit whose pre-activation lies within `tol` of zero has no side that float32 and
    # float64 agree on (tol: the band of tests/test_fullsize_gpu.py, 2e-5, or 4 x what the float32 oracle's
    # pre-activations differ from the float64 ones by on these inputs, whichever is larger) - see check_grads
    tol = max([2e-5] + [4.0 * float(np.abs(pre32[k] - pre64[k]).max()) for k in pre64])
    units = [(k, int(v), int(u)) for k in sorted(pre64) for v, u in zip(*np.nonzero(np.abs(pre64[k]) < tol))]
    kink = dict(tol=tol, units=units, sides={k: pre64[k] > 0 for k in {k for k, _, _ in units}})
    g64, g32 = flat_grads(r64["grads"]), flat_grads(r32["grads"])
    ref = dict(z=r64["z"], loss=r64["total_loss"], logdet=r64["log_det_jacobian"], grads=g64, moments=moments, gz=gz,
               kink=kink,
               dev=dict(z=float(np.abs(r32["z"] - r64["z"]).max()), loss=abs(r32["total_loss"] - r64["total_loss"]),
                        logdet=abs(r32["log_det_jacobian"] - r64["log_det_jacobian"]), gz=float(np.abs(gz32 - gz).max()) if inv else None,
                        grads={nm: float(np.abs(a.astype(np.float64) - b).max()) for (nm, a), (_, b) in zip(g32, g64)},
                        # batch moments: each bijector's own deviation (the variance scaled as check_forward_terms scales the
                        # device's error) - below n = 15, where the issue already finds float32 figures too noisy to compare
                        # gradients, the largest over the case's bijectors: there one bijector's figure is a sample of one
                        # or two roundings of the same arithmetic on columns of the same kind
                        mean={k: float(np.abs(m32[k][0] - moments[k][0]).max()) for k in moments},
                        var={k: float((np.abs(m32[k][1] - moments[k][1]) / (1.0 + np.abs(moments[k][1]))).max()) for k in moments}))
    if c.n < 15:
        for q in ("mean", "var"):
            ref["dev"][q] = dict.fromkeys(moments, max(ref["dev"][q].values()))
    # (a block that ends in snt.LayerNorm has |s| up to ~2 per feature whatever the inputs: its z is finite, not small)
    assert np.isfinite(ref["z"]).all() and (c.layer_norm or np.abs(ref["z"]).max() < 10.0), "the oracle itself cannot take these inputs"
    _REFS[c] = ref
    return ref


def _device_moments(net, t):
    return {(half, i): (net.bns[half][i].batch_mean.cpu().numpy().copy(), net.bns[half][i].batch_variance.cpu().numpy().copy())
            for half in range(2) for i in range(t)}


def make_net(c, fused):
    from gnf_amd.factories import make_product_grevnet
    pr = problem(c)
    net = make_product_grevnet(pr["hp"], pr["p"])
    net.fused = fused
    return net


def device_graph(c):
    from helpers import graph_from_arrays
    pr = problem(c)
    return graph_from_arrays(pr["nn"], pr["ne"], pr["s"], pr["r"], pr["x"], DEV)


def run_forward(c, fused):
    """log_prob_terms (the plain forward: no stash), every bijector's batch moments, then g(zs)."""
    import torch
    from gnf_amd.flow import log_prob_terms
    net, graph = make_net(c, fused), device_graph(c)
    out = log_prob_terms(net, graph)
    torch.cuda.synchronize()
    res = dict(z=out["z_graph"].nodes.cpu().numpy(), loss=float(out["total_loss"]), logdet=float(out["log_det_jacobian"]),
               moments=_device_moments(net, c.t))
    zs = graph.replace(nodes=torch.as_tensor(problem(c)["zs"]).to(DEV))
    res["gz"] = net(zs, inverse=False).nodes.cpu().numpy()
    return res


def run_training(c, fused):
    """GRevNetTrainer.loss_and_grads (the training forward, which may stash and so take other kernels, + the backward walk):
    z, loss, moments again, the reversible reconstruction, every gradient."""
    import torch
    from gnf_amd.train import GRevNetTrainer
    net, graph = make_net(c, fused), device_graph(c)
    tr = GRevNetTrainer(net)
    out = tr.loss_and_grads(graph)
    torch.cuda.synchronize()
    return dict(z=out["z_graph"].nodes.cpu().numpy(), loss=float(out["total_loss"]), logdet=float(out["log_det_jacobian"]),
                moments=_device_moments(net, c.t), recon=out["reconstruction"].cpu().numpy(),
                grads=flat_grads(tr.named_gradients()))


class Report:
    """Every figure is printed before anything is asserted: `pytest -s` shows err / bound (float32-oracle deviation)."""

    def __init__(self, title):
        self.title, self.bad, self.worst = title, [], {}

    def add(self, family, name, err, project, dev):
        bound = max(project, 4.0 * dev)
        w = self.worst.get(family)
        if w is None or err / bound > w[1] / w[2]:
            self.worst[family] = (name, err, bound, dev)
        if not err <= bound:      # (NaN fails)
            self.bad.append(f"{name}: err {err:.3e} > {bound:.3e} (project bound {project:.3e}, float32 oracle off by {dev:.3e})")

    def finish(self):
        for fam, (name, err, bound, dev) in self.worst.items():
            print(f"[bn-routes] {self.title} {fam}: worst {name} err {err:.3e} bound {bound:.3e} f32-oracle {dev:.3e}")
        assert not self.bad, self.title + "\n" + "\n".join(self.bad)


def check_forward_terms(rep, got, ref, n, tag=""):
    """z: 5e-4 max(1, |ref|max); loss and log-det: 1e-4 per node; batch mean: 3e-5; batch variance: 3e-5 + 3e-5 |ref|, and
    never negative - each widened to 4 x the float32 oracle's own deviation where that is larger."""
    dev = ref["dev"]
    rep.add("z", tag + "z", float(np.abs(got["z"] - ref["z"]).max()), 5e-4 * max(1.0, float(np.abs(ref["z"]).max())), dev["z"])
    rep.add("loss", tag + "total_loss", abs(got["loss"] - ref["loss"]), 1e-4 * n, dev["loss"])
    rep.add("loss", tag + "log_det_jacobian", abs(got["logdet"] - ref["logdet"]), 1e-4 * n, dev["logdet"])
    for key, (m, v) in ref["moments"].items():
        gm, gv = got["moments"][key]
        rep.add("mean", f"{tag}batch_mean{key}", float(np.abs(gm - m).max()), 3e-5, dev["mean"][key])
        rep.add("var", f"{tag}batch_variance{key}", float((np.abs(gv - v) / (1.0 + np.abs(v))).max()), 3e-5, dev["var"][key])
        if not (gv >= 0.0).all():
            rep.bad.append(f"{tag}batch_variance{key}: negative entries {gv[gv < 0.0]}")


def check_inverse(rep, got, ref):
    rep.add("g(zs)", "g(zs)", float(np.abs(got["gz"] - ref["gz"]).max()), 5e-4 * max(1.0, float(np.abs(ref["gz"]).max())),
            ref["dev"]["gz"])


def check_reconstruction(rep, got, x):
    """The reversible walk rebuilds its input: the project's atol = rtol = 3e-4."""
    rep.add("recon", "reconstruction", float((np.abs(got["recon"] - x) / (1.0 + np.abs(x))).max()), 3e-4, 0.0)


def _grads_with_sides(c, ref, flips):
    """float64 autograd with the other side of the relu for the hidden units in `flips` (all inside the band; every unit
    outside it keeps the oracle's own side: Fp32Gather._act_kink)."""
    pr, k = problem(c), ref["kink"]
    masks = {key: m.copy() for key, m in k["sides"].items()}
    for key, v, u in flips:
        masks[key][v, u] = not masks[key][v, u]
    state = {"masks": masks, "tol": k["tol"]}
    out = flat_grads(O.loss_and_grads(pr["s"], pr["r"], pr["n"], pr["x"], pr["p"], c.t, pr.get("ws", False), kink=state,
                                      **pr["kw"])["grads"])
    assert state.get("outside", 0) == 0, state
    return out


def _kink_sides_taken(c, got, ref):
    """Which of the units inside the band took the other side on the device?  To first order every such unit adds its own
    term to the gradient: a least-squares fit of the device's difference from the float64 gradient over those terms
    (one autograd run each), rounded to taken / not taken."""
    units, g0 = ref["kink"]["units"], np.concatenate([b.ravel() for _, b in ref["grads"]])
    terms = np.stack([np.concatenate([b.ravel() for _, b in _grads_with_sides(c, ref, [a])]) - g0 for a in units], axis=1)
    theta = np.linalg.lstsq(terms, np.concatenate([a.ravel() for _, a in got["grads"]]).astype(np.float64) - g0, rcond=None)[0]
    # a unit took one side or the other: a fit that lands in between explains something else and may not choose sides
    assert all(min(abs(th), abs(th - 1.0)) <= 0.25 for th in theta), ("kink fit is not a set of sides", list(zip(units, theta)))
    return [a for a, th in zip(units, theta) if th > 0.5]


def check_grads(rep, got, ref, c):
    """_check_grads' 3e-4 max|g| + 1e-5 + 1e-6 gmax per weight tensor, 3e-4 max|g| + 1e-4 for a bijector's gamma / beta,
    each widened to 4 x the float32 oracle's own deviation where that is larger.
    Where a tensor misses and the reference has hidden units inside its kink band (reference()), the gradient is compared
    once more with float64 autograd that takes, for THOSE units only, the side the device's gradient shows it took (the
    project's kink-aware pin, tests/test_fullsize_gpu.py, with the sides fitted instead of read from a stash): a relu has no
    derivative at zero and float32 puts such a unit on either side; the bounds stay what they are."""
    assert [nm for nm, _ in got["grads"]] == [nm for nm, _ in ref["grads"]]

    def compare(rp, want):
        gmax = max(float(np.abs(b).max()) for nm, b in want if not nm.startswith("bn"))
        for (nm, a), (_, b) in zip(got["grads"], want):
            top = float(np.abs(b).max())
            project = 3e-4 * top + 1e-4 if nm.startswith("bn") else 3e-4 * top + 1e-5 + 1e-6 * gmax
            rp.add("bn-grad" if nm.startswith("bn") else "grad", nm, float(np.abs(a - b).max()), project, ref["dev"]["grads"][nm])

    units = ref["kink"]["units"]
    if units and len(units) <= 256:
        trial = Report(rep.title)
        compare(trial, ref["grads"])
        if trial.bad:
            flips = _kink_sides_taken(c, got, ref)
            print(f"[bn-routes] {rep.title}: {len(units)} hidden units within {ref['kink']['tol']:.1e} of a kink, "
                  f"{len(flips)} on the other side on the device: {flips}; against the float64 sides: {trial.bad[0]}")
            compare(rep, _grads_with_sides(c, ref, flips) if flips else ref["grads"])
            return
    compare(rep, ref["grads"])


# ---- the attention cases (shared with the child interpreter) ------------------------------------------------------------
ATTN_CASES = [attn(d, n) for d in (2, 34, 64) for n in (17, 513, 528)] + [
    attn(2, 528, concat=False), attn(34, 513, concat=False),      # no concat: the widths the on-load instance needs at odd H
    attn(66, 513), attn(64, 513, layer_norm=True)]                # refused by fused_bn_on_load_ok / front_fold_ok


def _child(path):
    out = {}
    for c in ATTN_CASES:
        for fused in (True, False):
            got = run_training(c, fused)
            key = f"{case_id(c)}|{int(fused)}|"
            out[key + "z"], out[key + "recon"] = got["z"], got["recon"]
            out[key + "scalars"] = np.array([got["loss"], got["logdet"]], np.float64)
            for nm, a in got["grads"]:
                out[key + "g|" + nm] = a
            for (half, i), (m, v) in got["moments"].items():
                out[key + f"m|{half}|{i}"] = np.stack([m, v])
    np.savez(path, **out)
    print("bn-routes-child-ok")


def load_child(path, c, fused):
    d = np.load(path)
    key = f"{case_id(c)}|{int(fused)}|"
    names = [nm for nm, _ in reference(c)["grads"]]
    return dict(z=d[key + "z"], recon=d[key + "recon"], loss=float(d[key + "scalars"][0]), logdet=float(d[key + "scalars"][1]),
                grads=[(nm, d[key + "g|" + nm]) for nm in names],
                moments={(half, i): tuple(d[key + f"m|{half}|{i}"]) for half in range(2) for i in range(c.t)})


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[1])
