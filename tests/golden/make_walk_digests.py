#!/usr/bin/env python3
"""Record the bits of the forward and inverse walk (gnf_grevnet_from_f32, gnf_grevnet_per_graph_f32,
gnf_grevnet_inverse_per_graph_f32), case by case, on the device.

    python tests/golden/make_walk_digests.py        # -> tests/golden/walk_digests.json

Public Python API only - factories.make_product_grevnet, GRevNet.f / g / f_per_graph / g_per_graph,
GRevNetTrainer.loss_and_grads, _abi.set_option and _abi.last_route - so the same file runs in a checkout of an older commit.
Unless a case says otherwise: D = 8, latent 32, K = 3, T = 2 on 40 nodes in complete graphs of 11, 13 and 16.  Every net keeps
its seeded initial weights with the last layer of each MLP scaled by 0.3 (as tools/backward_routes_dump.py); the node
features are 0.7 N(0, 1).  Per case and call the file holds the sha256 of every output's bytes (out, sums, graph_sums;
a training step: z, the reconstruction, the sums, the loss and every gradient tensor in order) and the names of the route
bits gnf_last_route reports after the call: a walk that changes kernel fails even where the bits agree.  An output that is
not finite is an error.  tests/test_walk_bits_gpu.py holds the library to the file.

The digests pin the toolchain's expf as much as the kernels: after a ROCm upgrade re-record them ON PURPOSE, from a build of
the commit named in the file (GNF_DIGESTS_COMMIT names it when the library comes from another checkout).
"""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "walk_digests.json")
DEV = "cuda:0"

MP = dict(D=8, latent=32, K=3, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
GEO = dict(MP, D=64, latent=256, K=5)   # the geometry k_half_fused_geo takes (tests/test_fused_geo_gpu.py)
DM = dict(MP, activation="relu", attn=dict(num_heads=2, kq_dim=3, v_dim=4, out_dim=6, concat=True, kq_dim_division=True,
                                           residual=False))
DM_LN = dict(DM, attn=dict(DM["attn"], layer_norm=True, residual=True))
SELF = dict(MP, activation="relu", attn=dict(scope="graph", kq_dim=3, v_dim=5))
MULTI = dict(MP, activation="relu", attn=dict(scope="graph", kq_dim=3, v_dim=5, num_heads=2, out_dim=6))
# the drivers' attention geometry, as tests/batch_norm_routes.py: at D = 64 the bijectors are applied on load, at D = 34 not
DM_BN = dict(MP, latent=32, K=2, epsilon=0.0, activation="relu", use_batch_norm=True,
             attn=dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80, concat=True, kq_dim_division=False, residual=False))
SMALL = [11, 13, 16]
ALL4 = ("f", "g", "f_per_graph", "g_per_graph")

# name, hyper-parameters, net.fused, library options, batch (graph sizes | ("rings", n): n nodes in rings of 64 | "empty"),
# calls ("train": one GRevNetTrainer.loss_and_grads; "g*" after "moving": after update_moving_statistics), padded nodes view
CASES = [
    ("mp_fused", MP, True, {}, SMALL, ("f", "g"), False),
    ("mp_layered", MP, False, {}, SMALL, ("f", "g"), False),
    ("mp_geo", GEO, True, {}, SMALL, ("f", "g"), False),
    ("mp_shared_T3", dict(MP, T=3, weight_sharing=True), True, {}, SMALL, ("f", "g"), False),
    ("mp_T1", dict(MP, T=1), True, {}, SMALL, ("f", "g"), False),
    ("mp_one_net_32", MP, True, dict(force_shape=21), SMALL, ("f", "g"), False),   # one net per workgroup + the coupling kernel
    ("mp_padded_view", MP, True, {}, SMALL, ("f", "g"), True),
    ("mp_bn_fused", dict(MP, use_batch_norm=True), True, {}, SMALL, ("f", "g", "f_per_graph", "moving", "g", "g_per_graph"), False),
    ("mp_bn_layered", dict(MP, use_batch_norm=True), False, {}, SMALL, ("f", "g", "f_per_graph", "moving", "g", "g_per_graph"), False),
    ("dm_bn_on_load", dict(DM_BN, D=64), True, {}, SMALL, ALL4, False),
    ("dm_bn_passes", dict(DM_BN, D=34), True, {}, SMALL, ALL4, False),
    ("dm_packed", DM, True, {}, SMALL, ("f", "g"), False),
    ("dm_attn_kernel", DM, True, dict(attn_kernel=1), SMALL, ("f", "g"), False),
    ("dm_layer_norm", DM_LN, True, {}, SMALL, ("f", "g"), False),
    ("self_attn", SELF, True, {}, SMALL, ("f", "g"), False),
    ("multihead_self_attn", MULTI, True, {}, SMALL, ("f", "g"), False),
    ("mp_n8192", dict(MP, D=4), True, {}, ("rings", 8192), ("f",), False),
    ("mp_n8193", dict(MP, D=4), True, {}, ("rings", 8193), ("f",), False),
    ("mp_bn_n16384", dict(MP, D=4, use_batch_norm=True), True, {}, ("rings", 16384), ("f",), False),
    ("mp_bn_n16385", dict(MP, D=4, use_batch_norm=True), True, {}, ("rings", 16385), ("f",), False),
    ("mp_bn_n16384_layered", dict(MP, D=4, use_batch_norm=True), False, {}, ("rings", 16384), ("f",), False),
    ("mp_bn_n16385_layered", dict(MP, D=4, use_batch_norm=True), False, {}, ("rings", 16385), ("f",), False),
    ("mp_split_tiles", dict(MP, D=4), True, {}, ("rings", 9216), ("f", "g"), False),   # 576 row tiles: 64 of them split on 256 CUs
    ("mp_big", dict(MP, D=4), True, {}, ("rings", 11392), ("f", "g"), False),           # 712 row tiles: too many on top to split
    ("train_mp", MP, True, {}, SMALL, ("train",), False),
    ("train_dm", DM, True, {}, SMALL, ("train",), False),
    ("train_self_attn", SELF, True, {}, SMALL, ("train",), False),
    ("empty", MP, True, {}, "empty", ALL4, False),
]
# the only case a parent that is not deterministic on it may lose (two workgroups share a split row tile)
MAY_BE_UNSTABLE = ("mp_split_tiles",)


def tamed(node):
    """a get_params() container with the last layer (W, b) of every MLP scaled by 0.3"""
    if isinstance(node, dict):
        return {k: tamed(v) if k in ("s", "t", "mlp") else v for k, v in node.items()}
    if node and isinstance(node[0], (tuple, list)) and len(node[0]) == 2 and hasattr(node[0][0], "shape"):   # an MLP: [(W, b), ...]
        return list(node[:-1]) + [(node[-1][0] * 0.3, node[-1][1] * 0.3)]
    return [tamed(v) for v in node]


def batch(spec, d, seed, padded=False):
    import numpy as np
    import torch
    from gnf_amd.datasets import senders_receivers
    from gnf_amd.graphs import GraphsTuple
    if spec == "empty":
        n_node, s, r, ne = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    elif spec[0] == "rings":     # rings of 64 nodes, both directions (a last graph of one node: its self loop)
        n = spec[1]
        n_node = np.asarray([64] * (n // 64) + ([n % 64] if n % 64 else []), np.int32)
        off = np.concatenate([[0], np.cumsum(n_node)[:-1]])
        s = np.concatenate([o + np.concatenate([np.arange(m), (np.arange(m) + 1) % m]) for o, m in zip(off, n_node)])
        r = np.concatenate([o + np.concatenate([(np.arange(m) + 1) % m, np.arange(m)]) for o, m in zip(off, n_node)])
        ne = 2 * n_node
    else:
        n_node = np.asarray(spec, np.int32)
        s, r, ne = senders_receivers(n_node)
    n = int(n_node.sum())
    x = torch.as_tensor((np.random.default_rng(seed).standard_normal((n, d)) * 0.7).astype(np.float32)).to(DEV)
    if padded:   # a view whose row stride is larger than D: the library copies first instead of running the first step out of place
        wide = torch.full((n, d + 3), float("nan"), dtype=torch.float32, device=DEV)
        wide[:, :d] = x
        x = wide[:, :d]
        assert x.stride(0) == d + 3
    return GraphsTuple(nodes=x, edges=torch.zeros(len(s), device=DEV), receivers=torch.as_tensor(np.asarray(r, np.int32)).to(DEV),
                       senders=torch.as_tensor(np.asarray(s, np.int32)).to(DEV), globals=torch.zeros(len(n_node), device=DEV),
                       n_node=torch.as_tensor(n_node).to(DEV), n_edge=torch.as_tensor(np.asarray(ne, np.int32)).to(DEV))


def _sha(what, *arrays):
    import numpy as np
    import torch
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        assert np.all(np.isfinite(a)), f"{what}: an output that is not finite - the case proves nothing"
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _leaves(tree):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k])
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from _leaves(v)
    else:
        yield tree


def run_case(name, hp, fused, opts, spec, calls, padded):
    """{"<case>/<call>": {"sha256": {output: digest}, "route": [names]}}"""
    import torch
    from gnf_amd import _abi, gnn
    from gnf_amd.factories import make_product_grevnet
    from gnf_amd.train import GRevNetTrainer
    out = {}
    gnn.set_random_seed(12345)
    net = make_product_grevnet(hp)
    net.fused = fused
    tr = GRevNetTrainer(net) if "train" in calls else None
    try:
        for k, v in opts.items():
            _abi.set_option(k, v)
        if tr is not None:
            tr.loss_and_grads(batch(SMALL, hp["D"], 3))     # builds the nets
        else:
            net.f(batch(SMALL, hp["D"], 3))
        net.set_params(tamed(net.get_params()))
        x, z = batch(spec, hp["D"], 3, padded), batch(spec, hp["D"], 4, padded)
        tag = ""
        for call in calls:
            key = f"{name}/{call}{tag}"
            if call == "moving":     # the moving statistics leave their initial values: the batch moments of the calls so far
                for half in net.bns:
                    for b in half:
                        b.update_moving_statistics()
                tag = "_moved"
                continue
            if call == "f":
                res, _ = net.f(x)
                got = dict(out=res.nodes, sums=net.last_sums)
            elif call == "g":
                got = dict(out=net.g(z).nodes)
            elif call == "f_per_graph":
                res, _ = net.f_per_graph(x)
                got = dict(out=res.nodes, sums=net.last_sums, graph_sums=net.last_graph_sums)
            elif call == "g_per_graph":
                res, _ = net.g_per_graph(z)
                got = dict(out=res.nodes, sums=net.last_sums, graph_sums=net.last_graph_sums)
            else:
                terms = tr.loss_and_grads(x)
                got = dict(out=terms["z_graph"].nodes, reconstruction=terms["reconstruction"], sums=terms["sums"],
                           loss=terms["total_loss"])
            torch.cuda.synchronize()
            route = sorted(_abi.last_route())
            digests = {k: _sha(f"{key} {k}", v) for k, v in got.items()}
            if call == "train":
                digests["gradients"] = _sha(f"{key} gradients", *_leaves(tr.named_gradients()))
            out[key] = dict(sha256=digests, route=route)
    finally:
        for k in opts:
            _abi.set_option(k, 0)
    return out


def measure(only=None):
    """every case's digests and routes from the library gnf_amd._abi loads"""
    from gnf_amd import _abi
    _abi.lib()
    out = {}
    for case in CASES:
        if only is None or case[0] in only:
            out.update(run_case(*case))
    return out


if __name__ == "__main__":
    commit = os.environ.get("GNF_DIGESTS_COMMIT")    # (set it when the library comes from another checkout's build)
    if not commit:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    out_path = sys.argv[1] if len(sys.argv) > 1 else OUT
    digests = measure()
    with open(out_path, "w") as f:
        json.dump({"commit": commit, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} calls of {len(CASES)} cases from commit {commit} -> {out_path} ({os.path.getsize(out_path)} B)")
