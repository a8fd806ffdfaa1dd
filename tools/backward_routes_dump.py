#!/usr/bin/env python
"""Bits of one training step on every route of the backward walk (gnf_grevnet_backward_f32), for comparing two builds of
the library: run it once per build and diff the two outputs.

    python tools/backward_routes_dump.py [--tensors] [case ...] > routes.txt

Public Python API only (no library hook), so the same file runs in a checkout of an older commit.  For a fixed list of
small seeded cases it prints the sha256 of z, of the reconstructed input, of the forward sums, the loss, and one sha256
over the bytes of every tensor of GRevNetTrainer.named_gradients() in order (--tensors: also one line per tensor, to find
which one differs), and next to each case the route the walk is presumed to take, worked out from the flags the case sets
(the library is not asked).  D = 8, latent 32, K = 3, T = 2 on 40 nodes in three graphs unless the case says otherwise.  The
nets keep their seeded initial weights with the last layer of every MLP scaled by 0.3 (as the suite's final_scale), so that
deep flows stay finite; a case whose loss or gradients are not finite is an error.  Every library option a case sets is
reset afterwards."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnf_amd import _abi, gnn  # noqa: E402
from gnf_amd.datasets import senders_receivers  # noqa: E402
from gnf_amd.factories import make_product_grevnet  # noqa: E402
from gnf_amd.graphs import GraphsTuple  # noqa: E402
from gnf_amd.train import GRevNetTrainer  # noqa: E402

DEV = "cuda:0"
MP = dict(D=8, latent=32, K=3, T=2, agg="mean", combine="agg", epsilon=1.0, activation="leaky_relu", weight_sharing=False)
DM = dict(MP, activation="relu", attn=dict(num_heads=2, kq_dim=3, v_dim=4, out_dim=6, concat=True, kq_dim_division=True,
                                           residual=False))
DM_LN = dict(DM, attn=dict(DM["attn"], layer_norm=True, residual=True))
SELF = dict(MP, activation="relu", attn=dict(scope="graph", kq_dim=3, v_dim=5))
MULTI = dict(MP, activation="relu", attn=dict(scope="graph", kq_dim=3, v_dim=5, num_heads=2, out_dim=6))
SMALL, BIG = [11, 13, 16], "big"  # BIG: 264 graphs of 9 .. 16 nodes, more than 192 tiles (tools/dw_modes_check.py big)
MID = "mid"                        # 150 such graphs: about 120 tiles - the merged launch with enough k-steps for stream-K
WIDE = dict(MP, D=48, latent=200)  # hidden layers of 2 x 2 wide-kernel tiles

# name, hyper-parameters, library options, trainer attributes, graph sizes ([]: the empty batch after a SMALL one)
CASES = [
    ("mp_stash", MP, {}, {}, SMALL),
    ("mp_recompute", MP, {}, dict(stash_mlp_rows=False), SMALL),
    ("mp_shared_T3", dict(MP, T=3, weight_sharing=True), {}, {}, SMALL),
    ("mp_batch_norm", dict(MP, use_batch_norm=True), {}, {}, SMALL),
    ("mp_grouped_stash", MP, dict(dw_grouped=1), {}, SMALL),
    ("mp_grouped_recompute", MP, dict(dw_grouped=1), dict(stash_mlp_rows=False), SMALL),
    ("mp_grouped_stash_serial", MP, dict(dw_grouped=1), dict(overlap_weight_grads=False), SMALL),
    ("mp_grouped_recompute_serial", MP, dict(dw_grouped=1), dict(stash_mlp_rows=False, overlap_weight_grads=False), SMALL),
    ("mp_grouped_T4", dict(MP, T=4), dict(dw_grouped=1), {}, SMALL),
    ("mp_generic", MP, dict(bwd_generic=1), {}, SMALL),
    ("dm_bn_stash", dict(DM, use_batch_norm=True), {}, {}, SMALL),
    ("dm_bn_recompute", dict(DM, use_batch_norm=True), {}, dict(stash_mlp_rows=False, stash_attention=False), SMALL),
    ("dm_bn_grouped", dict(DM, use_batch_norm=True), dict(dw_grouped=1), {}, SMALL),
    ("dm_layer_norm", DM_LN, {}, {}, SMALL),
    ("self_attn", SELF, {}, {}, SMALL),
    ("multihead_self_attn", MULTI, {}, {}, SMALL),
    ("layered_stash", dict(MP, D=24, latent=1280, activation="relu"), {}, {}, SMALL),
    ("mp_big", WIDE, {}, {}, BIG),
    # the wide weight-gradient kernel's shapes, forced: the summation order of a gradient is fixed by the launch plan (how
    # the node axis is cut, which slabs the reduce adds), so any change of a plan's cut shows in these
    *[(f"mp_units{u}", MP, dict(dw_wide_units=u), {}, SMALL) for u in (8, 13, 200)],
    ("mp_thin_on_dw", MP, dict(dw_thin_on_dw=1), {}, SMALL),
    ("mp_mid", WIDE, {}, {}, MID),
    *[(f"mp_mid_units{u}", WIDE, dict(dw_wide_units=u), {}, MID) for u in (8, 13, 200)],
    ("mp_mid_thin_on_dw", WIDE, dict(dw_thin_on_dw=1), {}, MID),
    ("mp_mid_recompute", WIDE, {}, dict(stash_mlp_rows=False), MID),
    *[(f"mp_big_units{u}", WIDE, dict(dw_wide_units=u), {}, BIG) for u in (8, 13, 200)],
    ("mp_big_thin_on_dw", WIDE, dict(dw_thin_on_dw=1), {}, BIG),
    ("mp_empty", MP, {}, {}, []),
]


def route(hp, opts, attrs, sizes):
    """the route the walk is PRESUMED to take, from the case's own flags and the library's documented thresholds (merged
    launch: up to 192 tiles and neither dw_grouped nor bwd_generic; fused kernels: hidden layers below 512) - a label for
    the reader, not something the library reported"""
    if sizes == []:
        return "empty batch (gradients zeroed)"
    stash = "MLP-row stash " + ("offered" if attrs.get("stash_mlp_rows", True) else "off")
    aux = "auxiliary stream " + ("offered" if attrs.get("overlap_weight_grads", True) else "off")
    if opts.get("bwd_generic"):
        return f"presumed streams / generic (bwd_generic=1), {aux}"
    if hp["latent"] >= 512:
        return f"presumed streams / generic (hidden width {hp['latent']}), {stash} (layered mode), {aux}"
    if opts.get("dw_grouped"):
        return f"presumed streams / fused (dw_grouped=1), {stash}, {aux}"
    if sizes == BIG:
        return f"presumed streams / fused (more than 192 tiles), {stash} (the library declines it above one tile per CU), {aux}"
    return f"presumed merged, {stash}"


def tamed(node):
    """a get_params() container with the last layer (W, b) of every MLP scaled by 0.3"""
    if isinstance(node, dict):
        return {k: tamed(v) if k in ("s", "t", "mlp") else v for k, v in node.items()}
    if node and isinstance(node[0], (tuple, list)) and len(node[0]) == 2 and hasattr(node[0][0], "shape"):   # an MLP: [(W, b), ...]
        return list(node[:-1]) + [(node[-1][0] * 0.3, node[-1][1] * 0.3)]
    return [tamed(v) for v in node]


def batch(sizes, d, seed):
    n_node = np.random.default_rng(5).integers(9, 17, size=264 if sizes == BIG else 150) if sizes in (BIG, MID) else np.asarray(sizes)
    n_node = n_node.astype(np.int32)
    s, r, ne = senders_receivers(n_node) if len(n_node) else (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    x = (np.random.default_rng(seed).standard_normal((int(n_node.sum()), d)) * 0.7).astype(np.float32)
    return GraphsTuple(nodes=torch.as_tensor(x).to(DEV), edges=torch.zeros(len(s), device=DEV),
                       receivers=torch.as_tensor(np.asarray(r, np.int32)).to(DEV),
                       senders=torch.as_tensor(np.asarray(s, np.int32)).to(DEV), globals=torch.zeros(len(n_node), device=DEV),
                       n_node=torch.as_tensor(n_node).to(DEV), n_edge=torch.as_tensor(np.asarray(ne, np.int32)).to(DEV))


def sha(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() + f"  {a.dtype}{list(a.shape)}"


def leaves(tree, path=""):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaves(tree[k], f"{path}.{k}" if path else str(k))
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaves(v, f"{path}[{i}]")
    else:
        yield path, tree


def run(name, hp, opts, attrs, sizes, per_tensor):
    print(f"== {name}: {route(hp, opts, attrs, sizes)}", flush=True)
    gnn.set_random_seed(12345)
    net = make_product_grevnet(hp)
    tr = GRevNetTrainer(net)
    for k, v in attrs.items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    try:
        for k, v in opts.items():
            _abi.set_option(k, v)
        tr.loss_and_grads(batch(SMALL, hp["D"], 3))       # builds the nets
        net.set_params(tamed(net.get_params()))
        steps = [SMALL, []] if sizes == [] else [sizes]   # (the empty batch: after one step that left non-zero gradients)
        for sz in steps:
            out = tr.loss_and_grads(batch(sz, hp["D"], 3))
            torch.cuda.synchronize()
    finally:
        for k in opts:
            _abi.set_option(k, 0)
    print(f"  nodes {int(out['z_graph'].nodes.shape[0])}  total_loss {float(out['total_loss']).hex()}")
    print(f"  z               {sha(out['z_graph'].nodes)}")
    print(f"  reconstruction  {sha(out['reconstruction'])}")
    print(f"  sums            {sha(out['sums'])}")
    zeros, every, count = True, hashlib.sha256(), 0
    for path, g in leaves(tr.named_gradients()):
        zeros = zeros and not np.any(np.asarray(g))
        every.update(np.ascontiguousarray(g).tobytes())
        count += 1
        if per_tensor:
            print(f"  grad {path:24s} {sha(g)}")
    finite = np.isfinite(float(out["total_loss"])) and all(np.all(np.isfinite(g)) for _, g in leaves(tr.named_gradients()))
    assert finite, f"{name}: non-finite loss or gradients - the case proves nothing"
    print(f"  gradients       {every.hexdigest()}  {count} tensors, all zero: {zeros}", flush=True)


if __name__ == "__main__":
    _abi.lib()
    names = [a for a in sys.argv[1:] if a != "--tensors"]
    for case in CASES:
        if not names or case[0] in names:
            run(*case, "--tensors" in sys.argv)
