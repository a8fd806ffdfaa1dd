"""Graph-scope attention (GnfAttn.scope == GNF_ATTN_GRAPH) at the places where a windowed flash attention goes wrong, against
the float64 oracle (tests/graph_attn_ref.py, its per-graph form) at test_graph_attn_gpu.py's tolerances and checks.

The kernel instance is chosen from the head widths (launch_attn_graph_front / launch_attn_graph_backward):
  I1  kq, v <= 16  <1,1,8>    128 keys per window chunk
  I4  kq, v <= 64  <4,4,8>    128
  I16 otherwise    <16,16,4>   64
Every instance meets every batch layout forward and in training gradients: empty graphs (leading, interior, trailing), graph
boundaries on and next to a 64-row tile boundary, graphs of CH - 1 .. 2 CH + 1 nodes with a tile whose window spans two graphs
larger than CH, one graph of more than 1000 nodes.  Then: batches of one-node graphs (no softmax at all), a softmax whose
maximum arrives in a late chunk far above the earlier ones (the cross-chunk rescale, the backward's use of the forward's m
and Z), kq_dim_division=False, H > 256 (the dL/dx kernel's second column stripe), both backward walks, whole-graph shards,
and tools/fuzz_parity.py --graph."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import graph_attn_ref as R
from helpers import graph_from_arrays
from test_graph_attn_gpu import _batch, _check_flow, _flat_all, _net, _train_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (geometry, keys per window chunk of its instance)
GEOMS = {
    "I1_8x10_wo": (dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80), 128),       # run_grevnet.py's defaults
    "I1_64x4_wo": (dict(num_heads=64, kq_dim=4, v_dim=4, out_dim=32), 128),
    "I4_1x64": (dict(num_heads=1, kq_dim=64, v_dim=64), 128),                        # SelfAttention: no Wo
    "I4_3x24_20_wo": (dict(num_heads=3, kq_dim=24, v_dim=20, out_dim=24), 128),     # float4 staging
    "I4_2x33_17_wo": (dict(num_heads=2, kq_dim=33, v_dim=17, out_dim=16), 128),     # scalar staging
    "I16_1x256": (dict(num_heads=1, kq_dim=256, v_dim=256), 64),
    "I16_2x128_17_wo": (dict(num_heads=2, kq_dim=128, v_dim=17, out_dim=24), 64),
    "I16_3x80_72_wo_ln": (dict(num_heads=3, kq_dim=80, v_dim=72, out_dim=32, layer_norm=True), 64),
}


def layout(name, ch):
    if name == "empties":              # zero-node graphs leading, interior (two in a row) and trailing
        return [0, 5, 0, 0, 70, 1, 0]
    if name == "tile_edges":           # boundaries at 64, 128 (on), 129, 192 (on), 257 (one after), 384 (on); N % 64 == 1
        return [64, 64, 1, 63, 65, 127, 129]
    if name == "tile_edges_aligned":   # ... N % 64 == 0
        return [64, 64, 1, 63, 65, 127, 128]
    if name == "chunk_edges":          # rows CH - 1 .. CH + 1 of the first two graphs share a tile: its window is both
        return [ch + 1, 2 * ch + 1, ch - 1, ch]
    assert name == "big"
    return [1030]


def _problem(geom_name, lay, seed, d=8, kq_dim_division=True, t=2, latent=32, k=2, final_scale=0.5):
    geom, ch = GEOMS[geom_name]
    rng = np.random.default_rng(seed)
    p = R.make_graph_attn_grevnet_params(seed + 1, d // 2, latent, k, t, final_scale=final_scale,
                                         kq_dim_division=kq_dim_division, **geom)
    nn, ne, s, r = _batch(layout(lay, ch), rng)
    x = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    return p, nn, ne, s, r, x


FWD_LAYOUTS = ["empties", "tile_edges", "tile_edges_aligned", "chunk_edges"]
FWD_CASES = [(g, lay) for g in GEOMS for lay in FWD_LAYOUTS] + [("I4_3x24_20_wo", "big"), ("I16_2x128_17_wo", "big")]


@pytest.mark.parametrize("geom,lay", FWD_CASES, ids=[f"{g}-{lay}" for g, lay in FWD_CASES])
def test_forward_inverse_log_prob(geom, lay):
    """z, log-prob, g(f(x)) and g(zs) of a T = 2 flow; every tile_edges_aligned case runs with kq_dim_division=False"""
    div = lay != "tile_edges_aligned"
    d, t = 8, 2
    p, nn, ne, s, r, x = _problem(geom, lay, 100 + FWD_CASES.index((geom, lay)), d, div, t)
    _check_flow(_net(p, d, 32, 2, t), nn, ne, s, r, x, p, t, per_graph=True)


# (geometry, layout, kq_dim_division): every instance meets every layout once
GRAD_CASES = [
    ("I1_8x10_wo", "empties", True),
    ("I1_64x4_wo", "tile_edges", True),
    ("I1_8x10_wo", "chunk_edges", False),
    ("I4_3x24_20_wo", "empties", True),
    ("I4_2x33_17_wo", "tile_edges_aligned", False),
    ("I4_1x64", "chunk_edges", True),
    ("I4_3x24_20_wo", "big", True),
    ("I16_3x80_72_wo_ln", "empties", True),
    ("I16_1x256", "tile_edges", False),
    ("I16_2x128_17_wo", "chunk_edges", True),
    ("I16_2x128_17_wo", "big", True),
]


@pytest.mark.parametrize("geom,lay,div", GRAD_CASES, ids=[f"{g}-{lay}-{'div' if v else 'nodiv'}" for g, lay, v in GRAD_CASES])
def test_training_gradients(geom, lay, div):
    d, latent, k, t = 8, 64, 2, 2
    p, nn, ne, s, r, x = _problem(geom, lay, 200 + GRAD_CASES.index((geom, lay, div)), d, div, t, latent, k, 0.25)
    _train_check(p, nn, ne, s, r, (x * 0.8).astype(np.float32), d, latent, k, t, per_graph=True)


# ---- one-node graphs: every row of a tile in a graph of its own ----------------------------------------------------------
SINGLETON_GEOMS = ["I1_8x10_wo", "I4_1x64", "I16_2x128_17_wo"]


def _block(geom, h, latent=32, k=2, seed=0, kq_dim_division=True):
    """one graph-scope block (the module and its parameters), as test_graph_attn_gpu.test_block_alone builds it"""
    from gnf_amd import gnn
    g = dict(geom)
    g["kq_dim_division"] = kq_dim_division
    net = R.make_graph_attn_net_params(np.random.default_rng(seed), h, latent, k, **g)
    mk = lambda: gnn.make_mlp_model(latent, h, k)   # noqa: E731
    if "out_dim" in g:
        blk = gnn.multihead_self_attn_gnn(g["kq_dim"], g["v_dim"], g["out_dim"], mk, num_heads=g["num_heads"],
                                          kq_dim_division=kq_dim_division, layer_norm=g.get("layer_norm", False))
    else:
        blk = gnn.self_attn_gnn(g["kq_dim"], g["v_dim"], mk, kq_dim_division)
    return blk, net


def _block_run(blk, net, nn, ne, s, r, x):
    blk.set_attn_params(net["attn"])
    blk._mlp.set_params(net["mlp"])
    out = blk(graph_from_arrays(nn, ne, s, r, x, DEV)).nodes.cpu().numpy()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("geom", SINGLETON_GEOMS)
def test_singletons(geom):
    """~130 one-node graphs: the block is mlp([x || (x Wv) Wo]) with no softmax, the flow matches the oracle, and wq / wk
    get no gradient (a softmax over one key has none)"""
    rng = np.random.default_rng(7)
    h = 5
    nn, ne, s, r = _batch([1] * 131, rng)
    x = rng.standard_normal((131, h)).astype(np.float32)
    blk, net = _block(GEOMS[geom][0], h, seed=3)
    out = _block_run(blk, net, nn, ne, s, r, x)
    o = R.GraphAttnGather(s, r, nn, activation="relu")
    o.attended = lambda xx, a: xx @ a["wv"]                        # no softmax at all
    want = o.attn_gnn(o.to_t(x), o.prep_params({"n": [net]})["n"][0]).numpy()
    np.testing.assert_allclose(out, want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=1e-4)
    d, latent, k, t = 8, 64, 2, 2
    p = R.make_graph_attn_grevnet_params(9, d // 2, latent, k, t, final_scale=0.5, **GEOMS[geom][0])
    x = rng.standard_normal((131, d)).astype(np.float32)
    _check_flow(_net(p, d, latent, k, t), nn, ne, s, r, x, p, t, per_graph=True)
    tr, _ = _train_check(p, nn, ne, s, r, x, d, latent, k, t, per_graph=True)
    grads = _flat_all(tr.named_gradients())
    gmax = max(float(np.abs(g).max()) for _, g in grads)
    logit_side = [(name, g) for name, g in grads if name.endswith(".attn.wq") or name.endswith(".attn.wk")]
    assert len(logit_side) == 2 * 2 * t * 2
    for name, g in logit_side:
        assert float(np.abs(g).max()) <= 1e-6 * gmax, f"{name}: {np.abs(g).max():.3e} vs max gradient {gmax:.3e}"


# ---- a softmax maximum that arrives in a late chunk ----------------------------------------------------------------------
ADV_GEOMS = ["I1_8x10_wo", "I4_3x24_20_wo", "I16_2x128_17_wo"]
ADV_SIZES = [300, 40, 9]   # the 300-node graph first: every tile over it has its window from row 0, chunks at multiples of CH
ADV_NODE = 270             # in chunk 4 (CH = 64) / chunk 2 (CH = 128): keys 256 ..
GAMMA = 20.0               # the logit of feature 0 alone: GAMMA x_i0 x_j0


def _make_adversarial(attn, x_nodes, col, kq_dim_division):
    """Feature `col` drives every head's logit with weight GAMMA (wq, wk rows `col` set to beta, the same in every column),
    ADV_NODE's feature is 8 where every other node's is ~N(0, 1): rows with x_i0 > 0 see that key far above every key before
    its chunk, rows with x_i0 < 0 far below everything (its weight underflows)."""
    kq = int(attn["kq_dim"])
    beta = math.sqrt(GAMMA / (math.sqrt(kq) if kq_dim_division else kq))
    for w in ("wq", "wk"):
        attn[w] = np.array(attn[w], np.float32)
        attn[w][col] = beta
    x_nodes[ADV_NODE, col] = 8.0


def _adversarial_logits_hold(attn, x, col, ch, kq_dim_division):
    """the construction does what it says on this batch: in many (row, head) pairs of the big graph the late key's logit is
    >= 20 above every key of the earlier chunks, in many others its weight is below float32's smallest (e^-104)"""
    nh, kq = int(attn["num_heads"]), int(attn["kq_dim"])
    xs = np.asarray(x, np.float64)[:ADV_SIZES[0], :attn["wq"].shape[0]]
    q = (xs @ np.asarray(attn["wq"], np.float64)).reshape(-1, nh, kq)
    k = (xs @ np.asarray(attn["wk"], np.float64)).reshape(-1, nh, kq)
    lg = np.einsum("ihd,jhd->hij", q, k) / (math.sqrt(kq) if kq_dim_division else 1.0)
    e0 = ch * (ADV_NODE // ch)
    assert e0 >= 2 * ch
    above = lg[:, :, ADV_NODE] - lg[:, :, :e0].max(-1)
    below = lg[:, :, ADV_NODE] - lg.max(-1)
    assert (above >= 20).mean() >= 0.3 and (below <= -104).mean() >= 0.2, ((above >= 20).mean(), (below <= -104).mean())


@pytest.mark.parametrize("div", [True, False], ids=["div", "nodiv"])
@pytest.mark.parametrize("geom", ADV_GEOMS)
def test_adversarial_softmax_block(geom, div):
    """the block alone (gnf_gnn_apply_f32) against float64: the online softmax rescales the earlier chunks' sums"""
    rng = np.random.default_rng(21)
    h = 6
    nn, ne, s, r = _batch(ADV_SIZES, rng)
    x = rng.standard_normal((int(nn.sum()), h)).astype(np.float32)
    blk, net = _block(GEOMS[geom][0], h, seed=4, kq_dim_division=div)
    _make_adversarial(net["attn"], x, 0, div)
    _adversarial_logits_hold(net["attn"], x, 0, GEOMS[geom][1], div)
    out = _block_run(blk, net, nn, ne, s, r, x)
    o = R.GraphAttnGather(s, r, nn, activation="relu", per_graph=True)
    want = o.attn_gnn(o.to_t(x), o.prep_params({"n": [net]})["n"][0]).numpy()
    np.testing.assert_allclose(out, want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=1e-4)


@pytest.mark.parametrize("div", [True, False], ids=["div", "nodiv"])
@pytest.mark.parametrize("geom", ADV_GEOMS)
def test_adversarial_softmax_gradients(geom, div):
    """the same construction in every block of a T = 1 flow (feature 0 of both halves): log-prob, z, the inverse and the
    training gradients, whose backward rebuilds P from the forward's m and Z"""
    d, latent, k, t = 8, 64, 2, 1
    h = d // 2
    rng = np.random.default_rng(22)
    p = R.make_graph_attn_grevnet_params(23, h, latent, k, t, final_scale=0.25, kq_dim_division=div, **GEOMS[geom][0])
    nn, ne, s, r = _batch(ADV_SIZES, rng)
    x = (rng.standard_normal((int(nn.sum()), d)) * 0.8).astype(np.float32)
    xa, xb = x[:, :h].copy(), x[:, h:].copy()
    for m in p["s"][0] + p["s"][1] + p["t"][0] + p["t"][1]:
        _make_adversarial(m["attn"], xa, 0, div)
        _make_adversarial(m["attn"], xb, 0, div)
    x = np.concatenate([xa, xb], axis=1)
    _adversarial_logits_hold(p["s"][0][0]["attn"], xa, 0, GEOMS[geom][1], div)
    _adversarial_logits_hold(p["s"][0][0]["attn"], xb, 0, GEOMS[geom][1], div)
    _check_flow(_net(p, d, latent, k, t), nn, ne, s, r, x, p, t, per_graph=True)
    _train_check(p, nn, ne, s, r, x, d, latent, k, t, per_graph=True)


# ---- H > 256: k_attn_graph_bwd_dx's second column stripe ---------------------------------------------------------------
@pytest.mark.parametrize("geom", ["I1_8x10_wo", "I4_3x24_20_wo"])
def test_training_gradients_wide_features(geom):
    d, latent, k, t = 600, 64, 2, 1
    rng = np.random.default_rng(31)
    p = R.make_graph_attn_grevnet_params(32, d // 2, latent, k, t, final_scale=0.25, **GEOMS[geom][0])
    nn, ne, s, r = _batch([40, 0, 70, 1, 30], rng)
    x = (rng.standard_normal((int(nn.sum()), d)) * 0.8).astype(np.float32)
    _train_check(p, nn, ne, s, r, x, d, latent, k, t, per_graph=True)


# ---- both backward walks: MLP rows stashed by the forward pass, or recomputed -------------------------------------------
@pytest.mark.parametrize("stash", [True, False], ids=["mlp_stash", "recompute"])
def test_training_gradients_both_walks(stash):
    d, latent, k, t = 8, 64, 2, 2
    p, nn, ne, s, r, x = _problem("I4_3x24_20_wo", "chunk_edges", 41, d, True, t, latent, k, 0.25)

    def setup(tr):
        tr.mlp_stash_max_bytes = None if stash else 0
    tr, _ = _train_check(p, nn, ne, s, r, (x * 0.8).astype(np.float32), d, latent, k, t, per_graph=True, setup=setup)
    if stash:
        assert tr.mlp_stash_declined is None and tr._mlp_stash is not None
    else:
        assert tr.mlp_stash_declined is not None


# ---- whole-graph shards ------------------------------------------------------------------------------------------------
def test_whole_graph_shards_add_up():
    """shard_graph_ids over a batch with empty graphs: each shard's own GraphsTuple (its node_offsets rebuilt from its n_node
    slice) through forward_shard_sums; the shards' sums are the whole batch's"""
    from gnf_amd.flow import forward_shard_sums
    from gnf_amd.sharding import shard_graph_ids
    rng = np.random.default_rng(51)
    d, t = 8, 2
    p = R.make_graph_attn_grevnet_params(52, d // 2, 32, 2, t, final_scale=0.5, **GEOMS["I4_3x24_20_wo"][0])
    nn, ne, s, r = _batch([0, 40, 0, 0, 70, 1, 0, 90, 33, 0, 64, 129, 0], rng)
    n = int(nn.sum())
    x = rng.standard_normal((n, d)).astype(np.float32)
    net = _net(p, d, 32, 2, t)
    z_full, sums_full = forward_shard_sums(net, graph_from_arrays(nn, ne, s, r, x, DEV))
    z_full, sums_full = z_full.cpu().numpy(), sums_full.cpu().numpy()
    shards = shard_graph_ids(nn, ne, 3)
    assert sorted(np.concatenate(shards).tolist()) == list(range(len(nn)))
    off = np.concatenate([[0], np.cumsum(nn)])
    total = np.zeros(3)
    for sh in shards:
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in sh])
        n2, e2, s2, r2 = _batch(nn[sh], rng)
        assert len(n2) == len(sh) and (n2 == 0).any() == (nn[sh] == 0).any()
        z2, sums2 = forward_shard_sums(net, graph_from_arrays(n2, e2, s2, r2, x[rows], DEV))
        np.testing.assert_allclose(z2.cpu().numpy(), z_full[rows], atol=1e-5, rtol=1e-5)
        total += sums2.cpu().numpy()
    assert total[2] == n
    assert abs(total[0] - sums_full[0]) <= 1e-4 * n and abs(total[1] - sums_full[1]) <= 1e-4 * n
    ref = R.log_prob(nn, s, r, x, p, t, activation="relu", per_graph=True)
    lp = (-0.5 * total[1] - 0.5 * d * math.log(2 * math.pi) * n + total[0]) / n
    assert abs(lp - ref["log_prob_xs_per_node"]) <= 1e-4


# ---- tools/fuzz_parity.py --graph -------------------------------------------------------------------------------------
def test_fuzz_parity_graph_scope():
    """24 random graph-scope flows at a fixed seed: forward, inverse and gradients against the oracle"""
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    counts = {}
    for i in range(24):
        res = fz.run_graph_case(i, 0)
        counts[res] = counts.get(res, 0) + 1
    assert sum(v for k_, v in counts.items() if k_.startswith("ok")) >= 20, counts
