"""Graph-scope attention GNNs (MultiheadSelfAttention / SelfAttention, reference gnn.py:576-738) on the MI355X:
forward, inverse and per-node log-prob against the float64 restatement (tests/graph_attn_ref.py), the edge list ignored
bitwise, agreement with the edge family on complete graphs, training gradients, the block alone, hipGraph capture,
checkpoints and run_grevnet.py --make_gnn_fn multihead_self_attn."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import graph_attn_ref as R
from helpers import graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 15, 17, 63, 65, 100, 300]
RUN_GREVNET = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80)    # run_grevnet.py:74-77
DATA_DRIVER = dict(num_heads=1, kq_dim=64, v_dim=64)                # train_grevnet_with_data.py:40-46 (SelfAttention)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


def _batch(n_node, rng, edges="sparse"):
    """n_node graphs with a random sparse edge list (or none, or complete with self loops): the edges must not matter"""
    n_node = np.asarray(n_node, np.int64)
    if edges == "complete":
        s, r = R.complete_edges(n_node)
        ne = n_node * n_node
    else:
        ss, rr, ne, off = [], [], [], 0
        for nn in n_node:
            e = 0 if edges == "none" else int(rng.integers(0, 3 * nn + 1))
            ss.append(rng.integers(0, nn, e) + off)
            rr.append(rng.integers(0, nn, e) + off)
            ne.append(e)
            off += nn
        s, r = np.concatenate(ss).astype(np.int32), np.concatenate(rr).astype(np.int32)
        ne = np.asarray(ne, np.int64)
    return n_node, np.asarray(ne, np.int64), s, r


def _net(p, d, latent, k, t, ws=False):
    return make_product_grevnet(R.hp_of(p, d, latent, k, t, ws), p)


def _check_flow(net, nn, ne, s, r, x, p, t, ws=False, lp_tol=1e-4, z_tol=3e-4, per_graph=False):
    """per_graph: the oracle's block-diagonal form (large batches; the same numbers as the dense one)"""
    from gnf_amd.flow import log_prob_terms
    n, d = x.shape
    ref = R.log_prob(nn, s, r, x, p, t, ws, activation="relu", per_graph=per_graph)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    out = log_prob_terms(net, graph)
    torch.cuda.synchronize()
    assert abs(float(out["log_prob_xs_per_node"]) - ref["log_prob_xs_per_node"]) <= lp_tol
    z = out["z_graph"].nodes.cpu().numpy()
    np.testing.assert_allclose(z, ref["z"], atol=z_tol, rtol=z_tol)
    if "bn" not in p:   # (with batch norm the inverse de-normalises with the moving statistics: not f's inverse)
        back = net(out["z_graph"], inverse=False).nodes.cpu().numpy()
        np.testing.assert_allclose(back, x, atol=z_tol, rtol=z_tol)
    zs = np.random.default_rng(5).standard_normal((n, d)).astype(np.float32)
    xg = net(graph.replace(nodes=torch.as_tensor(zs).to(DEV)), inverse=False).nodes.cpu().numpy()
    np.testing.assert_allclose(xg, R.inverse(nn, s, r, zs, p, t, ws, activation="relu", per_graph=per_graph), atol=z_tol,
                               rtol=z_tol)
    return graph


@pytest.mark.parametrize("fused", [True, False], ids=["packed", "raw_weights"])
@pytest.mark.parametrize("case", ["multihead", "multihead_ln_bn", "single_ws", "single_bn"])
def test_forward_inverse_log_prob(case, fused):
    rng = np.random.default_rng(len(case) * 7 + 1)
    ws = case.endswith("_ws")
    if case.startswith("multihead"):
        d, kw = 2, dict(RUN_GREVNET, layer_norm="ln" in case)
    else:
        d, kw = 8, dict(num_heads=1, kq_dim=12, v_dim=20)
    t = 2
    p = R.make_graph_attn_grevnet_params(31, d // 2, 32, 2, t, weight_sharing=ws, final_scale=0.5, **kw)
    if case.endswith("_bn"):
        p["bn"] = O.make_bn_params(32, d // 2, t)
    nn, ne, s, r = _batch(SIZES, rng)
    x = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    net = _net(p, d, 32, 2, t, ws)
    net.fused = fused
    _check_flow(net, nn, ne, s, r, x, p, t, ws)


@pytest.mark.parametrize("geom", [dict(num_heads=64, kq_dim=4, v_dim=4, out_dim=32), dict(num_heads=1, kq_dim=256, v_dim=256, out_dim=16),
                                  dict(num_heads=2, kq_dim=128, v_dim=17, out_dim=24), dict(num_heads=1, kq_dim=64, v_dim=64)],
                         ids=["64_heads", "kq_v_256", "odd_widths", "data_driver_single"])
def test_geometry_edges_of_the_limit(geom):
    rng = np.random.default_rng(3)
    d, t = 6, 1
    p = R.make_graph_attn_grevnet_params(41, d // 2, 32, 2, t, final_scale=0.5, **geom)
    nn, ne, s, r = _batch([17, 65, 100], rng)
    x = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    _check_flow(_net(p, d, 32, 2, t), nn, ne, s, r, x, p, t)


def test_one_graph_of_more_than_a_thousand_nodes():
    rng = np.random.default_rng(4)
    d, t = 4, 1
    p = R.make_graph_attn_grevnet_params(51, d // 2, 32, 2, t, final_scale=0.5, num_heads=2, kq_dim=16, v_dim=16, out_dim=16)
    nn, ne, s, r = _batch([1100], rng)
    x = rng.standard_normal((1100, d)).astype(np.float32)
    _check_flow(_net(p, d, 32, 2, t), nn, ne, s, r, x, p, t)


def test_edges_are_ignored_bitwise():
    from gnf_amd.flow import forward_shard_sums
    rng = np.random.default_rng(6)
    d, t = 2, 2
    p = R.make_graph_attn_grevnet_params(61, 1, 32, 2, t, final_scale=0.5, **RUN_GREVNET)
    n_node = [5, 40, 70]
    x = rng.standard_normal((115, d)).astype(np.float32)
    net = _net(p, d, 32, 2, t)
    outs = []
    for edges in ("none", "complete", "sparse"):
        nn, ne, s, r = _batch(n_node, rng, edges)
        z, sums = forward_shard_sums(net, graph_from_arrays(nn, ne, s, r, x, DEV))
        outs.append((z.clone(), sums[:2].clone()))
    torch.cuda.synchronize()
    for z, sums in outs[1:]:
        assert torch.equal(z, outs[0][0]) and torch.equal(sums, outs[0][1])


def _dm_equivalent(p, heads, ws=False):
    """The edge family's parameters that compute the same flow on complete graphs with self loops: Wq <-> Wk exchanged (the
    edge scope takes q at the sender), Wv = the shared value block, no Wo -> identity for SelfAttention."""
    def conv(m):
        if isinstance(m, dict) and "attn" in m:
            a = m["attn"]
            nv = int(a["v_dim"])
            wv = np.asarray(a["wv"])[:, :nv]
            da = {"num_heads": heads, "kq_dim": a["kq_dim"], "v_dim": nv, "concat": True, "kq_dim_division": a["kq_dim_division"],
                  "residual": False, "wq": a["wk"], "wk": a["wq"], "wv": wv,
                  "wo": a["wo"] if "wo" in a else np.eye(nv, dtype=np.float32)}
            return {"attn": da, "mlp": m["mlp"]}
        return [conv(q) for q in m]
    return {k: conv(v) for k, v in p.items()}


@pytest.mark.parametrize("heads", [8, 1])
def test_agrees_with_dm_self_attn_on_complete_graphs(heads):
    from gnf_amd.flow import forward_shard_sums
    rng = np.random.default_rng(8)
    d, t, latent = 4, 2, 32
    kw = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80) if heads == 8 else dict(num_heads=1, kq_dim=10, v_dim=10)
    p = R.make_graph_attn_grevnet_params(71, d // 2, latent, 2, t, final_scale=0.5, **kw)
    for m in p["s"][0] + p["s"][1] + p["t"][0] + p["t"][1]:   # one value block repeated over the heads
        a = m["attn"]
        a["wv"] = np.tile(np.asarray(a["wv"])[:, :10], (1, heads))
    nn, ne, s, r = _batch([7, 30, 100], rng, "complete")
    x = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    z_g, s_g = forward_shard_sums(_net(p, d, latent, 2, t), graph)
    dm = _dm_equivalent(p, heads)
    a0 = dm["s"][0][0]["attn"]
    hp = dict(D=d, latent=latent, K=2, T=t, agg="sum", combine="agg", epsilon=0.0, activation="relu", weight_sharing=False,
              attn=dict(num_heads=heads, kq_dim=10, v_dim=10, out_dim=int(np.asarray(a0["wo"]).shape[1]), concat=True,
                        kq_dim_division=True, residual=False))
    z_d, s_d = forward_shard_sums(make_product_grevnet(hp, dm), graph)
    torch.cuda.synchronize()
    scale = float(z_d.abs().max())
    assert float((z_g - z_d).abs().max()) <= 1e-5 * max(scale, 1.0)
    assert abs(float(s_g[0] - s_d[0])) <= 1e-4 * int(nn.sum())


def _flat_all(g):
    out = []

    def walk(x, name):
        if isinstance(x, dict):
            for k in sorted(x):
                walk(x[k], f"{name}.{k}")
        elif isinstance(x, (list, tuple)):
            for i, q in enumerate(x):
                walk(q, f"{name}[{i}]")
        else:
            out.append((name, np.asarray(x)))
    walk(g, "")
    return out


def _check_all_grads(got, ref, scale, ref32=None):
    """every tensor within `scale` of its own maximum - or, where single precision itself costs more on these inputs
    (relu kinks, long sums: the same autograd in float32, ref32), within three times what it costs"""
    ga, gb = _flat_all(got), _flat_all(ref)
    g32 = _flat_all(ref32) if ref32 is not None else [(n_, b) for n_, b in gb]
    assert [a for a, _ in ga] == [b for b, _ in gb]
    gmax = max(float(np.abs(b).max()) for _, b in gb)
    for (name, a), (_, b), (_, c) in zip(ga, gb, g32):
        cost32 = float(np.abs(np.asarray(c, np.float64) - b).max())
        tol = max(scale * float(np.abs(b).max()), 3 * cost32) + 1e-5 + 1e-6 * gmax
        err = float(np.abs(np.asarray(a, np.float64) - b).max())
        assert err <= tol, f"{name}: max err {err:.3e} > {tol:.3e} (max|g| {np.abs(b).max():.3e})"


def _train_check(p, nn, ne, s, r, x, d, latent, k, t, ws=False, scale=5e-4, l2=None, per_graph=False, setup=None):
    """per_graph: as in _check_flow; setup(trainer) runs before the step (e.g. to choose the backward walk)"""
    from gnf_amd.train import GRevNetTrainer
    net = _net(p, d, latent, k, t, ws)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    ref = R.loss_and_grads(nn, s, r, x, p, t, ws, activation="relu", per_graph=per_graph)
    tr = GRevNetTrainer(net)
    if setup is not None:
        setup(tr)
    out = tr.loss_and_grads(graph)
    torch.cuda.synchronize()
    n = int(nn.sum())
    assert abs(float(out["total_loss"]) - ref["total_loss"]) <= 1e-4 * n
    np.testing.assert_allclose(out["reconstruction"].cpu().numpy(), x, atol=3e-4, rtol=3e-4)
    r32 = R.loss_and_grads(nn, s, r, x, p, t, ws, activation="relu", dtype=torch.float32, per_graph=per_graph)
    _check_all_grads(tr.named_gradients(), ref["grads"], scale, r32["grads"])
    if l2 is not None:
        gb = _flat_all(ref["grads"])
        gmax = max(float(np.abs(b).max()) for _, b in gb)
        for (name, a), (_, b) in zip(_flat_all(tr.named_gradients()), gb):
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            rel = float(np.linalg.norm(a - b)) / max(float(np.linalg.norm(b)), 1e-3 * gmax * np.sqrt(b.size))
            assert rel <= l2, f"{name}: 2-norm error {rel:.2e} > {l2:.0e}"
    return tr, graph


def test_training_gradients_run_grevnet_defaults():
    """run_grevnet.py's attention defaults (8 heads of 10 / 10, C = 80, kq_dim_division, D = 2) on 4 complete 100-node
    graphs, T = 3.  The MLPs are 64 x 3: at the driver's 256 x 5 relu widths pre-activations within rounding of the kink
    take the other side than in float64 and move whole terms of a weight column (tests/test_fullsize_gpu.py needs a
    kink-aware oracle for the edge family there), which says nothing about the attention."""
    rng = np.random.default_rng(9)
    d, latent, k, t = 2, 64, 3, 3
    p = R.make_graph_attn_grevnet_params(81, 1, latent, k, t, final_scale=0.25, **RUN_GREVNET)
    nn, ne, s, r = _batch([100] * 4, rng, "complete")
    x = rng.standard_normal((400, d)).astype(np.float32)
    _train_check(p, nn, ne, s, r, x, d, latent, k, t)


@pytest.mark.parametrize("case", ["data_driver_literal", "weight_sharing_ln", "single_bn"])
def test_training_gradients(case):
    rng = np.random.default_rng(10)
    if case == "data_driver_literal":   # 1 x 64 / 64, relu 2048 x 3, D = 200, batch norm, two small graphs
        d, latent, k, t, ws = 200, 2048, 3, 1, False
        kw = dict(num_heads=1, kq_dim=64, v_dim=64, out_dim=64)
        sizes = [9, 14]
    elif case == "weight_sharing_ln":
        d, latent, k, t, ws = 4, 64, 2, 3, True
        kw = dict(num_heads=4, kq_dim=6, v_dim=5, out_dim=12, layer_norm=True)
        sizes = [1, 17, 40]
    else:
        d, latent, k, t, ws = 8, 64, 2, 2, False
        kw = dict(num_heads=1, kq_dim=20, v_dim=12)
        sizes = [3, 65, 30]
    p = R.make_graph_attn_grevnet_params(91, d // 2, latent, k, t, weight_sharing=ws, final_scale=0.25, **kw)
    if case != "weight_sharing_ln":
        p["bn"] = O.make_bn_params(92, d // 2, t)
    nn, ne, s, r = _batch(sizes, rng)
    x = (rng.standard_normal((int(nn.sum()), d)) * 0.8).astype(np.float32)
    _train_check(p, nn, ne, s, r, x, d, latent, k, t, ws)


@pytest.mark.parametrize("single", [False, True], ids=["multihead", "single"])
def test_block_alone(single):
    """gnf_gnn_apply_f32 through the block's own _build"""
    from gnf_amd import gnn
    rng = np.random.default_rng(11)
    h = 5
    kw = dict(num_heads=1, kq_dim=7, v_dim=9) if single else dict(num_heads=3, kq_dim=7, v_dim=9, out_dim=11, layer_norm=True)
    net = R.make_graph_attn_net_params(rng, h, 32, 2, **kw)
    nn, ne, s, r = _batch([4, 33, 70], rng)
    x = rng.standard_normal((int(nn.sum()), h)).astype(np.float32)
    mk = lambda: gnn.make_mlp_model(32, h, 2)
    blk = gnn.self_attn_gnn(7, 9, mk, True) if single else gnn.multihead_self_attn_gnn(7, 9, 11, mk, num_heads=3, layer_norm=True)
    blk.set_attn_params(net["attn"])
    blk._mlp.set_params(net["mlp"])
    out = blk(graph_from_arrays(nn, ne, s, r, x, DEV)).nodes.cpu().numpy()
    o = R.GraphAttnGather(s, r, nn, activation="relu")
    want = o.attn_gnn(o.to_t(x), o.prep_params({"n": [net]})["n"][0]).numpy()
    np.testing.assert_allclose(out, want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=1e-4)


def test_hipgraph_capture_replays_bitwise():
    from gnf_amd.flow import forward_shard_sums
    from gnf_amd.graphs import csr_of
    from gnf_amd.train import GRevNetTrainer
    rng = np.random.default_rng(12)
    d, t = 4, 2
    p = R.make_graph_attn_grevnet_params(101, 2, 64, 3, t, final_scale=0.25, num_heads=4, kq_dim=8, v_dim=8, out_dim=16)
    nn, ne, s, r = _batch([20, 100, 45], rng)
    x1 = rng.standard_normal((165, d)).astype(np.float32)
    x2 = rng.standard_normal((165, d)).astype(np.float32)
    graph = graph_from_arrays(nn, ne, s, r, x1, DEV)
    x1, x2 = graph.nodes.clone(), torch.as_tensor(x2).to(DEV)
    net = _net(p, d, 64, 3, t)
    tr = GRevNetTrainer(net)
    eager = {}
    for name, x in (("x1", x1), ("x2", x2)):
        graph.nodes.copy_(x)
        z, s3 = forward_shard_sums(net, graph)
        back = net(graph.replace(nodes=z), inverse=False).nodes
        out = tr.loss_and_grads(graph)
        torch.cuda.synchronize()
        eager[name] = (z.clone(), s3.clone(), back.clone(), tr.grad.clone(), out["total_loss"].clone())
    graph.nodes.copy_(x1)
    csr_of(graph), csr_of(graph, by_sender=True)
    torch.cuda.synchronize()
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        z_c, _ = forward_shard_sums(net, graph, sums)
        back_c = net(graph.replace(nodes=z_c), inverse=False).nodes
        out_c = tr.loss_and_grads(graph)
    for name, x in (("x2", x2), ("x1", x1)):
        graph.nodes.copy_(x)
        tr.grad.zero_()
        cg.replay()
        torch.cuda.synchronize()
        z_e, s_e, b_e, g_e, l_e = eager[name]
        assert torch.equal(z_c, z_e) and torch.equal(sums[:2], s_e[:2]) and torch.equal(back_c, b_e), name
        assert torch.equal(tr.grad, g_e) and torch.equal(out_c["total_loss"], l_e), name


@pytest.mark.parametrize("single", [False, True], ids=["multihead", "single"])
def test_checkpoint_round_trip(tmp_path, single):
    from gnf_amd.train import GRevNetTrainer, load_checkpoint, save_checkpoint
    rng = np.random.default_rng(13)
    d, t = 4, 2
    kw = dict(num_heads=1, kq_dim=6, v_dim=6) if single else dict(num_heads=2, kq_dim=6, v_dim=6, out_dim=8)
    p = R.make_graph_attn_grevnet_params(111, 2, 32, 2, t, final_scale=0.25, **kw)
    nn, ne, s, r = _batch([10, 30], rng)
    x = rng.standard_normal((40, d)).astype(np.float32)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    tr = GRevNetTrainer(_net(p, d, 32, 2, t))
    tr.step(graph)
    tr.step(graph)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(tr, path)
    tr2 = GRevNetTrainer(_net(p, d, 32, 2, t))
    tr2.loss_and_grads(graph)   # (connects the trainer: its variables exist)
    load_checkpoint(tr2, path)
    a, b = tr.step(graph), tr2.step(graph)
    torch.cuda.synchronize()
    assert torch.equal(tr.theta, tr2.theta)
    assert float(a["total_loss"]) == float(b["total_loss"])


def test_run_grevnet_multihead_self_attn_trains():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_grevnet.py"), "--make_gnn_fn", "multihead_self_attn",
           "--num_train_iters", "3"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    losses = [float(w) for line in res.stdout.splitlines() for w in line.replace(",", " ").split()
              if "loss" in line.lower() and _is_float(w)]
    assert losses and all(np.isfinite(losses)), res.stdout[-2000:]


def _is_float(w):
    try:
        float(w)
        return True
    except ValueError:
        return False
