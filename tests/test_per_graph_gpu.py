"""Per-graph log-likelihoods from one batched forward pass (gnf_grevnet_per_graph_f32, GRevNet.f_per_graph,
flow.log_prob_per_graph) on the MI355X, against the float64 reference of tests/per_graph_ref.py: every GNN family, every
kernel instance the forward dispatch can take, batch norm with the batch's moments, row strides and guard bands, hipGraph
capture, and the config-2 bench batch.

Tolerances.  Small synthetic cases: what the neighbouring parity tests use for the same shapes (test_parity_gpu.py,
test_graph_attn_gpu.py: 1e-4 on the per-node log-prob, 3e-4 on z; blocks that end in LayerNorm: 1e-4 + 6 x the error of
the CPU fp32 restatement on the same inputs), applied per node of EACH graph.  Full size: PER_GRAPH_FACTOR x e_parent below."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import graph_attn_ref as R
import per_graph_ref as P
from helpers import GuardBanded, graph_from_arrays, make_product_grevnet
from oracle import gnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Full-size tolerance (config-2 bench batch, 2718 nodes, 64 graphs, no batch norm), max over the graphs of
# |log_prob_xs_per_node(g) - float64 reference|:
#   E_PARENT_MEASURED  what the code before this feature can do - each graph run alone through flow.log_prob_terms
#   E_NEW_MEASURED     the one-pass per-graph path on the same batch
# The bound is 2 x e_parent, e_parent measured in the same test run: the factor allows for another summation order of the
# same fp32 terms and nothing more.
E_PARENT_MEASURED = 1.656699e-06   # MI355X, this batch
E_NEW_MEASURED = 1.656699e-06      # the same figure: per row the arithmetic is identical, only the fp64 summation order differs
PER_GRAPH_BOUND_MEASURED = 2.0 * E_PARENT_MEASURED   # = 3.313398e-06: what the assertion below came to on that run
PER_GRAPH_FACTOR = 2.0


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gnf_amd import _abi
    _abi.lib()


@pytest.fixture(autouse=True)
def _options_reset():
    from gnf_amd import _abi
    yield
    for name in ("force_shape", "attn_kernel"):
        _abi.set_option(name, 0)


# ---- batches ---------------------------------------------------------------------------------------------------------
def _with_one_node_graph(nn, ne, s, r):
    """a one-node graph (with its self loop) in front of the batch: every later boundary moves by one row"""
    return (np.concatenate([[1], nn]), np.concatenate([[1], ne]), np.concatenate([[0], np.asarray(s) + 1]).astype(np.int32),
            np.concatenate([[0], np.asarray(r) + 1]).astype(np.int32))


def _batch(dataset, ids, topology="sparse"):
    """dataset graphs (sizes 4 .. 20 on grid_small: boundaries fall inside the 16-row tiles) + a one-node graph"""
    nn, ne, s, r = O.batch_graphs(*dataset, ids)
    if topology == "complete":
        s, r = R.complete_edges(nn)
        ne = np.asarray(nn, np.int64) ** 2
    return _with_one_node_graph(np.asarray(nn, np.int64), np.asarray(ne, np.int64), s, r)


def _gather_ref(nn, s, r, x, p, t, ws, hp, dtype=None):
    """the per-graph reference on the gather formulation (float64 by default; float32 = what fp32 arithmetic costs)"""
    o = P.PerGraphGraphAttn(s, r, nn, dtype=dtype, agg=hp["agg"], combine=hp["combine"], epsilon=hp["epsilon"],
                            activation=hp["activation"])
    return o.per_graph_terms(x, p, t, ws)


def _dense_ref(nn, s, r, x, p, t, ws, hp):
    o = P.PerGraphDense(s, r, int(np.sum(nn)), agg=hp["agg"], combine=hp["combine"], epsilon=hp["epsilon"],
                        activation=hp["activation"])
    return o.per_graph_terms(x, p, t, nn, ws)


def _exact_abs_diff(a, b):
    return abs(Fraction(float(a)) - Fraction(float(b)))


def _check(net, nn, ne, s, r, x, ref, tol=1e-4, z_tol=3e-4):
    """items 1, 3, 4 on one batch: parity per graph, bitwise z / sums against f, reproducible, sum over graphs vs sums"""
    from gnf_amd.flow import log_prob_per_graph, log_prob_terms
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    out = log_prob_per_graph(net, graph)
    gs = net.last_graph_sums.clone()
    sums = net.last_sums.clone()
    z = out["z_graph"].nodes.clone()
    torch.cuda.synchronize()
    num = np.maximum(np.asarray(nn, np.float64), 1.0)
    for key in ("log_det_jacobian", "log_prob_zs", "log_prob_xs"):
        got = out[key].cpu().numpy()
        err = np.abs(got - ref[key]) / num
        print(f"[per-graph] {key}: max per-node error over {len(nn)} graphs {err.max():.3e} (tol {tol:.1e})")
        assert err.max() <= tol, (key, int(err.argmax()), float(err.max()))
    np.testing.assert_allclose(out["log_prob_xs_per_node"].cpu().numpy(), ref["log_prob_xs_per_node"], atol=tol)
    np.testing.assert_array_equal(out["num_nodes"].cpu().numpy(), np.asarray(nn, np.float64))
    np.testing.assert_allclose(z.cpu().numpy(), ref["z"], atol=z_tol, rtol=z_tol)
    # the batch scalars come out of the same call
    assert float(out["batch"]["log_det_jacobian"]) == float(sums[0])
    # item 3: the variant does not change the arithmetic of the flow, and two runs give the same bits
    plain = log_prob_terms(net, graph)
    torch.cuda.synchronize()
    assert torch.equal(plain["z_graph"].nodes, z)
    assert torch.equal(net.last_sums, sums)
    net.f_per_graph(graph)
    torch.cuda.synchronize()
    assert torch.equal(net.last_graph_sums, gs) and torch.equal(net.last_sums, sums)
    # item 4: both sides sum the same fp32 s and z^2 values in different orders
    for col, key in ((0, "log_det_jacobian"), (1, "sumsq")):
        total = float(gs[:, col].sum())
        ref_total = float(np.sum(ref[key]))
        d_sides = _exact_abs_diff(total, float(sums[col]))
        bound = _exact_abs_diff(total, ref_total) + _exact_abs_diff(float(sums[col]), ref_total)
        print(f"[per-graph] sum over graphs vs sums[{col}]: {float(d_sides):.3e}, bound {float(bound):.3e}")
        assert d_sides <= bound, (key, float(d_sides), float(bound))
    return graph, out


def _mp_case(dataset, d, latent, k, t, agg, combine, ws, topology, bn, ids=None):
    hp = dict(D=d, latent=latent, K=k, T=t, agg=agg, combine=combine, epsilon=0.5 if combine == "agg" else 0.0,
              activation="leaky_relu", weight_sharing=ws, use_batch_norm=bn)
    nn, ne, s, r = _batch(dataset, list(range(12)) if ids is None else ids, topology)
    n = int(nn.sum())
    rng = np.random.default_rng(d * 1000 + latent + (7 if bn else 0))
    x = rng.standard_normal((n, d)).astype(np.float32)
    dense = topology == "complete" or agg == "sum"
    p = O.make_grevnet_params(d + k, d // 2, latent, k, t, combine=combine, weight_sharing=ws,
                              final_scale=(0.02 if topology == "complete" else 0.1) if dense and agg == "sum" else 0.3)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    return hp, nn, ne, s, r, x, p


MP_CASES = [
    # D, latent, K, T, agg, combine, weight_sharing, topology
    (2, 16, 3, 2, "mean", "agg", False, "sparse"),
    (64, 64, 3, 2, "sum", "concat", True, "sparse"),
    (100, 48, 2, 2, "sum", "agg", False, "complete"),
    (64, 256, 5, 2, "mean", "concat", False, "complete"),
]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("case", MP_CASES, ids=[f"D{c[0]}_L{c[1]}_{c[4]}_{c[5]}_{c[7]}" for c in MP_CASES])
def test_message_passing_per_graph_parity(grid_small, case, bn, fused):
    d, latent, k, t, agg, combine, ws, topology = case
    hp, nn, ne, s, r, x, p = _mp_case(grid_small, d, latent, k, t, agg, combine, ws, topology, bn)
    ref = _dense_ref(nn, s, r, x, p, t, ws, hp)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _check(net, nn, ne, s, r, x, ref)


def _attn_case(grid_small, community_medium, shape, bn, layer_norm):
    d, latent, k, t, nh, kq, vd, c, concat, div, res, ws = shape
    akw = dict(num_heads=nh, kq_dim=kq, v_dim=vd, out_dim=c, concat=concat, kq_dim_division=div, residual=res)
    if layer_norm:
        akw["layer_norm"] = True
    hp = dict(D=d, latent=latent, K=k, T=t, agg="mean", combine="agg", epsilon=0.0, activation="relu", weight_sharing=ws,
              attn=akw, use_batch_norm=bn)
    nn, ne, s, r = _batch(grid_small, list(range(12))) if d != 64 else _batch(community_medium, [3, 77, 150, 9])
    n = int(nn.sum())
    rng = np.random.default_rng(d * 100 + nh)
    x = (rng.standard_normal((n, d)) * (0.3 if res else 1.0)).astype(np.float32)
    p = O.make_attn_grevnet_params(d + nh, d // 2, latent, k, t, weight_sharing=ws, final_scale=0.3, **akw)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    return hp, nn, ne, s, r, x, p


ATTN_CASES = [
    # D, latent, K, T, heads, kq, v, C, concat, kq_div, residual, ws   (test_parity_gpu.py ATTN_SHAPES)
    (64, 256, 5, 2, 8, 10, 10, 80, True, False, False, False),     # the drivers' defaults: the fused kernel's attention instance
    (20, 48, 2, 1, 3, 7, 5, 20, False, True, False, True),         # no concat, scaled logits, shared nets
]


def _ln_tol(nn, s, r, x, p, t, ws, hp, ref):
    """blocks that end in LayerNorm: |z| grows to ~e^3 over the flow; the bound is the error the CPU fp32 restatement makes
    on the same inputs (x 6) next to the usual 1e-4 - as test_attention_layer_norm_vs_oracle, per node of each graph"""
    r32 = _gather_ref(nn, s, r, x, p, t, ws, hp, dtype=torch.float32)
    num = np.maximum(np.asarray(nn, np.float64), 1.0)
    e32 = max(float((np.abs(r32[k] - ref[k]) / num).max()) for k in ("log_det_jacobian", "log_prob_zs", "log_prob_xs"))
    return 1e-4 + 6.0 * e32


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("layer_norm", [False, True], ids=["no_ln", "layer_norm"])
@pytest.mark.parametrize("shape", ATTN_CASES, ids=[f"D{s[0]}_h{s[4]}" for s in ATTN_CASES])
def test_edge_attention_per_graph_parity(grid_small, community_medium, shape, layer_norm, bn, fused):
    hp, nn, ne, s, r, x, p = _attn_case(grid_small, community_medium, shape, bn, layer_norm)
    t, ws = shape[3], shape[11]
    ref = _dense_ref(nn, s, r, x, p, t, ws, hp)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _check(net, nn, ne, s, r, x, ref, tol=_ln_tol(nn, s, r, x, p, t, ws, hp, ref) if layer_norm else 1e-4)


def _graph_attn_case(kind, bn, d=8, sizes=(1, 15, 17, 63, 5, 30)):
    nn = np.asarray(sizes, np.int64)
    rng = np.random.default_rng(41 + d)
    ss, rr, ne, off = [], [], [], 0
    for m in nn:   # a random sparse edge list: the graph scope ignores it
        e = int(rng.integers(0, 3 * m + 1))
        ss.append(rng.integers(0, m, e) + off), rr.append(rng.integers(0, m, e) + off), ne.append(e)
        off += m
    s, r = np.concatenate(ss).astype(np.int32), np.concatenate(rr).astype(np.int32)
    kw = dict(num_heads=8, kq_dim=10, v_dim=10, out_dim=80) if kind == "multihead" else dict(num_heads=1, kq_dim=16, v_dim=16)
    k, t, latent = 3, 2, 64
    p = R.make_graph_attn_grevnet_params(17, d // 2, latent, k, t, final_scale=0.3, **kw)
    if bn:
        p["bn"] = O.make_bn_params(d + 3, d // 2, t)
    x = rng.standard_normal((int(nn.sum()), d)).astype(np.float32)
    return R.hp_of(p, d, latent, k, t), nn, np.asarray(ne, np.int64), s, r, x, p, t


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("kind", ["self_attn", "multihead"])
def test_graph_scope_attention_per_graph_parity(kind, bn, fused):
    hp, nn, ne, s, r, x, p, t = _graph_attn_case(kind, bn)
    ref = _gather_ref(nn, s, r, x, p, t, False, hp)
    net = make_product_grevnet(hp, p)
    net.fused = fused
    _check(net, nn, ne, s, r, x, ref)


# ---- item 2: every kernel instance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("shape", [12, 22, 11, 21, 10, 30, 40])
def test_forced_shapes_message_passing(community_medium, shape, bn):
    """the fused shapes (12 / 22: coupling in k_half_fused; 11 / 21: one net per workgroup + k_coupling / k_coupling_rows)
    and the large-batch kernel with 1 / 3 / 4 row tiles per workgroup at most, on a batch of 9 row tiles"""
    from gnf_amd import _abi
    hp, nn, ne, s, r, x, p = _mp_case(community_medium, 64, 256, 5, 2, "mean", "agg", False, "sparse", bn, ids=[3, 77, 150, 9])
    ref = _dense_ref(nn, s, r, x, p, 2, False, hp)
    net = make_product_grevnet(hp, p)
    _abi.set_option("force_shape", shape)
    _check(net, nn, ne, s, r, x, ref)


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
@pytest.mark.parametrize("attn_kernel", [1, 2, 3])
def test_forced_attention_kernels(grid_small, community_medium, attn_kernel, bn):
    """the front-end kept out of the fused kernel's prologue: the MLP kernel reads h0 from memory, same epilogue"""
    from gnf_amd import _abi
    hp, nn, ne, s, r, x, p = _attn_case(grid_small, community_medium, ATTN_CASES[0], bn, False)
    ref = _dense_ref(nn, s, r, x, p, 2, False, hp)
    net = make_product_grevnet(hp, p)
    _abi.set_option("attn_kernel", attn_kernel)
    _check(net, nn, ne, s, r, x, ref)


@pytest.mark.parametrize("shape", [22, 40])
def test_forced_shapes_edge_attention_residual(grid_small, community_medium, shape):
    """residual blocks add x_cond to s in the epilogue: the row sums must carry it (32-row shape, large-batch kernel)"""
    from gnf_amd import _abi
    sh = (20, 48, 2, 1, 3, 7, 5, 20, False, True, True, True)   # (test_parity_gpu.py ATTN_SHAPES: residual, shared nets)
    hp, nn, ne, s, r, x, p = _attn_case(grid_small, community_medium, sh, False, False)
    ref = _dense_ref(nn, s, r, x, p, 1, True, hp)
    net = make_product_grevnet(hp, p)
    _abi.set_option("force_shape", shape)
    _check(net, nn, ne, s, r, x, ref)


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
def test_wide_nets_on_the_layered_path(grid_small, bn):
    """the data driver's 2048 x 3 nets at D = 200: too wide for the fused kernels - the wide-layer GEMMs, the last layer's
    partial-product slabs, k_coupling (plain) / k_coupling_rows (batch norm)"""
    hp, nn, ne, s, r, x, p = _mp_case(grid_small, 200, 2048, 3, 2, "mean", "agg", False, "sparse", bn)
    ref = _dense_ref(nn, s, r, x, p, 2, False, hp)
    net = make_product_grevnet(hp, p)
    _check(net, nn, ne, s, r, x, ref)


def test_split_row_tiles_of_the_large_batch_kernel():
    """a config-4 batch whose even deal splits row tiles between two workgroups (where this device's CU count gives it any):
    the workgroup that couples a split tile writes its rows' sums.  z bitwise the 32-row shape's, the per-graph values up
    to the order of the row sums' additions (fp64: 1e-9 relative is generous)."""
    from gnf_amd import _abi
    from test_fullsize_gpu import _bench_batch
    g_cpu, p, hp = _bench_batch("config4", 53)
    nn = g_cpu.n_node.numpy()
    hp1 = dict(hp, T=1)
    p1 = {k: [[half[0]] for half in p[k]] for k in ("s", "t")}
    net = make_product_grevnet(hp1, p1)
    graph = graph_from_arrays(nn, g_cpu.n_edge.numpy(), g_cpu.senders.numpy(), g_cpu.receivers.numpy(), g_cpu.nodes.numpy(), DEV)
    res = {}
    for shape in (22, 40):
        _abi.set_option("force_shape", shape)
        zg, _ = net.f_per_graph(graph)
        res[shape] = (zg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone())
        plain, _ = net(graph, inverse=True)
        assert torch.equal(plain.nodes, res[shape][0]) and torch.equal(net.last_sums, res[shape][2])
    torch.cuda.synchronize()
    assert torch.equal(res[22][0], res[40][0])
    a, b = res[22][1].cpu().numpy(), res[40][1].cpu().numpy()
    assert np.isfinite(b).all()
    np.testing.assert_allclose(b, a, rtol=1e-9, atol=1e-9)
    assert abs(float(b[:, 0].sum()) - float(res[40][2][0])) <= 1e-9 * max(1.0, abs(float(res[40][2][0])))


# ---- item 5: batch norm ----------------------------------------------------------------------------------------------
def test_batch_norm_uses_the_batch_moments_not_each_graphs(grid_small):
    """per-graph values under batch norm match the reference computed with the BATCH's moments and differ from what each
    graph gives alone (today's only way) - the case that could not be obtained at all"""
    from gnf_amd.flow import log_prob_terms
    hp, nn, ne, s, r, x, p = _mp_case(grid_small, 64, 64, 3, 2, "mean", "agg", False, "sparse", True)
    ref = _dense_ref(nn, s, r, x, p, 2, False, hp)
    net = make_product_grevnet(hp, p)
    _, out = _check(net, nn, ne, s, r, x, ref)
    got = out["log_prob_xs"].cpu().numpy()
    alone = []
    for n1, e1, s1, r1, x1 in P.single_graph_batches(nn, ne, s, r, x):
        alone.append(float(log_prob_terms(net, graph_from_arrays(n1, e1, s1, r1, x1, DEV))["log_prob_xs"]))
    alone = np.asarray(alone)
    big = np.asarray(nn) >= 4   # (a one-node graph alone has variance 0: also different, trivially)
    assert (np.abs(got - alone)[big] / np.asarray(nn, np.float64)[big]).min() > 1e-2
    assert abs(got.sum() - float(out["batch"]["log_prob_xs"])) <= 1e-6 * abs(got.sum())


# ---- item 6: row strides -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(72, 0, 96, 0), (67, 1, 81, 3), (64, 0, 64, 0)], ids=["padded", "misaligned", "dense"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layered"])
def test_row_strides_and_guard_bands(community_medium, layout, fused):
    """ld_src > D, a misaligned base, guard-banded source, destination, sums, graph_out and workspace: nothing outside
    graph_out[0 : 2 n_graphs], x and the workspace is written, and the numbers are those of the contiguous call"""
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_desc, csr_of
    lds_, c0s, ldd, c0d = layout
    hp, nn, ne, s, r, x, p = _mp_case(community_medium, 64, 256, 5, 2, "mean", "agg", False, "sparse", False, ids=[3, 77, 150, 9])
    net = make_product_grevnet(hp, p)
    net.fused = fused
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    zg, _ = net.f_per_graph(graph)
    want_z, want_gs, want_sums = zg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone()
    n, d, b = x.shape[0], 64, len(nn)
    lib = _abi.lib()
    flow = net._flow(d // 2, torch.device(DEV))
    csr = csr_desc(graph, csr_of(graph), True)
    src = GuardBanded(n, d, lds_, c0s, device=DEV, fill=x)
    dst = GuardBanded(n, d, ldd, c0d, device=DEV)
    ws_bytes = lib.gnf_per_graph_workspace_bytes(n, b, d, C.byref(flow))
    # fp64 outputs and the workspace inside sentinel-filled buffers of their own
    outs = torch.full((2 + 2 * b + 64,), float("nan"), dtype=torch.float64, device=DEV)
    sums, gout = outs[16:18], outs[32:32 + 2 * b]
    ws_words = (ws_bytes + 7) // 8
    wsbuf = torch.full((ws_words + 2 * 512,), float("nan"), dtype=torch.float64, device=DEV)
    ws_ptr = wsbuf.data_ptr() + 512 * 8
    with torch.cuda.device(DEV):
        _abi.check(lib.gnf_grevnet_per_graph_f32(C.byref(csr), C.byref(flow), src.ptr(), lds_, dst.ptr(), ldd, d,
                                                 C.c_void_p(sums.data_ptr()), C.c_void_p(gout.data_ptr()), C.c_void_p(ws_ptr),
                                                 ws_bytes, _abi.stream_ptr(torch.device(DEV))), "gnf_grevnet_per_graph_f32")
    torch.cuda.synchronize()
    src.check_guard(), dst.check_guard()
    np.testing.assert_array_equal(src.numpy(), x)                       # the source is read only
    assert torch.isnan(outs[:16]).all() and torch.isnan(outs[18:32]).all() and torch.isnan(outs[32 + 2 * b:]).all()
    assert torch.isnan(wsbuf[:512]).all() and torch.isnan(wsbuf[512 + ws_words:]).all()
    got_z = dst.window.clone()
    if src.aligned() and dst.aligned():   # the same vector / scalar load decisions: the same bits
        assert torch.equal(got_z, want_z) and torch.equal(gout.view(b, 2), want_gs) and torch.equal(sums, want_sums)
    else:   # (other load widths may add a row's neighbours up in another order: the parity tests' tolerances)
        np.testing.assert_allclose(got_z.cpu().numpy(), want_z.cpu().numpy(), atol=3e-4, rtol=3e-4)
        err = (gout.view(b, 2) - want_gs).abs().cpu().numpy() / np.maximum(np.asarray(nn, np.float64), 1.0)[:, None]
        assert err[:, 0].max() <= 1e-4 and err[:, 1].max() <= 64 * 3e-4 * 10, err.max(axis=0)


def test_missing_node_offsets_is_an_error_before_any_launch(grid_small):
    from gnf_amd import _abi
    from gnf_amd.graphs import csr_of
    hp, nn, ne, s, r, x, p = _mp_case(grid_small, 8, 16, 2, 1, "mean", "agg", False, "sparse", False)
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    lib = _abi.lib()
    flow = net._flow(4, torch.device(DEV))
    out = torch.full((x.shape[0], 8), 7.0, device=DEV)
    buf = torch.zeros(4 + 2 * len(nn), dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.gnf_per_graph_workspace_bytes(x.shape[0], len(nn), 8, C.byref(flow)), dtype=torch.uint8, device=DEV)
    rc = lib.gnf_grevnet_per_graph_f32(C.byref(csr_of(graph).desc), C.byref(flow), _abi.ptr(graph.nodes), 8, _abi.ptr(out), 8, 8,
                                       C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 32), _abi.ptr(ws), ws.numel(),
                                       _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == -1 and "node_offsets" in lib.gnf_last_error().decode()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(buf.abs().max()) == 0.0


def test_empty_batch_and_empty_graphs(grid_small):
    """n_nodes == 0 leaves zeros in the n_graphs entries; an empty graph inside a batch gets {0, 0} and 0 per node, not NaN"""
    from gnf_amd.flow import log_prob_per_graph
    hp, nn, ne, s, r, x, p = _mp_case(grid_small, 8, 16, 2, 1, "mean", "agg", False, "sparse", False, ids=[0, 5])
    net = make_product_grevnet(hp, p)
    empty = graph_from_arrays([0, 0, 0], [0, 0, 0], np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 8), np.float32), DEV)
    out = log_prob_per_graph(net, empty)
    torch.cuda.synchronize()
    assert out["log_prob_xs"].shape == (3,) and float(out["log_prob_xs"].abs().max()) == 0.0
    assert float(out["log_prob_xs_per_node"].abs().max()) == 0.0 and float(net.last_sums.abs().max()) == 0.0
    # an empty graph between two real ones
    nn2, ne2 = np.array([nn[0], nn[1], 0, nn[2]]), np.array([ne[0], ne[1], 0, ne[2]])
    ref = _dense_ref(nn2, s, r, x, p, 1, False, hp)
    _, out = _check(net, nn2, ne2, s, r, x, ref)
    assert float(out["log_prob_xs"][2]) == 0.0 and float(out["log_prob_xs_per_node"][2]) == 0.0


# ---- item 7: capture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn", [False, True], ids=["plain", "batch_norm"])
def test_f_per_graph_captured_and_replayed_with_new_node_values(community_medium, bn):
    hp, nn, ne, s, r, x, p = _mp_case(community_medium, 64, 256, 5, 2, "mean", "agg", False, "sparse", bn, ids=[3, 77, 150, 9, 20, 21])
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    x1 = graph.nodes.clone()
    x2 = torch.as_tensor(np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)).to(DEV)
    eager = {}
    for name, xv in (("x1", x1), ("x2", x2)):
        graph.nodes.copy_(xv)
        zg, ld = net.f_per_graph(graph)      # (also the first launches: caches, per-device kernel attributes)
        eager[name] = (zg.nodes.clone(), net.last_graph_sums.clone(), net.last_sums.clone())
    assert float((eager["x1"][1] - eager["x2"][1]).abs().max()) > 0
    graph.nodes.copy_(x1)
    torch.cuda.synchronize()
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        z_c, ld_c = net.f_per_graph(graph, sums)
        gs_c = net.last_graph_sums
    for name, xv in (("x2", x2), ("x1", x1), ("x2", x2)):
        graph.nodes.copy_(xv)
        z_c.nodes.zero_(), gs_c.zero_(), sums.zero_()
        cg.replay()
        torch.cuda.synchronize()
        z_e, gs_e, s_e = eager[name]
        assert torch.equal(z_c.nodes, z_e), name
        assert torch.equal(gs_c, gs_e), name
        assert torch.equal(sums, s_e), name


# ---- item 8 and the tolerance of the per-graph value: the config-2 bench batch -------------------------------------
def test_config2_bench_batch_per_graph_within_twice_the_single_graph_error():
    """2718 nodes, 64 graphs, no batch norm.  e_parent = max_g |log_prob_xs_per_node(g) - reference| with each graph run
    ALONE through flow.log_prob_terms (all the code before this feature can do); the one-pass per-graph path must stay
    within PER_GRAPH_FACTOR x e_parent on the same batch.  Measured on the MI355X: see E_PARENT_MEASURED / E_NEW_MEASURED."""
    from gnf_amd.flow import log_prob_per_graph, log_prob_terms
    from test_fullsize_gpu import _bench_batch
    g_cpu, p, hp = _bench_batch()
    assert g_cpu.nodes.shape[0] == 2718 and g_cpu.n_node.shape[0] == 64
    x = g_cpu.nodes.numpy()
    s, r = g_cpu.senders.numpy(), g_cpu.receivers.numpy()
    nn, ne = g_cpu.n_node.numpy(), g_cpu.n_edge.numpy()
    ref = _gather_ref(nn, s, r, x, p, hp["T"], False, hp)
    net = make_product_grevnet(hp, p)
    graph = graph_from_arrays(nn, ne, s, r, x, DEV)
    out = log_prob_per_graph(net, graph)
    torch.cuda.synchronize()
    new = out["log_prob_xs_per_node"].cpu().numpy()
    alone = []
    for n1, e1, s1, r1, x1 in P.single_graph_batches(nn, ne, s, r, x):
        alone.append(float(log_prob_terms(net, graph_from_arrays(n1, e1, s1, r1, x1, DEV))["log_prob_xs_per_node"]))
    e_parent = float(np.abs(np.asarray(alone) - ref["log_prob_xs_per_node"]).max())
    e_new = float(np.abs(new - ref["log_prob_xs_per_node"]).max())
    print(f"[per-graph] config-2: e_parent {e_parent:.6e}  e_new {e_new:.6e}  bound {PER_GRAPH_FACTOR * e_parent:.6e}")
    # the batch's own figures, as everywhere else
    assert abs(float(out["batch"]["log_prob_xs_per_node"]) - float(np.sum(ref["log_prob_xs"])) / 2718.0) <= 1e-4
    np.testing.assert_allclose(out["z_graph"].nodes.cpu().numpy(), ref["z"], atol=5e-4, rtol=5e-4)
    plain = log_prob_terms(net, graph)
    assert torch.equal(plain["z_graph"].nodes, out["z_graph"].nodes)
    assert e_new <= PER_GRAPH_FACTOR * e_parent, (e_new, e_parent)
